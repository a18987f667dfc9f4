"""CPU tests of tests/projective_ref.py, the numpy restatement of ann/projective_search.hpp, on hand-built cases whose answers follow from
the reference's text alone; and of the projective search's presence in the C-ABI and the Python package (no GPU needed)."""
import ctypes
import os

import numpy as np

import projective_ref as pr

W, H = 16, 8


def at(u, v, r=5.0, W=W, H=H):
    """A point of range r whose projection is the centre of pixel (u, v): the inverse of projective_search.hpp:13-27."""
    lon = ((u + 0.5) / W - 0.5) * 2.0 * np.pi
    lat = ((v + 0.5) / H - 0.5) * np.pi
    return np.array([r * np.cos(lat) * np.sin(lon), -r * np.sin(lat), r * np.cos(lat) * np.cos(lon)])


def cloud(*pts):
    return np.asarray(pts, dtype=np.float32)


def search(tgt, q, k=1, W=W, H=H, **kw):
    img, _ = pr.build(tgt, np.zeros(3), W, H)
    return pr.knn(img, tgt, np.zeros(3), np.atleast_2d(np.asarray(q, dtype=np.float64)), k, **kw)


def test_pixel_of_constructed_points():
    pts = np.array([at(u, v) for u in range(W) for v in range(H)])
    u, v, finite, amb = pr.pixel(pts, W, H)
    assert finite.all() and not amb.any()
    assert (u == np.repeat(np.arange(W), H)).all() and (v == np.tile(np.arange(H), W)).all()


def test_axes_are_camera_convention():
    # z forward -> the image centre, y (down) > 0 -> smaller v (lat = -asin(b.y)), x (right) > 0 -> larger u
    u, v, _, _ = pr.pixel(np.array([[0.0, 0.0, 1.0], [0.0, 0.9, 0.1], [0.9, 0.0, 0.1]]), W, H)
    assert (u[0], v[0]) == (W // 2, H // 2)
    assert v[1] < H // 2 and u[1] == W // 2
    assert u[2] > W // 2 and v[2] == H // 2


def test_seam_u_equals_width_is_dropped():
    # lon = +pi exactly: uv.x = 1, u = W, out of range (projective_search.hpp:58-60); -0.0 gives lon = -pi, u = 0
    img, _ = pr.build(cloud([0.0, 0.0, -3.0], [-0.0, 0.0, -3.0]), np.zeros(3), W, H)
    assert (img != pr.INVALID).sum() == 1
    assert img[H // 2, 0] == 1


def test_seam_wrap_repeat_and_clamp():
    tgt = cloud(at(W - 1, 3), at(6, 3))
    i, d, _ = search(tgt, at(0, 3), wh=2, wv=1)
    assert i[0, 0] == 0  # across the seam
    i, d, _ = search(tgt, at(0, 3), wh=2, wv=1, repeat_h=False)
    assert i[0, 0] == -1 and np.isinf(d[0, 0])


def test_pole_rows_are_skipped_not_clamped():
    tgt = cloud(at(4, 0))
    i, _, _ = search(tgt, at(4, 0), k=8, wh=0, wv=5)
    assert list(i[0]) == [0] + [-1] * 7  # a clamp would push row 0 six times
    tgt = cloud(at(4, H - 1))
    i, _, _ = search(tgt, at(4, 0), wh=0, wv=2)
    assert i[0, 0] == -1  # BorderClamp vertically: no wrap to the bottom row


def test_repeat_vertically_and_clamp_horizontally():
    tgt = cloud(at(4, H - 1))
    i, _, _ = search(tgt, at(4, 0), wh=0, wv=2, repeat_v=True)
    assert i[0, 0] == 0
    i, _, _ = search(tgt, at(4, 0), wh=0, wv=2, repeat_v=False)
    assert i[0, 0] == -1
    tgt = cloud(at(W - 1, 2))
    i, _, _ = search(tgt, at(0, 2), wh=2, wv=0, repeat_h=False, repeat_v=True)
    assert i[0, 0] == -1
    i, _, _ = search(tgt, at(0, 2), wh=2, wv=0, repeat_h=True, repeat_v=True)
    assert i[0, 0] == 0


def test_last_index_wins_a_pixel():
    tgt = cloud(at(5, 5, r=4.0), at(5, 5, r=9.0), at(5, 5, r=6.0))
    img, _ = pr.build(tgt, np.zeros(3), W, H)
    assert img[5, 5] == 2 and (img != pr.INVALID).sum() == 1
    i, _, _ = search(tgt, at(5, 5, r=4.0), k=3)
    assert list(i[0]) == [2, -1, -1]  # the nearer point 0 is gone from the image


def test_near_origin_point_goes_to_the_centre():
    img, _ = pr.build(cloud([0.01, -0.02, 0.0]), np.zeros(3), W, H)
    assert img[H // 2, W // 2] == 0
    u, v, _, _ = pr.pixel(np.array([[0.0, 0.0, 0.0]]), W, H)
    assert (u[0], v[0]) == (W // 2, H // 2)


def test_non_finite_points_are_skipped():
    tgt = cloud(at(3, 3), [np.nan, 1.0, 1.0], [np.inf, 0.0, 1.0], at(4, 3))
    img, _ = pr.build(tgt, np.zeros(3), W, H)
    assert sorted(img[img != pr.INVALID].tolist()) == [0, 3]
    i, _, _ = search(tgt, [np.nan, 0.0, 1.0])
    assert i[0, 0] == -1


def test_first_in_scan_order_wins_a_tie():
    # equidistant from the origin query (pixel (W/2, H/2)); the point with x < 0 has the smaller u and is scanned first (du outer)
    tgt = cloud([1.0, 0.0, 3.0], [-1.0, 0.0, 3.0])
    i, d, _ = search(tgt, [0.0, 0.0, 0.0], k=2)
    assert d[0, 0] == d[0, 1]
    assert list(i[0]) == [1, 0]
    tgt = cloud([1.0, -1.0, 3.0], [1.0, 1.0, 3.0])  # the same column: dv inner, the smaller v (y > 0, below the horizon) first
    u, v, _, _ = pr.pixel(tgt.astype(np.float64), W, H)
    assert u[0] == u[1] and v[1] < v[0]
    i, _, _ = search(tgt, [1.0, 0.0, 3.0])
    assert i[0, 0] == 1
    i, _, _ = search(tgt[::-1].copy(), [1.0, 0.0, 3.0])
    assert i[0, 0] == 0


def test_knn_keeps_duplicates_of_a_column_visited_twice():
    # W = 8 < 2 h + 1 = 21, query column 0: u + du = -10 .. 10 wraps once, so column 1 is reached at du = -7, 1 and 9
    w8 = 8
    tgt = cloud(at(1, 2, W=w8))
    i, d, _ = search(tgt, at(0, 2, W=w8), k=4, W=w8, wh=10, wv=0)
    assert list(i[0]) == [0, 0, 0, -1]
    assert d[0, 0] == d[0, 1] == d[0, 2]


def test_knn_order_and_max_sq_filter():
    tgt = cloud(at(5, 4, r=5.0), at(6, 4, r=5.5), at(4, 4, r=7.0))
    i, d, _ = search(tgt, at(5, 4, r=5.2), k=3)
    assert list(i[0]) == [0, 1, 2]
    assert (np.diff(d[0]) >= 0).all()
    img, _ = pr.build(tgt, np.zeros(3), W, H)
    i2, d2, _ = pr.knn(img, tgt, np.zeros(3), np.atleast_2d(at(5, 4, r=5.2)), 3, max_sq=float(d[0, 1]))
    assert list(i2[0]) == [0, 1, -1] and np.isinf(d2[0, 2])


def test_origin_enters_the_projection():
    # the same records in a device frame 1 km away project elsewhere: the projection adds the origin back
    rec = cloud(at(3, 3))
    o = np.array([1024.0, 0.0, 0.0])
    a, _ = pr.build(rec, np.zeros(3), W, H)
    b, _ = pr.build(rec - o.astype(np.float32), o, W, H)
    assert (a == b).all()
    c, _ = pr.build(rec, o, W, H)
    assert not (a == c).all()


def test_ambiguity_flag():
    lon = (3.0 / W - 0.5) * 2.0 * np.pi  # on the border between columns 2 and 3, to rounding
    _, _, _, amb = pr.pixel(np.array([[np.sin(lon), 0.3, np.cos(lon)], [1.0, 0.3, 2.0], [0.0, 0.0, 1.0], [0.7, 0.0, 0.0]]), W, H)
    assert amb[0] and not amb[1]
    assert not amb[2] and not amb[3]  # exact on every platform: atan2(0, z), atan2(x, 0), asin(0)


def test_c_abi_and_python_surface():
    import small_gicp_amd
    from small_gicp_amd._lib import SYMBOLS

    names = {s[0] for s in SYMBOLS}
    for name in ("sga_index_build_projective", "sga_projective_set_search_window", "sga_projective_set_border_modes", "sga_projective_download_map", "sga_projective_get_params"):
        assert name in names
    assert small_gicp_amd.ProjectiveSearch.__init__.__defaults__ == (10, 5, "repeat", "clamp")
    lib = ctypes.CDLL(small_gicp_amd.LIB_PATH)
    for name in names:
        getattr(lib, name)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "small_gicp_amd.h")).read()
    assert "sga_index_build_projective(sga_context* ctx, const sga_cloud* cloud, int width, int height, sga_index** out)" in hdr

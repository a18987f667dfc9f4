"""The restatement of the global registration (tests/global_ref.py) on cases small enough to work out by hand:
what the GPU tests of tests/test_global_registration_gpu.py compare against must itself say what the header says.  No device."""
import numpy as np
import pytest

import global_ref as ref

F32 = np.float32
Z = np.array([0.0, 0.0, 1.0])


def test_two_points_on_a_plane_with_equal_normals():
    # p1 - p0 along x, both normals +z: a1 = a2 = 0 (no swap), v = x cross z = -y, w = z cross -y = x, alpha = 0, theta = atan2(0, 1) = 0
    p = np.array([[0, 0, 0], [1, 0, 0]], F32)
    n = np.array([Z, Z], F32)
    counted, theta, alpha, phi, shaky = ref.pair_features(p[0].astype(float), Z, p[1].astype(float), Z)
    assert counted and theta == 0.0 and alpha == 0.0 and phi == 0.0
    assert not shaky  # |a1| == |a2| between EQUAL normals: exact in any arithmetic, no swap
    assert ref.pair_features(p[0].astype(float), Z, p[1].astype(float), np.array([0.0, 0.6, 0.8]))[4]  # a1 = a2 = 0 between different normals hangs on an ulp
    assert [int(ref.bins(c)) for c in ref.bin_coordinates(theta, alpha, phi)] == [5, 5, 5]
    r = ref.fpfh(p, n, 2)
    want = np.zeros(33)
    want[[5, 16, 27]] = 100.0
    assert np.array_equal(r["spfh"], [want, want])
    assert np.allclose(r["rows"], [want, want], rtol=0, atol=1e-12)  # SPFH + 1 x SPFH, rescaled to 100
    assert not r["band"].any()


def test_the_swap():
    # n_i = z, n_j tilted towards the line of sight: |a1| = 0 < |a2|, so j becomes the origin of the frame and d turns round
    pi, pj = np.zeros(3), np.array([1.0, 0.0, 0.0])
    nj = np.array([0.6, 0.0, 0.8])
    counted, theta, alpha, phi, shaky = ref.pair_features(pi, Z, pj, nj)
    assert counted and not shaky
    assert phi == pytest.approx(-0.6, abs=1e-15)  # -a2
    # n1 = nj, d = -x: v = (-x) cross nj = (0, 0.8, 0) -> y; w = nj cross y = (-0.8, 0, 0.6); n2 = z
    assert alpha == pytest.approx(0.0, abs=1e-15) and theta == pytest.approx(np.arctan2(0.6, 0.8), abs=1e-15)
    # without the swap the same pair reads differently
    c2, t2, a2, p2, _ = ref.pair_features(pj, nj, pi, Z)  # seen from j: a1 = nj . (-x) = -0.6, a2 = 0: no swap, the same frame
    assert c2 and p2 == pytest.approx(-0.6, abs=1e-15) and t2 == pytest.approx(theta, abs=1e-15) and a2 == pytest.approx(alpha, abs=1e-15)


def test_coincident_points_are_skipped_and_weigh_nothing():
    p = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    n = np.tile(np.array([0.0, 0.6, 0.8], F32), (4, 1))
    r = ref.fpfh(p, n, 3)
    # point 0 has three neighbours, one of them coincident: two pairs counted, each a share of 50
    assert sorted(r["spfh"][0][:11][r["spfh"][0][:11] > 0].tolist()) in ([50.0, 50.0], [100.0])
    assert r["spfh"][0][:11].sum() == 100.0 and r["spfh"][0][11:22].sum() == 100.0 and r["spfh"][0][22:].sum() == 100.0
    assert np.array_equal(r["spfh"][0], r["spfh"][1])  # the twin sees the same pairs
    assert np.isfinite(r["rows"]).all()
    idx, d2, _ = ref.neighbours(p, 3)
    assert idx[0, 0] == 1 and d2[0, 0] == 0.0  # the twin is the nearest OTHER record, at distance 0


def test_a_sub_histogram_that_stays_zero():
    # every normal is zero: v = d cross 0 = 0, every pair is skipped, nothing is counted
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F32)
    r = ref.fpfh(p, np.zeros((3, 3), F32), 2)
    assert not r["spfh"].any() and not r["rows"].any()
    assert not ref.fpfh(p[:1], np.zeros((1, 3), F32), 5)["rows"].any()  # n = 1: a zero row
    assert ref.fpfh(p[:0], np.zeros((0, 3), F32), 5)["rows"].shape == (0, 33)


def test_the_viewpoint_turns_normals_without_writing_them():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0.2]], F32)
    n = np.array([Z, -Z, Z, -Z], F32)
    up = ref.fpfh(p, n, 3, viewpoint=(0, 0, 10))
    same = ref.fpfh(p, np.abs(n), 3)
    assert np.array_equal(up["rows"], same["rows"])
    far = ref.fpfh(p, n, 3, viewpoint=(1280, 0, 10), origin=(1280, 0, 0))  # the records are relative to the origin
    assert np.array_equal(far["rows"], same["rows"])


def test_rows_sum_to_100_per_sub_histogram():
    rng = np.random.default_rng(3)
    p = rng.uniform(-1, 1, (200, 3)).astype(F32)
    n = rng.normal(size=(200, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(F32)
    r = ref.fpfh(p, n, 10)
    for off in (0, 11, 22):
        assert np.allclose(r["rows"][:, off:off + 11].sum(axis=1), 100.0, rtol=1e-13)
    assert r["band"].sum() <= 2


def test_ties_go_to_the_lowest_index_and_duplicates_are_not_band():
    B = np.array([[1, 0], [0, 1], [1, 0], [5, 5]], F32)
    A = np.array([[1, 0], [0.9, 0.1], [0.5, 0.5], [4, 4]], F32)
    m = ref.match(A, B, mutual=False)
    assert m["match"].tolist() == [0, 0, 0, 3]  # rows 0 and 2 of B are equal: 0 wins; (0.5, 0.5) is equidistant from B0 and B1: 0 wins
    assert m["band"].tolist() == [False, False, True, False]  # ... and only that last tie is between DIFFERENT rows
    assert m["dist"][0] == 0.0 and m["dist"][3] == pytest.approx(np.sqrt(2.0))
    empty = ref.match(A, B[:0], mutual=True)
    assert (empty["match"] == -1).all() and np.isinf(empty["dist"]).all()


def test_the_screened_search_is_the_plain_one():
    rng = np.random.default_rng(8)
    B = rng.uniform(0, 100, (3000, 33)).astype(F32)
    A = np.concatenate([B[rng.integers(0, 3000, 50)] + rng.normal(0, 1.0, (50, 33)).astype(F32), rng.uniform(0, 100, (150, 33)).astype(F32)])
    B[7], B[1200] = B[3], B[3]  # equal rows
    A[0], A[1] = B[3], (B[10].astype(np.float64) + B[20]).astype(F32) / 2  # an exact tie among equal rows; a near tie between different ones
    plain, fast = ref._nearest_rows(A, B, screen=False), ref._nearest_rows(A, B, screen=True)
    assert all(np.array_equal(x, y) for x, y in zip(plain, fast))
    assert plain[0][0] == 3 and plain[1][0] == 0.0 and not plain[2][0]


def test_the_mutual_rule():
    A = np.array([[0.0], [1.0], [10.0]], F32)
    B = np.array([[0.4], [9.0]], F32)
    one = ref.match(A, B, mutual=False)
    assert one["match"].tolist() == [0, 0, 1]
    both = ref.match(A, B, mutual=True)
    assert both["match"].tolist() == [0, -1, 1]  # B0's nearest source row is A0, so A1 loses it
    assert both["dist"][0] == pytest.approx(0.4, rel=1e-6) and np.isinf(both["dist"][1])


def test_the_generator():
    for M in (3, 4, 1000):
        tri = ref.draws(7, np.arange(5000), M)
        assert tri.min() >= 0 and tri.max() < M
        assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 0] != tri[:, 2]).all() and (tri[:, 1] != tri[:, 2]).all()
        assert all(tuple(tri[h]) == ref.draw(7, h, M) for h in range(0, 5000, 97))
        if M == 3:
            assert all(sorted(t) == [0, 1, 2] for t in tri.tolist())
        else:
            assert len({tuple(t) for t in tri.tolist()}) > (20 if M == 4 else 4900)  # every ordered triple of 4 shows up: 24
    # the values of the definition, fixed here: mix64 is splitmix64's finaliser over x + the golden-ratio constant
    assert ref.mix64(0) == 0xE220A8397B1DCDAF
    assert ref.mix64(1) == 0x910A2DEC89025CC1
    assert [ref.draw(0, h, 1000) for h in range(4)] == FIXED_DRAWS_SEED0_M1000
    assert [ref.draw(12345, h, 200) for h in (0, 1, 4095)] == FIXED_DRAWS_SEED12345_M200


FIXED_DRAWS_SEED0_M1000 = [(652, 367, 392), (626, 979, 709), (266, 896, 93), (966, 502, 941)]
FIXED_DRAWS_SEED12345_M200 = [(95, 15, 34), (92, 48, 147), (32, 75, 163)]


def rigid(axis, angle, t):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


def test_a_triangle_frame_pose_recovers_a_rigid_motion():
    T = rigid([0.1, 0.2, 0.97], np.deg2rad(150.0), [12.0, -7.0, 1.5])
    s = np.array([[0.0, 0, 0], [2, 0, 0], [0.5, 3, 1]])
    t = s @ T[:3, :3].T + T[:3, 3]
    R, tr, ok, shaky = ref.pose_from_triangles(s, t)
    assert ok and not shaky
    assert np.allclose(R, T[:3, :3], rtol=0, atol=1e-15) and np.allclose(tr, T[:3, 3], rtol=0, atol=1e-14)
    # collinear points have no frame
    assert not ref.pose_from_triangles(np.array([[0.0, 0, 0], [1, 0, 0], [3, 0, 0]]), t)[2]
    assert not ref.pose_from_triangles(np.array([[0.0, 0, 0], [0, 0, 0], [3, 1, 0]]), t)[2]


def test_ransac_on_planted_pairs_and_kabsch():
    rng = np.random.default_rng(5)
    T = rigid([0.3, -0.2, 0.9], 2.0, [1.0, 2.0, -0.5])
    ps = rng.uniform(-10, 10, (60, 3))
    pt = ps @ T[:3, :3].T + T[:3, 3]
    pt[20:] = rng.uniform(-10, 10, (40, 3))  # one third planted, the rest clutter
    r = ref.ransac(ps, pt, max_distance=0.05, iterations=2000, seed=1)
    assert r["best"] >= 0 and r["score"][r["best"]] == 20 and set(r["triple"][r["best"]]) <= set(range(20))
    assert r["valid"].sum() < 2000  # the edge test drops the mixed triples
    assert ref.pose_error(np.block([[r["R"][r["best"]], r["t"][r["best"]][:, None]], [np.zeros((1, 3)), np.ones((1, 1))]]), T)[0] < 1e-12
    noisy = pt[:20] + rng.normal(0, 0.01, (20, 3))
    K = ref.kabsch(ps[:20], noisy)
    dt, dr = ref.pose_error(K, T)
    assert dt < 0.02 and dr < 0.005
    assert np.linalg.det(K[:3, :3]) == pytest.approx(1.0, abs=1e-12)
    assert ref.pose_error(ref.kabsch(ps[:20], pt[:20]), T) < (1e-12, 1e-12)
    assert ref.ransac(ps[:2], pt[:2])["best"] == -1

"""tests/visibility_ref.py — the numpy float64 restatement of sga_cloud_visibility — on cases decided by hand:
one return and one map point in front of it, on it and behind it; the window's wrap across the azimuth seam; rows above and below the
field of view; ranges below min_range and above max_range; a scene checked against its own scan, which holds no seen-through point for
any margin >= 0; the band and the ambiguity helpers.  No device and no library call."""
import numpy as np
import pytest

import outliers_ref
import visibility_ref as ref

F32 = np.float32
DEG = np.pi / 180.0


def cloud(*rows):
    return np.array(rows, dtype=F32).reshape(-1, 3)


def states(map_pts, scan_pts, **kw):
    return ref.restate(map_pts, scan_pts, **kw)


def test_in_front_of_on_and_behind_one_return():
    scan = cloud([10.0, 0.0, 0.0])
    want = states(cloud([5.0, 0.0, 0.0], [10.0, 0.0, 0.0], [15.0, 0.0, 0.0], [10.25, 0.0, 0.0], [9.75, 0.0, 0.0]), scan)
    assert want["state"].tolist() == [ref.SEEN_THROUGH, ref.CONSISTENT, ref.OCCLUDED, ref.CONSISTENT, ref.CONSISTENT]  # tol = 0.2 + 1 %
    assert np.array_equal(want["clearance"], [5.0, 0.0, -5.0, -0.25, 0.25])
    assert want["counts"] == {"unobserved": 0, "consistent": 3, "occluded": 1, "seen_through": 1}
    img = want["image"]
    assert img.shape == (64, 1024) and np.isfinite(img).sum() == 1 and img[6, 512] == 10.0  # az 0 -> u = W / 2; el 0 -> v = floor(3 / 28 * 64)
    # another direction sees nothing: unobserved, NaN
    want = states(cloud([0.0, 5.0, 0.0]), scan)
    assert want["state"].tolist() == [ref.UNOBSERVED] and np.isnan(want["clearance"][0])


def test_the_least_range_of_a_cell_and_the_extremes_of_a_window():
    scan = cloud([10.0, 0.0, 0.0], [8.0, 0.0, 0.0], [12.0, 0.0, 0.0], [20.0, 0.2, 0.0])  # three in one cell, one a cell further left
    img, pr, _ = ref.range_image(scan)
    assert pr["u"].tolist() == [512, 512, 512, 513] and img[6, 512] == 8.0 and abs(img[6, 513] - np.sqrt(400.04)) < 1e-5
    want = states(cloud([7.0, 0.0, 0.0], [9.0, 0.0, 0.0], [19.0, 0.0, 0.0], [21.0, 0.0, 0.0]), scan)
    # m = 8, M = 20.001: 7 is in front of both, 9 and 19 between them, 21 behind both
    assert want["state"].tolist() == [ref.SEEN_THROUGH, ref.CONSISTENT, ref.CONSISTENT, ref.OCCLUDED]
    assert np.allclose(want["clearance"], [1.0, -1.0, -11.0, -13.0])
    # without the window the far return is not seen
    want = states(cloud([19.0, 0.0, 0.0]), scan, window_h=0, window_v=0)
    assert want["state"].tolist() == [ref.OCCLUDED]


def test_the_window_wraps_across_the_azimuth_seam():
    kw = dict(width=8, height=4, fov_up=30 * DEG, fov_down=-31 * DEG)
    scan = cloud([-10.0, -0.1, 0.0])  # az just above -pi: u = 0
    point = cloud([-5.0, 0.1, 0.0])   # az just below +pi: u = 7
    pr = ref.project(np.concatenate([scan, point]).astype(np.float64), 8, 4, 30 * DEG, -31 * DEG)
    assert pr["u"].tolist() == [0, 7] and pr["v"].tolist() == [1, 1]
    assert states(point, scan, window_h=1, window_v=0, **kw)["state"].tolist() == [ref.SEEN_THROUGH]
    assert states(point, scan, window_h=0, window_v=0, **kw)["state"].tolist() == [ref.UNOBSERVED]
    assert states(scan, point, window_h=1, window_v=0, **kw)["state"].tolist() == [ref.OCCLUDED]  # and from the other side
    # azimuth +pi is the direction of -pi: su = width becomes u = 0
    pr = ref.project(np.array([[-10.0, 0.0, 0.0], [-10.0, -0.0, 0.0]]), 8, 4, 30 * DEG, -31 * DEG)
    assert pr["su"].tolist() == [8.0, 0.0] and pr["u"].tolist() == [0, 0] and pr["inside"].all() and not pr["ambiguous"].any()
    # a window wider than the image visits cells twice: the multiset's extremes do not change
    assert states(point, scan, window_h=16, window_v=0, **kw)["state"].tolist() == [ref.SEEN_THROUGH]


def test_rows_above_and_below_the_field_of_view():
    kw = dict(width=16, height=4, fov_up=10 * DEG, fov_down=-10 * DEG, window_h=0, window_v=1)
    up, down = np.tan(12 * DEG) * 10.0, -np.tan(12 * DEG) * 10.0
    scan = cloud([10.0, 0.0, up], [10.0, 0.0, down], [10.0, 0.0, np.tan(9 * DEG) * 10.0])  # two outside the image, one in row 0
    img, pr, _ = ref.range_image(scan, **kw)
    assert pr["inside"].tolist() == [False, False, True] and np.isfinite(img).sum() == 1 and np.isfinite(img[0, 8])
    want = states(cloud([5.0, 0.0, up / 2], [5.0, 0.0, down / 2], [5.0, 0.0, np.tan(9 * DEG) * 5.0], [5.0, 0.0, np.tan(3 * DEG) * 5.0], [5.0, 0.0, -np.tan(9 * DEG) * 5.0]), scan, **kw)
    # out of the image above and below; row 0 (its window's row -1 is skipped); row 1 sees row 0; row 3 sees nothing (row 4 is skipped)
    assert want["state"].tolist() == [ref.UNOBSERVED, ref.UNOBSERVED, ref.SEEN_THROUGH, ref.SEEN_THROUGH, ref.UNOBSERVED]
    # the edges themselves: el = fov_up is row 0, el = fov_down is outside (sv = height)
    pr = ref.project(np.array([[np.cos(10 * DEG), 0.0, np.sin(10 * DEG)], [np.cos(10 * DEG), 0.0, -np.sin(10 * DEG)]]) * 7.0, 16, 4, 10 * DEG, -10 * DEG)
    assert pr["ambiguous"].all()  # sv within AMBIG of 0 and of height: either side may come out


def test_ranges_outside_min_and_max():
    def ray(*xs):  # off the x axis, where su would sit on a cell's edge; y = x / 32 is exact in fp32
        return cloud(*[[x, x / 32.0, 0.0] for x in xs])

    def rho(x):
        return float(np.sqrt(np.float64(F32(x)) ** 2 + np.float64(F32(x / 32.0)) ** 2))

    scan = ray(0.3, 20.0)  # the first is the ego vehicle: it would shadow everything
    kw = dict(min_range=rho(0.5), max_range=rho(60.0))
    img, pr, _ = ref.range_image(scan, **kw)
    assert pr["used"].tolist() == [False, True] and img[6, 517] == rho(20.0) and np.isfinite(img).sum() == 1
    want = states(ray(0.3, 0.5, 10.0, 60.0, 60.5), scan, **kw)
    assert want["state"].tolist() == [ref.UNOBSERVED, ref.SEEN_THROUGH, ref.SEEN_THROUGH, ref.OCCLUDED, ref.UNOBSERVED]
    assert want["band"].tolist() == [1, 3]  # rho exactly min_range / max_range
    # max_range does not bound the scan's returns, and may be infinite
    want = states(cloud([10.0, 0.0, 0.0], [90.0, 0.0, 0.0]), cloud([80.0, 0.0, 0.0]), max_range=float("inf"))
    assert want["state"].tolist() == [ref.SEEN_THROUGH, ref.OCCLUDED]
    # an empty scan: every point unobserved
    want = states(cloud([10.0, 0.0, 0.0]), np.zeros((0, 3), F32))
    assert want["state"].tolist() == [ref.UNOBSERVED] and not np.isfinite(want["image"]).any()


def test_non_finite_records_are_unobserved_and_in_no_output():
    scan = cloud([10.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0])
    want = states(cloud([5.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [5.0, -np.inf, 0.0], [0.0, 0.0, 0.0]), scan)
    assert want["state"].tolist() == [ref.SEEN_THROUGH, 0, 0, 0] and np.isfinite(want["image"]).sum() == 1
    assert ref.kept(want, "seen_through").tolist() == [0] and ref.kept(want, "rest").tolist() == [3]  # (the origin itself: rho = 0, unobserved, finite)


def test_the_pose_and_the_origins():
    T = np.eye(4)
    T[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]  # the sensor looks along the map's +y
    T[:3, 3] = [100.0, 200.0, 1.0]
    o_m, o_s = np.array([128.0, 128.0, 0.0]), np.array([0.0, 0.0, 0.0])
    scan = cloud([10.0, 0.0, 0.0])  # a return 10 m ahead: the map's (100, 210, 1)
    ahead = np.array([[100.0, 205.0, 1.0], [100.0, 215.0, 1.0]]) - o_m
    want = states(ahead.astype(F32), scan, o_m=o_m, T=T, o_s=o_s)
    assert np.array_equal(want["s"], [[5.0, 0.0, 0.0], [15.0, 0.0, 0.0]]) and want["state"].tolist() == [ref.SEEN_THROUGH, ref.OCCLUDED]
    # the scan's own origin moves its returns
    want = states(ahead.astype(F32), cloud([-118.0, 0.0, 0.0]), o_m=o_m, T=T, o_s=np.array([128.0, 0.0, 0.0]))
    assert want["state"].tolist() == [ref.SEEN_THROUGH, ref.OCCLUDED]


@pytest.mark.parametrize("margin, ratio", [(0.0, 0.0), (0.1, 0.01), (0.0, 0.05), (2.0, 0.0)])
def test_a_scene_against_its_own_scan_holds_no_seen_through_point(margin, ratio):
    scene = outliers_ref.planes_with_scatter(1, 1450, 100)
    for window in (0, 1, 2):
        want = states(scene, scene, width=128, height=32, fov_up=60 * DEG, fov_down=-60 * DEG, max_range=12.0, margin=margin, margin_ratio=ratio, window_h=window, window_v=window)
        # a point that is observed has its own return in its window: m <= rho
        assert want["counts"]["seen_through"] == 0 and want["counts"]["consistent"] + want["counts"]["occluded"] > 2500
        assert np.all(want["clearance"][want["state"] != 0] <= 0.0)


def test_the_band_and_the_ambiguity_helpers():
    scan = cloud([8.0, 0.25, 0.0])  # (off the x axis, where su would sit on a cell's edge)
    half = float(np.sqrt(16.015625))  # |(4, 0.125, 0)|, exactly half of |(8, 0.25, 0)|
    # rho + tol == m exactly, and just beside it
    want = states(cloud([4.0, 0.125, 0.0], [4.0 - 1e-3, 0.125, 0.0]), scan, margin=half, margin_ratio=0.0)
    assert want["state"].tolist() == [ref.CONSISTENT, ref.SEEN_THROUGH] and want["band"].tolist() == [0]
    assert np.all(want["B"] > 0) and np.all(want["B"] < 1e-12)
    # rho - tol == M exactly
    want = states(cloud([16.0, 0.5, 0.0], [16.0 + 1e-3, 0.5, 0.0]), scan, margin=2 * half, margin_ratio=0.0)
    assert want["state"].tolist() == [ref.CONSISTENT, ref.OCCLUDED] and want["band"].tolist() == [0]
    # a projection on a cell's edge: az = pi / 2 with a width of 8 is su = 6 exactly
    pr = ref.project(np.array([[0.0, 10.0, 0.0], [1.0, 10.0, 0.0]]), 8, 64, 3 * DEG, -25 * DEG)
    assert pr["ambiguous"].tolist() == [True, False] and pr["inside"].all()
    # an ambiguous scan return makes the cells it may land in unsure, and with them every map point whose window holds one
    amb_scan = cloud([0.0, 10.0, 0.0])
    img, spr, unsure = ref.range_image(amb_scan, width=8)
    assert spr["ambiguous"].tolist() == [True] and unsure.sum() == 2 and unsure[6, 5] and unsure[6, 6]
    want = states(cloud([-5.0, 4.0, 0.0], [5.0, 0.5, 0.0]), amb_scan, width=8, window_h=1)  # u = 7: its window holds cell 6; u = 4: cells 3 .. 5
    assert want["ambiguous_scan"] == 1 and want["band"].tolist() == [0, 1]
    want = states(cloud([5.0, 0.5, 0.0]), amb_scan, width=8, window_h=0)
    assert want["band"].tolist() == []
    # a point far out of the image is not ambiguous whatever its sv
    pr = ref.project(np.array([[1.0, 1.0, 30.0]]), 8, 64, 3 * DEG, -25 * DEG)
    assert not pr["inside"].any() and not pr["ambiguous"].any()

"""The numpy restatement of the plane segmentation (tests/plane_ref.py) on cases decided by hand.  No device,
no library: what the GPU tests hold the device against has to be right on its own."""
import numpy as np

import plane_ref
from global_ref import draw, draws

DROPPED = plane_ref.DROPPED


def wall_and_floor(seed=5):
    """a 3000-point wall x = 4 (4 m x 3 m) and a 1500-point floor z = 0, both with 5 mm of noise"""
    g = np.random.default_rng(seed)
    wall = np.stack([4.0 + 0.005 * g.standard_normal(3000), g.uniform(-2.0, 2.0, 3000), g.uniform(0.0, 3.0, 3000)], axis=1)
    floor = np.stack([g.uniform(0.0, 4.0, 1500), g.uniform(-2.0, 2.0, 1500), 0.005 * g.standard_normal(1500)], axis=1)
    return np.concatenate([wall, floor]).astype(np.float32)


def test_the_plane_z_0_with_outliers():
    g = np.random.default_rng(1)
    on = np.stack([g.uniform(-5, 5, 400), g.uniform(-5, 5, 400), np.zeros(400)], axis=1)
    off = np.stack([g.uniform(-5, 5, 100), g.uniform(-5, 5, 100), g.uniform(0.5, 5.0, 100)], axis=1)
    pts = np.concatenate([on, off]).astype(np.float32)
    r = plane_ref.segment_plane(pts, 0.05, 200, seed=3)
    assert r["found"] and r["refit"] == 1
    assert r["hypothesis_inliers"] == 400 and r["inliers"] == 400 and r["inlier_mask"][:400].all() and not r["inlier_mask"][400:].any()
    assert np.allclose(r["plane"], [0.0, 0.0, 1.0, 0.0], atol=1e-12) and r["rmse"] < 1e-12
    assert r["scores"][r["best_hypothesis"]] == 400 and (r["scores"][: r["best_hypothesis"]] != 400).all()  # the lowest h among the best
    assert r["scored"] == int((r["scores"] != DROPPED).sum()) and int(r["band"].sum()) == 0


def test_a_collinear_triple_is_dropped():
    line = np.stack([np.arange(10.0), 2.0 * np.arange(10.0), -np.arange(10.0)], axis=1).astype(np.float32)
    r = plane_ref.segment_plane(line, 0.1, 50, seed=0)
    assert r["scored"] == 0 and (r["scores"] == DROPPED).all() and not r["found"] and r["inliers"] == 0 and not r["plane"].any()
    same = np.ones((20, 3), np.float32)
    r = plane_ref.segment_plane(same, 0.1, 50, seed=0)
    assert r["scored"] == 0 and not r["found"]
    # a triple with a non-finite record is dropped as well
    pts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    for bad in (np.nan, np.inf):
        q = pts.copy()
        q[1, 0] = bad
        assert plane_ref.segment_plane(q, 0.1, 8)["scored"] == 0


def test_the_orientation_rule():
    n, ok, _ = plane_ref.orient(np.array([[0.0, 0.0, -1.0], [0.0, -1.0, 0.0], [-1.0, 0.0, 0.0], [0.6, 0.0, -0.8], [0.0, 0.6, 0.8]]))
    assert ok.all() and (n == np.array([[0, 0, 1.0], [0, 1.0, 0], [1.0, 0, 0], [-0.6, 0, 0.8], [0, 0.6, 0.8]])).all()
    # with an axis the normal is turned towards it, and kept within the angle only
    n, ok, _ = plane_ref.orient(np.array([[0.0, 0.0, 1.0], [0.0, 0.0, -1.0], [np.sin(0.2), 0.0, -np.cos(0.2)], [1.0, 0.0, 0.0]]), axis=(0, 0, -2.0), max_angle=0.1)
    assert (n[:2] == [0, 0, -1.0]).all() and list(ok) == [True, True, False, False]
    tilted = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.3, 0.3, 0.0]], np.float32)
    tilted[:, 2] = -0.1 * tilted[:, 0]  # z = -0.1 x: the upward normal is (0.1, 0, 1) / |.|
    r = plane_ref.segment_plane(tilted, 0.01, 20, seed=1)
    assert r["found"] and r["plane"][2] > 0 and np.allclose(r["plane"][:3], np.array([0.1, 0.0, 1.0]) / np.sqrt(1.01), atol=1e-7)


def test_a_tie_goes_to_the_lowest_hypothesis():
    # two parallel planes of 50 points each, far apart: every hypothesis within one plane scores 50
    g = np.random.default_rng(2)
    xy = g.uniform(-1, 1, (100, 2))
    pts = np.column_stack([xy, np.repeat([0.0, 5.0], 50)]).astype(np.float32)
    r = plane_ref.segment_plane(pts, 0.01, 64, seed=9, refit=False)
    top = int(r["scores"][r["scores"] != DROPPED].max())
    assert top == 50 and int((r["scores"] == 50).sum()) >= 2
    assert r["best_hypothesis"] == int(np.flatnonzero(r["scores"] == 50)[0]) and r["refit"] == 0
    tri = draws(9, [r["best_hypothesis"]], 100)[0]
    assert tuple(tri) == draw(9, r["best_hypothesis"], 100)
    assert r["anchor"].tolist() == pts[tri[0]].astype(np.float64).tolist()  # the triple's plane about its first record


def test_the_axis_constraint_picks_the_floor():
    pts = wall_and_floor()
    free = plane_ref.segment_plane(pts, 0.02, 300, seed=0)
    assert free["found"] and abs(free["plane"][0]) > 0.999 and free["inliers"] >= 2950 and abs(abs(free["plane"][3]) - 4.0) < 0.01
    held = plane_ref.segment_plane(pts, 0.02, 300, seed=0, axis=(0, 0, 1), max_angle=np.radians(10.0))
    assert held["found"] and held["plane"][2] > 0.999 and 1450 <= held["inliers"] <= 1600 and abs(held["plane"][3]) < 0.01
    assert held["scored"] < free["scored"] and held["scored"] == int((held["scores"] != DROPPED).sum())
    assert (held["scores"][free["scores"] == DROPPED] == DROPPED).all()


def test_the_loop_over_several_planes():
    g = np.random.default_rng(4)
    a = np.column_stack([g.uniform(0, 2, 400), g.uniform(0, 2, 400), np.zeros(400)])
    b = np.column_stack([np.zeros(250), g.uniform(0, 2, 250), g.uniform(0.1, 2, 250)])
    pts = np.concatenate([a, b]).astype(np.float32)
    r = plane_ref.segment_planes(pts, 4, 0.01, 200, seed=1, min_inliers=100)
    assert len(r["planes"]) == 2 and (r["labels"][:400] == 0).all() and (r["labels"][400:] == 1).all() and len(r["rest_indices"]) == 0

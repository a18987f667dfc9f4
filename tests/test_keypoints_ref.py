"""tests/keypoints_ref.py — the ISS keypoint rule of DESIGN.md section 3.28 in numpy — on cases whose answer is known by hand: each test
of rule 3 is the one that decides on a shape built for it, min_neighbors applies to either radius, and rule 4's tie goes to the lowest
index.  No device, no library."""
import numpy as np

import keypoints_ref as ref


def grid(xs, ys, zs=(0.0,)):
    x, y, z = np.meshgrid(np.asarray(xs, float), np.asarray(ys, float), np.asarray(zs, float), indexing="ij")
    return np.column_stack([x.ravel(), y.ravel(), z.ravel()])


def at(points, q):
    """the index of the point at q"""
    d = np.abs(np.asarray(points, np.float32).astype(np.float64) - np.asarray(q, np.float32).astype(np.float64)).max(axis=1)
    assert d.min() == 0.0
    return int(d.argmin())


STEP = np.arange(-8, 9) * 0.125  # a 1/8 m lattice: exact in fp32, every sum exact in double; every d2 is a multiple of 1/64, which none of the radii
# below is when squared: a neighbour exactly ON a radius would put the whole lattice in the band


def rule3(r, i, gamma=0.975):
    """which of the tests of rule 3 hold at point i, from the eigenvalues the restatement reports"""
    l1, l2, l3 = r["l1"][i], r["l2"][i], r["l3"][i]
    return l1 > 0.0, l2 < gamma * l1, l3 < gamma * l2, l3 > 1e-9 * l1


def test_a_flat_patch_is_stopped_by_the_floor_alone():
    p = grid(STEP, STEP[4:13])  # a strip 2 m x 1 m in z = 0: l1 > l2 > 0 and l3 = 0 up to rounding
    r = ref.iss(p, 1.05, 0.55)
    i = at(p, (0, 0, 0))
    assert rule3(r, i) == (True, True, True, False) and abs(r["l3"][i]) <= 1e-15 * r["l1"][i]
    assert not r["saliency"].any() and len(r["indices"]) == 0 and not r["band"].any()
    # tilted, the strip's l3 is rounding noise of either sign: still stopped, and not in the band (1e-9 l1 is far from 1e-12 l1)
    c, s = np.cos(0.3), np.sin(0.3)
    t = ref.iss(p @ np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]]), 1.05, 0.55)
    assert not t["saliency"].any() and not t["band"].any() and np.abs(t["l3"]).max() < 1e-7 * t["l1"].max()


def crease(theta):
    """two faces that meet along the x axis, each falling away at theta from the horizontal"""
    p = grid(STEP, STEP)
    return np.column_stack([p[:, 0], p[:, 1] * np.cos(theta), -np.abs(p[:, 1]) * np.sin(theta)])


def test_a_shallow_straight_edge_is_stopped_by_gamma_21_alone():
    """on the edge the neighbourhood is a disc folded by theta: l2 = cos^2(theta) l1, above 0.975 l1 below 9.1 degrees"""
    p = crease(np.deg2rad(5.0))
    r = ref.iss(p, 1.05, 0.55)
    i = at(p, (0, 0, 0))
    assert rule3(r, i) == (True, False, True, True) and r["saliency"][i] == 0.0
    assert abs(r["l2"][i] / r["l1"][i] - np.cos(np.deg2rad(5.0)) ** 2) < 1e-6  # (fp32 records)
    assert rule3(r, i, gamma=0.995) == (True, True, True, True)
    assert ref.iss(p, 1.05, 0.55, gamma_21=0.999)["saliency"][i] == r["l3"][i] > 0.0  # a wider gamma lets it through
    sharp = crease(np.deg2rad(45.0))
    s = ref.iss(sharp, 1.05, 0.55)
    assert rule3(s, at(sharp, (0, 0, 0))) == (True, True, True, True) and s["saliency"][at(sharp, (0, 0, 0))] > 0.0  # a sharp one passes


def test_blobs_are_stopped_by_gamma_32():
    rod = grid(STEP, STEP[6:11], STEP[6:11])  # 2 m long, 0.5 m x 0.5 m across: l1 > l2 = l3
    r = ref.iss(rod, 1.05, 0.55)
    i = at(rod, (0, 0, 0))
    assert rule3(r, i) == (True, True, False, True) and r["saliency"][i] == 0.0
    ball = grid(STEP[4:13], STEP[4:13], STEP[4:13])  # isotropic: l1 = l2 = l3, both gammas stop it
    b = ref.iss(ball, 0.55, 0.55)
    assert rule3(b, at(ball, (0, 0, 0))) == (True, False, False, True) and b["saliency"][at(ball, (0, 0, 0))] == 0.0


def corner():
    """three faces of a box of 1.0 x 0.75 x 0.5 m that meet at the origin (a cube's corner is symmetric: two equal eigenvalues)"""
    a, b, c = STEP[8:17], STEP[8:15], STEP[8:13]
    return np.unique(np.vstack([grid(a, b, [0.0]), grid(a, [0.0], c), grid([0.0], b, c)]), axis=0)


def test_a_corner_of_three_unequal_faces_passes():
    p = corner()
    r = ref.iss(p, 1.55, 0.8)
    i = at(p, (0, 0, 0))
    assert rule3(r, i) == (True, True, True, True) and r["saliency"][i] == r["l3"][i] > 0.0
    cube = np.unique(np.vstack([grid(STEP[8:17], STEP[8:17], [0.0]), grid(STEP[8:17], [0.0], STEP[8:17]), grid([0.0], STEP[8:17], STEP[8:17])]), axis=0)
    k = ref.iss(cube, 2.05, 0.8)
    j = at(cube, (0, 0, 0))
    assert k["saliency"][j] == 0.0 and not all(rule3(k, j))  # the symmetric corner: stopped by a gamma


def test_min_neighbors_applies_to_either_radius():
    p = corner()
    i = at(p, (0, 0, 0))
    full = ref.iss(p, 1.55, 0.8)
    c, w = int(full["count_salient"][i]), int(full["count_window"][i])
    assert c > w > 5
    assert ref.iss(p, 1.55, 0.8, min_neighbors=c)["saliency"][i] > 0.0
    assert ref.iss(p, 1.55, 0.8, min_neighbors=c + 1)["saliency"][i] == 0.0  # too few within the salient radius: no saliency
    # enough within the salient radius, too few in the window: salient, not a keypoint
    lone = np.vstack([p[np.linalg.norm(p, axis=1) > 0.8], [[0.0, 0.0, 0.0]]])
    i = len(lone) - 1
    r = ref.iss(lone, 1.55, 0.8)
    assert r["saliency"][i] > 0.0 and r["count_window"][i] == 1 and not r["keypoint"][i]
    assert ref.iss(lone, 1.55, 0.8, min_neighbors=1)["keypoint"][i]


def test_a_tie_goes_to_the_lowest_index():
    p = corner()
    best = ref.iss(p, 1.55, 0.8)
    i = int(np.argmax(best["saliency"]))
    assert best["keypoint"][i]  # (argmax: the first, so the lowest index, of the greatest saliency)
    n = len(p)
    twice = np.vstack([p, p])  # every point a second time: every sum doubles exactly, the covariances are the same bytes
    r = ref.iss(twice, 1.55, 0.8)
    assert np.array_equal(r["saliency"][:n], best["saliency"]) and np.array_equal(r["saliency"][n:], best["saliency"]) and r["ties"] >= 2
    assert np.array_equal(r["indices"], best["indices"]) and r["keypoint"][i] and not r["keypoint"][n:].any()  # only the lower copy
    flipped = ref.iss(twice[::-1], 1.55, 0.8)  # the same cloud back to front: the winners are the copies that now come first
    assert len(flipped["indices"]) >= 1 and (flipped["indices"] < n).all()
    # two points a hair apart share their neighbour set: the same covariance up to rounding, which is the band's business
    q = np.vstack([ref.bumpy_surface(400, 3, 4.0), [[2.0, 2.0, 0.0], [2.0 + 1e-4, 2.0, 0.0]]])
    n = ref.iss(q, 1.05, 0.55)
    a, b = len(q) - 2, len(q) - 1
    assert abs(n["saliency"][a] - n["saliency"][b]) <= 2e-12 * n["l1"][a] and n["band"][a] and n["band"][b]


def test_sizes_and_the_empty_cloud():
    for n in (0, 1, 4):
        r = ref.iss(ref.bumpy_surface(n, 1, 1.0), 1.05, 0.55)
        assert len(r["indices"]) == 0 and r["saliency"].shape == (n,) and not r["saliency"].any() and r["band"].shape == (n,)
    r = ref.iss(ref.bumpy_surface(2000, 2), 1.0, 0.5)
    assert r["band"].sum() == 0 and r["ties"] == 0 and 20 < len(r["indices"]) < 200 and np.all(np.diff(r["indices"]) > 0)
    assert np.array_equal(np.flatnonzero(r["keypoint"]), r["indices"]) and (r["saliency"][r["indices"]] > 0).all()

"""tests/overlap_ref.py, the fp64 restatement of sga_cloud_overlap, checked without a device: against scipy's cKDTree where scipy is
installed (and against a second, differently written brute force in any case), on hand-made cases, and — for the voxel maps — against
tests/map_search_ref.py, which states the same search rules with sorted keys instead of a dict."""
import numpy as np
import pytest

import map_search_ref
import outliers_ref
import overlap_ref as ref

F32 = np.float32


def pose(yaw, pitch, roll, t):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    T = np.eye(4)
    T[:3, :3] = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]]) @ np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T[:3, 3] = t
    return T


POSE = pose(0.3, -0.2, 0.1, (1.5, -2.0, 0.5))


def scene_pair(target_seed, source_seed, n_plane=340, n_scatter=50):
    target = outliers_ref.planes_with_scatter(target_seed, n_plane, n_scatter)
    scene = outliers_ref.planes_with_scatter(source_seed, n_plane, n_scatter).astype(np.float64)
    Ti = np.linalg.inv(POSE)
    return target, (scene @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32)


def slow_nearest(q, target):
    """the same answer one query at a time, with Python floats and math.sqrt"""
    import math

    out_i, out_d = [], []
    for x, y, z in q:
        best, win = math.inf, -1
        for j, (a, b, c) in enumerate(target.astype(np.float64)):
            d2 = (a - x) * (a - x) + (b - y) * (b - y) + (c - z) * (c - z)
            if d2 < best:
                best, win = d2, j
        out_i.append(win)
        out_d.append(math.sqrt(best))
    return np.array(out_i), np.array(out_d)


def test_brute_force_against_a_second_brute_force_and_scipy():
    target, source = scene_pair(5, 6)
    q, _ = ref.queries(source, T=POSE)
    idx, d, second = ref.brute_nearest(q, target, chunk=100)
    si, sd = slow_nearest(q[:200], target)
    assert np.array_equal(idx[:200], si) and np.array_equal(d[:200], sd)
    assert np.all(second >= d)
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return
    kd, ki = cKDTree(target.astype(np.float64)).query(q, k=2)
    assert np.array_equal(ki[:, 0], idx)
    assert np.allclose(kd[:, 0], d, rtol=1e-14, atol=0) and np.allclose(kd[:, 1], second, rtol=1e-14, atol=0)


def test_queries_follow_the_stated_order():
    rel = np.array([[1.0, 2.0, 3.0], [-4.0, 0.5, 0.25]], F32)
    o_c, o_t = np.array([500e3, 4000e3, 0.0]), np.array([500e3 + 128.0, 4000e3, 0.0])
    q, mag = ref.queries(rel, o_c, POSE, o_t)
    R, t = POSE[:3, :3], POSE[:3, 3]
    for i in range(2):
        for k in range(3):
            c = ((R[k, 0] * o_c[0] + R[k, 1] * o_c[1]) + R[k, 2] * o_c[2]) + t[k]
            assert q[i, k] == (R[k, 0] * float(rel[i, 0]) + R[k, 1] * float(rel[i, 1])) + R[k, 2] * float(rel[i, 2]) + (c - o_t[k])
    exact = (rel.astype(np.float64) + o_c) @ R.T + t - o_t
    assert np.all(np.abs(q - exact) <= 8 * ref.EPS64 * mag[:, None])
    q0, _ = ref.queries(rel)  # no pose, one frame: the records themselves
    assert np.array_equal(q0, rel.astype(np.float64))


def test_a_point_at_exactly_max_distance_is_matched():
    target = np.array([[0.25, 0.0, 0.0]], F32)
    rel = np.array([[0.0, 0.0, 0.0], [-0.25, 0.0, 0.0], [0.5, 0.0, 0.0]], F32)
    res = ref.restate_kd(rel, target, 0.25)
    assert res["matched"].tolist() == [True, False, True] and res["d"].tolist() == [0.25, np.inf, 0.25]
    assert res["nearest"].tolist() == [0, -1, 0] and res["n_matched"] == 2 and res["fitness"] == 2 / 3
    assert res["rmse"] == 0.25 and res["mean_distance"] == 0.25
    assert ref.kept(res, "matched").tolist() == [0, 2] and ref.kept(res, "unmatched").tolist() == [1]
    assert ref.band(res, 0.25, np.zeros(3)).tolist() == [0, 2] and ref.band(res, 0.25, np.full(3, 0.3)).tolist() == [0, 1, 2]


def test_non_finite_points_are_unmatched_and_in_no_output():
    target = np.zeros((1, 3), F32)
    rel = np.array([[0.1, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, np.inf, 0.0], [3.0, 0.0, 0.0]], F32)
    for max_distance in (1.0, np.inf):
        res = ref.restate_kd(rel, target, max_distance)
        assert res["matched"].tolist() == [True, False, False, max_distance > 3.0]
        assert res["points"] == 4 and res["nearest"][1] == res["nearest"][2] == -1 and np.isinf(res["d"][1:3]).all()
        assert ref.kept(res, "unmatched").tolist() == ([] if max_distance > 3.0 else [3])  # counted, but in no cloud
        assert ref.kept(res, "matched").tolist() == ([0, 3] if max_distance > 3.0 else [0])


def test_empty_target_empty_cloud_and_one_target_point():
    rel = outliers_ref.planes_with_scatter(3, 20, 5)
    res = ref.restate_kd(rel, np.zeros((0, 3), F32), 1.0)
    assert res["n_matched"] == 0 and res["fitness"] == 0.0 and res["rmse"] == 0.0 and res["mean_distance"] == 0.0
    assert np.isinf(res["d"]).all() and (res["nearest"] == -1).all() and len(ref.kept(res, "unmatched")) == len(rel)
    res = ref.restate_kd(np.zeros((0, 3), F32), rel, 1.0)
    assert res["points"] == 0 and res["fitness"] == 0.0 and len(ref.kept(res, "matched")) == 0
    one = ref.restate_kd(rel, rel[7:8], np.inf)
    assert (one["nearest"] == 0).all() and one["d"][7] == 0.0 and np.isinf(one["second"]).all() and one["fitness"] == 1.0
    assert len(ref.near_ties(one, np.full(len(rel), 1.0))) == 0


def test_the_first_of_equal_distances_wins():
    target = np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]], F32)
    res = ref.restate_kd(np.zeros((1, 3), F32), target, 2.0)
    assert res["nearest"].tolist() == [0] and res["second"].tolist() == [1.0]
    assert ref.near_ties(res, np.zeros(1)).tolist() == [0]


@pytest.mark.parametrize("offsets", [1, 7, 27])
@pytest.mark.parametrize("flat", [False, True])
def test_map_restatement_against_the_sorted_key_restatement(offsets, flat):
    rng = np.random.default_rng(11)
    leaf = 0.5
    coords = np.unique(rng.integers(-4, 4, (150, 3)), axis=0)
    V = len(coords)
    if flat:
        counts = rng.integers(1, 5, V)
        points = ((coords[:, None, :] + rng.uniform(0.0, 1.0, (V, ref.CAP, 3))) * leaf).astype(F32)
        kw = {"points": points, "counts": counts}
    else:
        kw = {"means": ((coords + rng.uniform(0.0, 1.0, (V, 3))) * leaf).astype(F32)}
    rel = rng.uniform(-2.5, 2.5, (400, 3)).astype(F32)
    rel[5] = np.nan
    res = ref.restate_map(rel, coords, leaf, offsets, 0.3, T=POSE, **kw)
    fin = np.isfinite(res["q"]).all(1)
    idx, d2, s2 = map_search_ref.nearest(coords, leaf, np.zeros(3), offsets, res["q"][fin], **kw)
    if flat:
        idx = np.where(idx >= 0, (idx >> 32) * ref.CAP + (idx & 0xFFFFFFFF), -1)
    assert np.array_equal(np.where(np.sqrt(d2) <= 0.3, idx, -1), res["nearest"][fin])
    assert np.array_equal(np.sqrt(d2), res["raw_d"][fin]) and np.array_equal(np.sqrt(s2), res["second"][fin])
    assert not res["matched"][5] and 0 < res["n_matched"] < fin.sum()
    if offsets == 1:  # every point in an occupied voxel has a winner; with max_distance = inf the unmatched are the points in empty voxels
        all_in = ref.restate_map(rel, coords, leaf, 1, np.inf, T=POSE, **kw)
        occupied = {tuple(c) for c in coords.tolist()}
        cell = ref.fast_floor(res["q"][fin] / leaf)
        assert np.array_equal(all_in["matched"][fin], np.array([tuple(c) in occupied for c in cell.tolist()]))

"""A posed cloud compared with a target on the device (csrc/cloud_overlap.hip: sga_cloud_overlap) against the fp64
restatement of tests/overlap_ref.py, which never goes through the library.

Inputs: outliers_ref.planes_with_scatter for the target and for the scene; the cloud is the scene seen from the pose (yaw 0.3, pitch -0.2,
roll 0.1, t = (1.5, -2.0, 0.5)): fp32(T^-1 scene); both are uploaded relative to a named origin (test_cloud_merge_gpu.upload_relative), so
their records are known exactly.

The comparison rule for kd-tree targets is derived, not tuned.  With e_i = |q_i - float(q_i)|: the walk minimises an fp32 squared
distance measured from float(q_i), which differs from the true one by at most e_i plus 3 ulp of fp32 on d, so
    d_ref - 64 eps64 mag_i  <=  d_dev  <=  d_ref + 2 e_i + 1e-6 d_ref + 64 eps64 mag_i        (overlap_ref.kd_floor / kd_bound),
mag_i the magnitudes that enter q_i.  A point with |d_ref - max_distance| within that bound may fall either way, and a point whose two
nearest target records differ by no more than it may report either: at most 2 of each per case, asserted ON THE REFERENCE before
anything is compared (if a cap ever fails: another seed, never a looser rule).  Reference figures of the seven main cases, from the
restatement on the CPU (no band points, no near-ties in any of them):
    target 1 source 2  n 3000  max_distance 0.05   238 matched          target 3 source 4  n 3000  0.25  2721 matched
    target 1 source 2  n 3000  0.10                991                  target 5 source 6  n  730  0.25   328
    target 1 source 2  n 3000  0.25               2703                  target 1 source 1  n 3000  0.05  3000 (fitness 1, d about 1e-6:
    target 1 source 2  n 3000  1.0                2911                                                    only the absolute part holds)
Everything outside the two bands is exact: matched and kept equal the restatement's, kept is ascending, output records and attributes
equal input [kept] bit for bit, fitness == matched / points, rmse and mean_distance lie within the bound propagated from d, and two calls
return identical bytes.  Voxel-map targets: the contents are downloaded and restated; d agrees to 64 eps64 mag, membership and the
winner are exact — the reference is asserted to hold no query within that distance of a voxel face and no near-tie."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import outliers_ref
import overlap_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import api
from conftest import ROOT
from test_cloud_merge_gpu import FAR, attributes, pose, records, upload_relative
from test_cloud_outliers_gpu import attributes_for, synthetic_thinned

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS64 = ref.EPS64
ZERO = np.zeros(3)
INF = float("inf")
MAX_BAND, MAX_TIES = 2, 2
POSE = pose(0.3, -0.2, 0.1, t=(1.5, -2.0, 0.5))
KEEPS = [None, "matched", "unmatched"]
MAIN = [  # (target seed, source seed, points per plane, scatter, max_distance, matched in the reference)
    (1, 2, 1450, 100, 0.05, 238),
    (1, 2, 1450, 100, 0.10, 991),
    (1, 2, 1450, 100, 0.25, 2703),
    (1, 2, 1450, 100, 1.0, 2911),
    (3, 4, 1450, 100, 0.25, 2721),
    (5, 6, 340, 50, 0.25, 328),
    (1, 1, 1450, 100, 0.05, 3000),
]


# ---- inputs and references, computed once -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(seed, n_plane=1450, n_scatter=100):
    p = outliers_ref.planes_with_scatter(seed, n_plane, n_scatter)
    p.setflags(write=False)
    return p


def seen_from(points, T=POSE):
    """fp32(T^-1 points): the scene in the frame of a sensor at T"""
    Ti = np.linalg.inv(T)
    return np.ascontiguousarray((points.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32))


@functools.lru_cache(maxsize=None)
def source(seed, n_plane=1450, n_scatter=100):
    p = seen_from(scene(seed, n_plane, n_scatter))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def big_source():
    """9001 points: three scenes and one more point, so that the reduction's unrolled stride loop (8 x 1024) and several compaction tiles are entered"""
    p = np.ascontiguousarray(np.concatenate([source(2), source(4), source(6), source(8)[:1]]))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def kd_reference(tseed, sseed, n_plane, n_scatter, max_distance, n=None, tn=None):
    return ref.restate_kd(source(sseed, n_plane, n_scatter)[:n], scene(tseed, n_plane, n_scatter)[:tn], max_distance, T=POSE)


# ---- the call and the comparison ------------------------------------------------------------------------------------------------------------
def run(cloud, target, T, max_distance, keep, ctx=None):
    res = cloud.overlap(target, T, max_distance, keep, return_dist=True, return_nearest=True, return_kept=keep is not None, ctx=ctx)
    got = {"stats": res[0], "out": res[1] if keep else None, "dist": res[-3] if keep else res[-2], "nearest": res[-2] if keep else res[-1], "kept": res[-1] if keep else None}
    assert got["dist"].dtype == np.float64 and got["nearest"].dtype == np.int64
    return got


def same_bytes(a, b):
    """two calls: every output identical"""
    assert a["dist"].tobytes() == b["dist"].tobytes() and a["nearest"].tobytes() == b["nearest"].tobytes()
    assert a["stats"]["points"] == b["stats"]["points"] and a["stats"]["matched"] == b["stats"]["matched"]
    assert np.array([a["stats"][w] for w in ("fitness", "rmse", "mean_distance")]).tobytes() == np.array([b["stats"][w] for w in ("fitness", "rmse", "mean_distance")]).tobytes()
    if a["kept"] is not None:
        assert np.array_equal(a["kept"], b["kept"]) and a["out"].size() == b["out"].size()
        if a["out"].size():
            assert records(a["out"])[0].tobytes() == records(b["out"])[0].tobytes()


def check(got, want, rel, max_distance, keep, upper, lower, exact_winner=False, nrm=None, cov6=None, origin=ZERO, what=""):
    """the call's results `got` against the restatement `want` of the cloud's records `rel`; upper / lower: how far the device's distance may
    lie above / below the restatement's"""
    n = len(rel)
    edge = ref.band(want, max_distance, upper)
    ties = ref.near_ties(want, upper)
    assert len(edge) <= (0 if exact_winner else MAX_BAND), (what, "the reference has %d points in the band" % len(edge))
    assert len(ties) <= (0 if exact_winner else MAX_TIES), (what, "the reference has %d near-ties" % len(ties))
    dist, nearest, st = got["dist"], got["nearest"], got["stats"]
    dev = np.isfinite(dist)
    both = dev & want["matched"]
    over = dist[both] - want["raw_d"][both]
    print("%s n %d keep %s: matched %d (reference %d), band %d, near-ties %d, d_dev - d_ref in [%.3e, %.3e], worst share of the bound %.3f, fitness %.6f rmse %.9g (%.9g) mean %.9g (%.9g)"
          % (what, n, keep, int(dev.sum()), want["n_matched"], len(edge), len(ties), over.min() if len(over) else 0.0, over.max() if len(over) else 0.0,
             float(np.max(over / np.maximum(upper[both], 1e-300))) if len(over) else 0.0, st["fitness"], st["rmse"], want["rmse"], st["mean_distance"], want["mean_distance"]))
    # matched: the restatement's set but for the band points; an unmatched point says so in both arrays
    sure = np.ones(n, bool)
    sure[edge] = False
    assert np.array_equal(dev[sure], want["matched"][sure]), what
    assert np.array_equal(nearest < 0, ~dev) and np.all(np.isposinf(dist[~dev])) and np.all(nearest[~dev] == -1), what
    assert np.all(dist[dev] <= max_distance), what
    # distances within the derived bound, winners exact but for the near-ties
    assert np.all(over <= upper[both]) and np.all(over >= -lower[both]), (what, over.min(), over.max())
    clear = both.copy()
    clear[ties] = False
    assert np.array_equal(nearest[clear], want["nearest"][clear]), what
    # statistics: counts exact; the sums are those of the device's own distances (any order of n non-negative terms: n eps64 relative), and
    # lie within the bound propagated from d
    m = int(dev.sum())
    assert st["points"] == n and st["matched"] == m and st["fitness"] == ((m / n) if n else 0.0), what
    slack = 2 * max(n, 1) * EPS64
    if m:
        d = dist[dev]
        assert abs(st["mean_distance"] - d.sum() / m) <= slack * (d.sum() / m) and abs(st["rmse"] - np.sqrt((d * d).sum() / m)) <= slack * np.sqrt((d * d).sum() / m), what
        lo, hi = np.maximum(want["raw_d"][dev] - lower[dev], 0.0), want["raw_d"][dev] + upper[dev]
        assert lo.sum() / m * (1 - slack) <= st["mean_distance"] <= hi.sum() / m * (1 + slack), what
        assert np.sqrt((lo * lo).sum() / m) * (1 - slack) <= st["rmse"] <= np.sqrt((hi * hi).sum() / m) * (1 + slack), what
    else:
        assert st["rmse"] == 0.0 and st["mean_distance"] == 0.0, what
    if keep is None:
        assert got["out"] is None and got["kept"] is None
        return
    # the output cloud: the device's own flags decide it, and they are the restatement's but for the band points
    out, kept = got["out"], got["kept"]
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0), what  # ascending
    assert np.array_equal(kept, np.nonzero((dev if keep == "matched" else ~dev) & want["finite"])[0]), what
    assert np.all(np.isin(np.setxor1d(kept, ref.kept(want, keep)), edge)), what
    assert out.size() == len(kept), what
    assert np.array_equal(out.origin(), np.asarray(origin, dtype=np.float64))  # the origin is kept
    if len(kept) == 0:
        assert out._has() == (False, False) and out._box() is None  # an empty cloud without attributes
        return
    assert out._has() == (nrm is not None, cov6 is not None)
    rec, _ = records(out)
    assert rec.tobytes() == np.ascontiguousarray(rel[kept]).tobytes(), what  # bit for bit
    nr, c6 = attributes(out)
    if nrm is not None:
        assert nr.tobytes() == np.ascontiguousarray(nrm[kept]).tobytes(), what
    if cov6 is not None:
        assert c6.tobytes() == np.ascontiguousarray(cov6[kept]).tobytes(), what
    lo, hi = out._box()  # the box of its own records, as the crop reports it
    assert np.array_equal(lo, rel[kept].min(axis=0)) and np.array_equal(hi, rel[kept].max(axis=0)), what


def check_kd(got, want, rel, max_distance, keep, **kw):
    check(got, want, rel, max_distance, keep, ref.kd_bound(want), ref.kd_floor(want), **kw)


# ---- 1. the main cases against a kd-tree ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAIN, ids=lambda c: "t%d-s%d-n%d-r%g" % (c[0], c[1], 2 * c[2] + c[3], c[4]))
def test_kd_results_match_the_restatement(case):
    tseed, sseed, n_plane, n_scatter, max_distance, matched = case
    rel = source(sseed, n_plane, n_scatter)
    want = kd_reference(tseed, sseed, n_plane, n_scatter, max_distance)
    assert want["n_matched"] == matched  # the figure in this file's docstring
    nrm, cov6 = attributes_for(len(rel)) if case is MAIN[0] else (None, None)
    cloud = upload_relative(rel, nrm, cov6, ZERO)
    tree = sga.KdTree(upload_relative(scene(tseed, n_plane, n_scatter), None, None, ZERO))
    for keep in KEEPS:
        got = run(cloud, tree, POSE, max_distance, keep)
        check_kd(got, want, rel, max_distance, keep, nrm=nrm, cov6=cov6, what=str(case))
        same_bytes(got, run(cloud, tree, POSE, max_distance, keep))
    if sseed == tseed:
        assert got["stats"]["fitness"] == 1.0 and got["dist"].max() < 1e-5
    # the optional outputs are optional, and the module function takes an array
    st = cloud.overlap(tree, POSE, max_distance)
    assert isinstance(st, dict) and st == got["stats"]
    assert sga.cloud_overlap(rel, tree, POSE, max_distance) == st
    st2, out = cloud.overlap(tree, POSE, max_distance, keep="unmatched")
    assert st2 == st and out.size() == len(got["kept"])


# ---- 2. sizes at which the kernels can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_clouds(n):
    rel = source(6, 340, 50)[:n]
    want = kd_reference(5, 6, 340, 50, 0.25, n)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(upload_relative(scene(5, 340, 50), None, None, ZERO))
    for keep in KEEPS:
        check_kd(run(cloud, tree, POSE, 0.25, keep), want, rel, 0.25, keep, what="cloud of %d" % n)


@pytest.mark.parametrize("tn", [1, 5, 0])  # below a leaf; an empty target
def test_small_and_empty_targets(tn):
    rel = source(6, 340, 50)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(upload_relative(scene(5, 340, 50)[:tn], None, None, ZERO))
    for max_distance in (3.0, INF):
        want = kd_reference(5, 6, 340, 50, max_distance, None, tn)
        for keep in KEEPS:
            got = run(cloud, tree, POSE, max_distance, keep)
            check_kd(got, want, rel, max_distance, keep, what="target of %d" % tn)
        if tn == 0:
            assert got["stats"]["matched"] == 0 and got["out"].size() == len(rel)  # every point unmatched
        elif max_distance == INF:
            assert got["stats"]["fitness"] == 1.0 and got["out"].size() == 0  # every point has a neighbour


def test_an_empty_cloud_launches_nothing():
    tree = sga.KdTree(upload_relative(scene(5, 340, 50), None, None, ZERO))
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    before = sga.cloud_overlap_launches()
    for keep in KEEPS:
        got = run(empty, tree, POSE, 0.25, keep)
        assert got["stats"] == {"points": 0, "matched": 0, "fitness": 0.0, "rmse": 0.0, "mean_distance": 0.0}
        assert len(got["dist"]) == 0 and len(got["nearest"]) == 0
        if keep:
            assert got["out"].size() == 0 and got["out"]._has() == (False, False) and len(got["kept"]) == 0
    assert sga.cloud_overlap_launches() == before


def test_a_cloud_of_9001_points():
    rel = big_source()
    assert len(rel) == 9001
    want = ref.restate_kd(rel, scene(1), 0.25, T=POSE)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(upload_relative(scene(1), None, None, ZERO))
    for keep in KEEPS:
        got = run(cloud, tree, POSE, 0.25, keep)
        check_kd(got, want, rel, 0.25, keep, what="9001 points")
    same_bytes(got, run(cloud, tree, POSE, 0.25, "unmatched"))
    assert 0 < got["stats"]["matched"] < 9001


def test_an_infinite_max_distance_matches_every_point_with_a_neighbour():
    rel = source(2)
    want = kd_reference(1, 2, 1450, 100, INF)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(upload_relative(scene(1), None, None, ZERO))
    for keep in KEEPS:
        got = run(cloud, tree, POSE, INF, keep)
        check_kd(got, want, rel, INF, keep, what="max_distance inf")
    assert got["stats"]["fitness"] == 1.0 and got["out"].size() == 0  # keep = unmatched: only what has no neighbour


def test_non_finite_points_are_counted_unmatched_and_in_no_output():
    rel = source(6, 340, 50).copy()
    rel[17, 1] = np.nan
    rel[401] = [np.inf, 0.0, 0.0]
    rel[64, 2] = -np.inf
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(upload_relative(scene(5, 340, 50), None, None, ZERO))
    for max_distance in (0.25, INF):
        want = ref.restate_kd(rel, scene(5, 340, 50), max_distance, T=POSE)
        assert not want["matched"][[17, 401, 64]].any()
        for keep in KEEPS:
            got = run(cloud, tree, POSE, max_distance, keep)
            check_kd(got, want, rel, max_distance, keep, what="non-finite points, max_distance %g" % max_distance)
            assert got["stats"]["points"] == len(rel) and np.all(got["nearest"][[17, 401, 64]] == -1)
            if keep:
                assert not np.isin([17, 401, 64], got["kept"]).any()
        assert got["out"].size() == (0 if max_distance == INF else len(rel) - 3 - want["n_matched"])


# ---- 3. frames ------------------------------------------------------------------------------------------------------------------------------
def test_far_device_frames_with_the_pose_carrying_the_difference():
    o_c, o_t = FAR, FAR + np.array([30.0, 0.0, 0.0])
    rel, tgt = source(2), scene(1)
    # caller's frame: the cloud's points are rel + o_c, the target's tgt + o_t; T takes the one into the other
    T = POSE.copy()
    T[:3, 3] = POSE[:3, 3] + o_t - POSE[:3, :3] @ o_c
    want = ref.restate_kd(rel, tgt, 0.25, o_c, T, o_t)
    plain = kd_reference(1, 2, 1450, 100, 0.25)
    assert np.abs(want["q"] - plain["q"]).max() < 1e-7 and abs(want["n_matched"] - plain["n_matched"]) <= 2  # the same geometry, 4 000 km away
    cloud = upload_relative(rel, None, None, o_c)
    tree = sga.KdTree(upload_relative(tgt, None, None, o_t))
    for keep in KEEPS:
        check_kd(run(cloud, tree, T, 0.25, keep), want, rel, 0.25, keep, origin=o_c, what="far frames")


def test_no_pose_with_both_in_one_frame():
    rel, tgt = scene(2), scene(1)  # the scene itself: its planes are the target's
    want = ref.restate_kd(rel, tgt, 0.1, FAR, None, FAR)
    assert np.array_equal(want["q"], rel.astype(np.float64)) and 0 < want["n_matched"] < len(rel)
    cloud = upload_relative(rel, None, None, FAR)
    tree = sga.KdTree(upload_relative(tgt, None, None, FAR))
    for keep in KEEPS:
        check_kd(run(cloud, tree, None, 0.1, keep), want, rel, 0.1, keep, origin=FAR, what="T = None")


# ---- 4. voxel-map targets -------------------------------------------------------------------------------------------------------------------
LEAF = 0.5


def index_origin(index):
    o = np.empty(3)
    api.check(sga.load().sga_index_origin(index.h, api._dp(o)))
    return o


@functools.lru_cache(maxsize=None)
def map_target(kind):
    """-> (the map, the keyword arguments of overlap_ref.restate_map that state its downloaded contents)"""
    tgt = scene(1)
    if kind == "flat":
        m = sga.IncrementalVoxelMap(LEAF)
        m.insert(upload_relative(tgt, None, None, ZERO))
        coords, counts, pts = m.download()
        points = np.zeros((len(coords), ref.CAP, 3), F32)
        points[np.arange(ref.CAP)[None, :] < counts[:, None]] = pts
        contents = {"coords": coords, "points": points, "counts": counts}
    else:
        cloud = upload_relative(tgt, None, attributes_for(len(tgt))[1], ZERO)
        if kind == "one-shot":
            m = sga.GaussianVoxelMap.from_cloud(cloud, LEAF)
        else:
            m = sga.GaussianVoxelMap(LEAF)
            m.insert(cloud)
        coords, means, _, _ = m.download()
        contents = {"coords": coords, "means": means}
    assert not index_origin(m).any() and m.size() > 100  # origin zero: the download is the records as they are
    return m, contents


@pytest.mark.parametrize("kind, offsets", [("one-shot", 1), ("one-shot", 7), ("one-shot", 27), ("incremental", 1), ("incremental", 7), ("incremental", 27), ("flat", 1), ("flat", 7)])
def test_voxel_map_targets(kind, offsets):
    m, contents = map_target(kind)
    m.set_search_offsets(offsets)
    rel = source(2)
    max_distance = 0.25
    want = ref.restate_map(rel, contents["coords"], LEAF, offsets, max_distance, T=POSE, means=contents.get("means"), points=contents.get("points"), counts=contents.get("counts"))
    tol = 64 * EPS64 * want["mag"]
    x = want["q"] / LEAF
    assert not (np.abs(x - np.rint(x)) <= (tol / LEAF)[:, None]).any()  # no query within the bound of a voxel face: membership is exact
    assert 0 < want["n_matched"] < len(rel)
    cloud = upload_relative(rel, None, None, ZERO)
    try:
        for keep in KEEPS:
            got = run(cloud, m, POSE, max_distance, keep)
            check(got, want, rel, max_distance, keep, tol, tol, exact_winner=True, what="%s map, %d offsets" % (kind, offsets))
        same_bytes(got, run(cloud, m, POSE, max_distance, "unmatched"))
        if offsets == 1:  # with an infinite max_distance the unmatched are exactly the points in unoccupied voxels
            occupied = {tuple(c) for c in np.asarray(contents["coords"]).tolist()}
            in_empty = np.array([tuple(c) not in occupied for c in ref.fast_floor(x).tolist()])
            got = run(cloud, m, POSE, INF, "unmatched")
            assert np.array_equal(got["kept"], np.nonzero(in_empty)[0]) and got["stats"]["matched"] == int((~in_empty).sum())
    finally:
        m.set_search_offsets(1)


def test_a_map_without_voxels_leaves_every_point_unmatched():
    rel = source(6, 340, 50)
    cloud = upload_relative(rel, None, None, ZERO)
    for m in (sga.GaussianVoxelMap(LEAF), sga.IncrementalVoxelMap(LEAF)):
        st, out, nearest = cloud.overlap(m, POSE, 0.5, keep="unmatched", return_nearest=True)
        assert st["matched"] == 0 and st["fitness"] == 0.0 and out.size() == len(rel) and np.all(nearest == -1)


# ---- 5. refusals that need live handles -----------------------------------------------------------------------------------------------------
def test_a_projective_target_is_refused():
    rel = source(6, 340, 50)
    cloud = upload_relative(rel, None, None, ZERO)
    before = sga.cloud_overlap_launches()
    with pytest.raises(sga.SgaError, match="projective"):
        cloud.overlap(sga.ProjectiveSearch(scene(5, 340, 50), 64, 32), POSE, 0.25)
    assert sga.cloud_overlap_launches() == before


def test_an_index_on_another_device_is_refused():
    if sga.load().sga_device_count() < 2:
        pytest.skip("ONE DEVICE ONLY: the refusal of an index that lives on another device was NOT exercised")
    other = sga.Context(1)
    tree = sga.KdTree(upload_relative(scene(5, 340, 50), None, None, ZERO, other))
    cloud = upload_relative(source(6, 340, 50), None, None, ZERO)
    with pytest.raises(sga.SgaError, match="index lives on another device"):
        cloud.overlap(tree, POSE, 0.25)
    with pytest.raises(sga.SgaError, match="cloud lives on another device"):
        cloud.overlap(tree, POSE, 0.25, ctx=other)


# ---- 6. the launch counter ------------------------------------------------------------------------------------------------------------------
def test_the_launch_counter_rises_by_the_documented_amounts():
    tree = sga.KdTree(upload_relative(scene(1), None, None, ZERO))
    m, _ = map_target("one-shot")
    outliers, crops = sga.cloud_outliers_launches(), sga.cloud_crop_launches()
    for rel in (source(2), big_source()):  # whatever the size
        cloud = upload_relative(rel, None, None, ZERO)
        for target in (tree, m):
            before = sga.cloud_overlap_launches()
            cloud.overlap(target, POSE, 0.25)
            assert sga.cloud_overlap_launches() - before == 2  # the distances, the sums
            before = sga.cloud_overlap_launches()
            cloud.overlap(target, POSE, 0.25, keep="matched", return_kept=True)
            assert sga.cloud_overlap_launches() - before == 4  # ... the compaction's table copy, the compaction
    assert sga.cloud_outliers_launches() == outliers and sga.cloud_crop_launches() == crops
    sga.remove_outliers(source(2))  # and the outlier filter still counts its own compaction
    assert sga.cloud_outliers_launches() - outliers == 4 and sga.cloud_overlap_launches() == before + 4


# ---- 7. ordering across contexts ------------------------------------------------------------------------------------------------------------
def test_a_target_built_on_another_context_that_returned_early():
    rel, tgt = source(2), scene(1)
    plain = run(upload_relative(rel, None, None, ZERO), sga.KdTree(upload_relative(tgt, None, None, ZERO)), POSE, 0.25, "unmatched")
    ctx, other = sga.Context(0), sga.Context(0)
    ctx.set_stream_ordered(True)
    other.set_stream_ordered(True)
    try:
        cloud = upload_relative(rel, None, None, ZERO, ctx)
        tree = sga.KdTree(upload_relative(tgt, None, None, ZERO, other))  # returns with its kernels in flight on the other context's stream
        got = run(cloud, tree, POSE, 0.25, "unmatched")
        same_bytes(got, plain)
        check_kd(got, kd_reference(1, 2, 1450, 100, 0.25), rel, 0.25, "unmatched", what="a tree of another context")
    finally:
        ctx.set_stream_ordered(False)
        other.set_stream_ordered(False)


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------------------
def test_submap_odometry_keyframe_selection():
    from small_gicp_amd import odometry, synthetic

    frames = 6
    plain = odometry.run_synthetic_submap(frames, window=3)
    assert plain["keyframes_added"] == frames and plain["fitness"] == []
    every = odometry.run_synthetic_submap(frames, window=3, keyframe_overlap=1.0)
    if max(every["fitness"]) >= 1.0:  # a scan the submap explains completely: no finite threshold lets it join
        every = odometry.run_synthetic_submap(frames, window=3, keyframe_overlap=INF)
    assert len(every["fitness"]) == frames - 1 and every["keyframes_added"] == frames
    assert all(a.tobytes() == b.tobytes() for a, b in zip(plain["estimated"], every["estimated"]))
    first = odometry.run_synthetic_submap(frames, window=3, keyframe_overlap=0.0)
    assert first["keyframes_added"] == 1 and len(first["fitness"]) == frames - 1
    # by hand: every scan against the first scan alone, from the previous pose
    ctx = sga.Context(0)
    ctx.set_stream_ordered(True)
    setting = api.make_setting("GICP", max_correspondence_distance=1.0)
    T_world, key, poses = np.eye(4), None, []
    for f in range(frames):
        cloud = api.voxelgrid_sampling(api.PointCloud(synthetic.kitti_like_scan(f)[0], ctx=ctx), 0.25)
        ctx.synchronize()
        tree = api.KdTree(cloud)
        api.estimate_covariances(cloud, tree, 20)
        if key is not None:
            p, o = np.ascontiguousarray(T_world[:3, 3]), np.zeros(3)
            sga.load().sga_choose_origin(api._dp(p), api._dp(p), api._dp(o))
            target = api.KdTree(api.merge_clouds([key], [np.eye(4)], origin=o, ctx=ctx))
            init = T_world.copy()
            T_world = api.Problem(target, tree, init).align(setting, init).T_target_source
        else:
            key = cloud
        poses.append(T_world.copy())
    ctx.set_stream_ordered(False)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first["estimated"], poses))
    some = odometry.run_synthetic_submap(frames, window=3, keyframe_overlap=0.9)
    print("fitness per registered scan (overlap_distance = the downsampling resolution, window 3): every scan a keyframe", ["%.4f" % v for v in every["fitness"]],
          "| threshold 0.9:", ["%.4f" % v for v in some["fitness"]], "keyframes", some["keyframes_added"], "| first scan only:", ["%.4f" % v for v in first["fitness"]])


# ---- 9. the C++ header ----------------------------------------------------------------------------------------------------------------------
def test_cpp_overlap(tmp_path):
    """include/small_gicp_amd.hpp: Overlap and PointCloud::overlap against the C-ABI call (tests/cpp/test_cpp_cloud_overlap.cpp, compiled
    with g++ as test_cloud_outliers_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_overlap"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_overlap.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    (tmp_path / "p.f32").write_bytes(synthetic_thinned().tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    out = [r for r in rows if r[0] == "OVERLAP"]
    assert [(r[1], r[3]) for r in out] == [(t, k) for k in "012" for t in ("kd", "map")]
    for r in out:  # OVERLAP target keep k points n matched m stats s kept k arrays a cloud c
        assert 0 < int(r[7]) < int(r[5]) and r[9] == "1" and r[11] == "1" and r[13] == "1" and r[15] == "1", r
    assert [r for r in rows if r[0] == "REFUSE"] == [["REFUSE", "equal", "1"]]

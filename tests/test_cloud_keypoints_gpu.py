"""ISS keypoints and the descriptor gather on the device (csrc/cloud_keypoints.hip, cloud_fpfh.hip: sga_cloud_iss_keypoints,
sga_features_select) against the float64 restatement of tests/keypoints_ref.py, which never goes through the
library.

The comparison rule.  The restatement marks its BAND (keypoints_ref.py says how), and every case first asserts ON THE RESTATEMENT that
the band holds at most 1 % of the points (if it ever fails: another seed, never a looser comparison).  On random clouds it also asserts
that the restatement has no exact tie — two salient points of one window with the same bytes: such an accident of numpy's rounding,
which the band's definition passes, says nothing about the device's rounding; only where every sum is exact (the lattice, duplicated
points) is a tie the same tie on both sides.  Outside the band: the keypoint set EQUAL, the indices ascending, the cloud of keep byte
for byte selected(indices), every saliency within 1e-12 l1_i of the restatement's and zero exactly where the restatement's is zero.
The seeds below were chosen on the CPU for an empty band.

The 10 m square of the issue's sizes holds almost no neighbours below a few hundred points, so each small size runs a second time on a
square of the 2000-point cloud's density (20 / m^2), where the kernels have something to decide.

Observed on the MI355X: the greatest saliency deviation outside the band, over all cases, is 5.0e-16 l1."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
from scipy.spatial import cKDTree

import global_ref
import keypoints_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import api, synthetic
from conftest import ROOT
from test_cloud_merge_gpu import attributes, records, upload_relative
# the terrain pair of the end-to-end case, its truth and its preprocessing: test_global_registration_gpu.py's own (cached there, so the
# two files share one preprocessing and one set of restated descriptors in a run of the whole suite)
from test_global_registration_gpu import ABOVE, T_TRUE, VOXEL, preprocessed, restated_pairs, terrain_pair

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = np.zeros(3)
TOL = 1e-12  # of l1_i: this project's band; sums of at most a few thousand exact differences and a Jacobi solve stay orders of magnitude below


@functools.lru_cache(maxsize=None)
def surface(n, seed, side=10.0):
    p = ref.bumpy_surface(n, seed, side)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def restated(n, seed, side, salient_radius, non_max_radius, min_neighbors=5):
    return ref.iss(surface(n, seed, side), salient_radius, non_max_radius, min_neighbors=min_neighbors)


def check(p, got, want, what, cloud=None, exact_ties=False):
    """the device's result `got` (PointCloud.iss_keypoints with keep and return_saliency) against the restatement `want`; -> the greatest
    saliency deviation outside the band in units of l1"""
    n = len(p)
    band = want["band"]
    assert band.sum() <= 0.01 * n, (what, "the restatement has %d of %d points in the band" % (band.sum(), n))
    assert exact_ties or want["ties"] == 0, (what, "the restatement has %d exact ties" % want["ties"])
    good = ~band
    idx, sal = got["indices"], got["saliency"]
    assert idx.dtype == np.int64 and got["count"] == len(idx) and np.all(np.diff(idx) > 0), what  # ascending
    is_kp = np.zeros(n, bool)
    is_kp[idx] = True
    assert np.array_equal(is_kp[good], want["keypoint"][good]), (what, np.flatnonzero((is_kp != want["keypoint"]) & good)[:5])
    assert sal.shape == (n,) and sal.dtype == np.float64 and np.all(sal >= 0.0), what
    dev = np.abs(sal - want["saliency"])
    worst = float((dev[good & (want["l1"] > 0)] / want["l1"][good & (want["l1"] > 0)]).max()) if (good & (want["l1"] > 0)).any() else 0.0
    print("%s: n %d, %d keypoints (restatement %d), %d salient, band %d, ties %d, greatest saliency deviation %.3e l1" % (
        what, n, len(idx), len(want["indices"]), (sal > 0).sum(), band.sum(), want["ties"], worst))
    assert np.all(dev[good] <= TOL * want["l1"][good]), (what, worst)
    assert np.array_equal(sal[good] == 0.0, want["saliency"][good] == 0.0), what
    assert (sal[idx] > 0.0).all(), what
    if cloud is not None:
        out = got["cloud"]
        sel = cloud.selected(idx)
        assert out.size() == len(idx) and np.array_equal(out.origin(), cloud.origin()), what
        assert out.points().tobytes() == sel.points().tobytes(), what
        for a, b in zip(attributes(out), attributes(sel)):
            assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes()), what
    return worst


def run(p, salient_radius, non_max_radius, origin=ZERO, tree="given", normals=None, **kw):
    cloud = upload_relative(p, normals, None, origin) if len(p) else sga.PointCloud(np.zeros((0, 3), F32))
    t = sga.KdTree(cloud) if tree == "given" and len(p) else None
    return cloud, cloud.iss_keypoints(salient_radius, non_max_radius, tree=t, keep=True, return_saliency=True, **kw)


# ---- sizes ---------------------------------------------------------------------------------------------------------------------------------
SPARSE = {0: 1, 1: 1, 4: 1, 5: 1, 6: 1, 63: 1, 64: 1, 65: 1, 129: 1379, 2000: 2}  # n -> seed: the 10 m square at radii (1.0, 0.5)
DENSE = {4: (67, 2.0), 5: (796, 2.0), 6: (48, 1.5), 63: (3, None), 64: (13, None), 65: (6, None), 129: (3, None)}  # n -> (seed, side): radii (0.5, 0.3), min_neighbors 3


@pytest.mark.parametrize("n", sorted(SPARSE))  # around min_neighbors, a wave and a workgroup
def test_sizes_in_the_ten_metre_square(n):
    seed = SPARSE[n]
    p = surface(n, seed)
    normals = np.tile(np.array([[0.0, 0.0, 1.0]], F32), (n, 1)) if n == 2000 else None
    cloud, got = run(p, 1.0, 0.5, normals=normals)
    check(p, got, restated(n, seed, 10.0, 1.0, 0.5), "n %d" % n, cloud)
    if n < 5:
        assert got["count"] == 0 and not got["saliency"].any() and got["cloud"].size() == 0  # fewer points than min_neighbors
    if n == 2000:
        assert got["count"] > 20 and got["cloud"]._has()[0]


@pytest.mark.parametrize("n", sorted(DENSE))
def test_small_sizes_at_the_density_of_the_large_cloud(n):
    seed, side = DENSE[n]
    side = side or max(1.5, float(np.sqrt(n / 20.0)))
    p = surface(n, seed, side)
    want = restated(n, seed, side, 0.5, 0.3, 3)
    assert (want["saliency"] > 0).any()
    cloud, got = run(p, 0.5, 0.3, min_neighbors=3)
    check(p, got, want, "dense n %d" % n, cloud)
    if n >= 5:
        assert got["count"] >= 1


# ---- radii ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, radii", [(14, (0.7, 0.7)), (2, (1.0, 1.5)), (2, (1.0, 30.0))], ids=["equal", "window-wider", "window-over-the-cloud"])
def test_radii(seed, radii):
    p = surface(2000, seed)
    cloud, got = run(p, *radii)
    want = restated(2000, seed, 10.0, *radii)
    check(p, got, want, "radii %s" % (radii,), cloud)
    if radii[1] > 20.0:  # every point is in every window: the one keypoint is the greatest saliency of the cloud
        assert got["count"] == 1 and got["indices"][0] == np.argmax(got["saliency"]) == np.argmax(want["saliency"])


def test_a_salient_radius_over_the_whole_cloud_and_one_below_the_spacing():
    p = surface(2000, 2)
    # every neighbourhood is the whole cloud: one covariance, 2000 saliencies that differ by rounding alone — the whole cloud is in the band,
    # so only what holds for any rounding is asserted: one keypoint or none
    cloud, got = run(p, 30.0, 30.0)
    assert got["count"] <= 1 and got["cloud"].size() == got["count"]
    s = got["saliency"]
    assert ((s > 0).all() or not s.any()) and s.max() - s.min() <= 1e-9 * s.max()
    # below the smallest spacing (0.1 m by construction): every c_i = 1
    for mn, count in ((2, 0), (5, 0)):
        cloud, got = run(p, 1e-3, 1e-3, min_neighbors=mn)
        assert got["count"] == count and not got["saliency"].any() and got["cloud"].size() == 0
    cloud, got = run(p, 1e-3, 1e-3, min_neighbors=1)  # a lone point has no scatter: l1 = 0
    assert got["count"] == 0 and not got["saliency"].any()


# ---- exact ties -----------------------------------------------------------------------------------------------------------------------------
def test_integer_lattice():
    """12 x 12 x 3 points with integer coordinates, spaced 1, 2 and 3 (unequal, so that no symmetry of the lattice swaps two axes: a
    mirror image changes signs alone, which no rounding sees).  Every sum is exact, so equal neighbourhoods — equal sets of offsets — give
    bytewise-equal saliencies, and rule 4's ties go to the lowest index on the device as in the restatement."""
    x, y, z = np.meshgrid(np.arange(12) * 1, np.arange(12) * 2, np.arange(3) * 3, indexing="ij")
    p = np.ascontiguousarray(np.column_stack([x.ravel(), y.ravel(), z.ravel()]), dtype=F32)
    cloud, got = run(p, 3.5, 2.5, min_neighbors=1)
    want = ref.iss(p, 3.5, 2.5, min_neighbors=1)
    assert want["ties"] > 100
    check(p, got, want, "lattice", cloud, exact_ties=True)
    assert np.array_equal(got["indices"], want["indices"]) and got["count"] >= 2
    pi = p.astype(np.int64)
    groups = {}
    for i, nb in enumerate(cKDTree(p.astype(np.float64)).query_ball_point(p.astype(np.float64), 3.5)):  # (no d2 is 12.25)
        off = pi[np.asarray(nb)] - pi[i]
        groups.setdefault(off[np.lexsort(off.T)].tobytes(), []).append(i)
    assert 10 < len(groups) < len(p)
    for members in groups.values():
        assert len(set(got["saliency"][members].tolist())) == 1


def test_duplicated_points():
    base = surface(1000, 1, 7.0)
    p = np.ascontiguousarray(np.vstack([base, base[:200]]))
    cloud, got = run(p, 1.0, 0.5)
    want = ref.iss(p, 1.0, 0.5)
    assert want["ties"] >= 2
    check(p, got, want, "duplicates", cloud, exact_ties=True)
    s = got["saliency"]
    assert s[:200].tobytes() == s[1000:].tobytes() and (s[:200] > 0).any()  # each copy has its twin's saliency
    assert got["count"] > 0 and (got["indices"] < 1000).all()  # only the lower index can be a keypoint


# ---- frames, trees, repeats -------------------------------------------------------------------------------------------------------------------
def test_far_origin_and_temporary_tree():
    p = surface(2000, 2)
    near_cloud, near = run(p, 1.0, 0.5)
    far_cloud, far = run(p, 1.0, 0.5, origin=np.array([256000.0, -128000.0, 512.0]))
    assert far["saliency"].tobytes() == near["saliency"].tobytes() and np.array_equal(far["indices"], near["indices"])  # the origin never enters
    assert far["cloud"].points().tobytes() == far_cloud.selected(far["indices"]).points().tobytes()
    temp_cloud, temp = run(p, 1.0, 0.5, tree=None)
    assert temp["saliency"].tobytes() == near["saliency"].tobytes() and temp["indices"].tobytes() == near["indices"].tobytes()
    assert temp["cloud"].points().tobytes() == near["cloud"].points().tobytes()
    got = sga.iss_keypoints(p, 1.0, 0.5)  # the free function over an array: the cloud about an origin of the library's choosing
    assert set(got) == {"indices", "count"} and got["count"] == len(got["indices"])


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("return_saliency", [False, True])
@pytest.mark.parametrize("given", [False, True])
def test_two_calls_give_the_same_bytes_and_the_launches_do_not_grow(keep, return_saliency, given):
    p = surface(2000, 2)
    cloud = upload_relative(p, None, None, ZERO)
    tree = sga.KdTree(cloud) if given else None
    results, counts = [], []
    for _ in range(2):
        before = (sga.iss_launches(), sga.iss_waits())
        results.append(cloud.iss_keypoints(1.0, 0.5, tree=tree, keep=keep, return_saliency=return_saliency))
        counts.append((sga.iss_launches() - before[0], sga.iss_waits() - before[1]))
    # the saliencies and the suppression, then the listing kernel — or, with a cloud, the compaction's table copy and the compaction; one wait
    assert counts == [(4 if keep else 3, 1)] * 2, counts
    a, b = results
    assert set(a) == {"indices", "count"} | ({"cloud"} if keep else set()) | ({"saliency"} if return_saliency else set())
    assert a["indices"].tobytes() == b["indices"].tobytes() and a["count"] == b["count"] == len(restated(2000, 2, 10.0, 1.0, 0.5)["indices"])
    if return_saliency:
        assert a["saliency"].tobytes() == b["saliency"].tobytes()
    if keep:
        assert a["cloud"].points().tobytes() == b["cloud"].points().tobytes()


def test_an_empty_cloud_launches_nothing():
    before = (sga.iss_launches(), sga.iss_waits())
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    got = empty.iss_keypoints(1.0, 0.5, return_saliency=True)
    assert got["count"] == 0 and got["indices"].shape == (0,) and got["saliency"].shape == (0,)
    got = empty.iss_keypoints(1.0, 0.5, keep=True)
    assert got["count"] == 0 and got["cloud"].size() == 0
    assert (sga.iss_launches(), sga.iss_waits()) == before


def test_refusals_through_the_live_library():
    p = surface(2000, 2)
    cloud = upload_relative(p, None, None, ZERO)
    before = (sga.iss_launches(), sga.iss_waits())
    with pytest.raises(sga.SgaError, match="index was built over a cloud of 1999 points, got 2000"):
        cloud.iss_keypoints(1.0, 0.5, tree=sga.KdTree(upload_relative(p[:1999], None, None, ZERO)))
    with pytest.raises(sga.SgaError, match="device frames differ"):
        cloud.iss_keypoints(1.0, 0.5, tree=sga.KdTree(upload_relative(p, None, None, np.array([128.0, 0.0, 0.0]))))
    bad = p.copy()
    bad[17, 1] = np.nan
    with pytest.raises(sga.SgaError, match="contains non-finite coordinates"):
        upload_relative(bad, None, None, ZERO).iss_keypoints(1.0, 0.5)
    with pytest.raises(sga.SgaError, match="salient_radius must be finite"):
        cloud.iss_keypoints(0.0, 0.5)
    assert (sga.iss_launches(), sga.iss_waits()) == before  # nothing was enqueued


# ---- the descriptor gather ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [33, 7])
def test_features_selected(D):
    rows = np.random.default_rng(40 + D).uniform(0, 100, (2000, D)).astype(F32)
    f = sga.Features.from_array(rows)
    g = np.random.default_rng(41)
    for m in (0, 1, 64, 65, 1000):
        idx = np.sort(g.permutation(2000)[:m]).astype(np.int64)
        s = f.selected(idx)
        assert s.size() == m and s.dim == D and s.numpy().tobytes() == rows[idx].tobytes(), m
    idx = np.array([5, 5, 1999, 0, 5, 1999], np.int64)  # repeats, in any order
    assert f.selected(idx).numpy().tobytes() == rows[idx].tobytes()
    assert f.selected(idx).selected([2, 2]).numpy().tobytes() == rows[[1999, 1999]].tobytes()
    with pytest.raises(sga.SgaError, match=r"indices\[3\] = 2000 is outside the 2000 rows"):
        f.selected([0, 1, 2, 2000])
    with pytest.raises(sga.SgaError, match=r"indices\[0\] = -1 is outside the 2000 rows"):
        f.selected([-1])
    none = sga.Features.from_array(np.zeros((0, D), F32))
    assert none.selected([]).size() == 0 and none.selected([]).dim == D
    assert f.numpy().tobytes() == rows.tobytes()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
SALIENT, NON_MAX = 3.0 * VOXEL, 1.5 * VOXEL  # the keypoint defaults of global_align


@functools.lru_cache(maxsize=None)
def restated_keypoint_pairs():
    """the restatement's keypoints of the two downsampled clouds (the device's records are the inputs), and its mutual pairs over the
    keypoints' rows of the restated descriptors, as cloud indices"""
    tgt, _, src, _ = preprocessed()
    ft, fs, _, _ = restated_pairs()
    kt, ks = ref.iss(records(tgt)[0], SALIENT, NON_MAX), ref.iss(records(src)[0], SALIENT, NON_MAX)
    m = global_ref.match(fs["rows"].astype(F32)[ks["indices"]], ft["rows"].astype(F32)[kt["indices"]], True)
    keep = np.flatnonzero(m["match"] >= 0)
    return kt, ks, np.stack([ks["indices"][keep], kt["indices"][m["match"][keep]]], axis=1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_to_end_pose_with_keypoints(seed):
    tgt, ttree, src, stree = preprocessed()
    kt, ks, pairs = restated_keypoint_pairs()
    setting = sga.make_setting("GICP")
    # 1, 2: the restatement first — its winner, refitted by numpy, lies in the basin
    ps, pt = src.xyz64()[pairs[:, 0]], tgt.xyz64()[pairs[:, 1]]
    true = np.linalg.norm(ps @ T_TRUE[:3, :3].T + T_TRUE[:3, 3] - pt, axis=1) < 1.5 * VOXEL
    want = global_ref.ransac(ps, pt, 1.5 * VOXEL, 20000, seed, 0.9, 2.0 * VOXEL)
    b = want["best"]
    inl = np.linalg.norm(ps @ want["R"][b].T + want["t"][b] - pt, axis=1) <= 1.5 * VOXEL
    dt, dr = global_ref.pose_error(global_ref.kabsch(ps[inl], pt[inl]), T_TRUE)
    print("seed %d restatement: keypoints %d / %d (band %d / %d), %d pairs of which %d true, best %d with %d inliers, coarse error %.3f m %.3f deg" % (
        seed, len(ks["indices"]), len(kt["indices"]), ks["band"].sum(), kt["band"].sum(), len(pairs), true.sum(), b, inl.sum(), dt, np.rad2deg(dr)))
    assert dt < 0.5 and dr < np.deg2rad(5.0)
    # 3: the device, through global_align
    target, source = terrain_pair()
    coarse, refined = sga.global_align(target, source, VOXEL, k=20, iterations=20000, seed=seed, refine=True, setting=setting, viewpoint=ABOVE, keypoints=True)
    dt, dr = global_ref.pose_error(coarse["T"], T_TRUE)
    print("seed %d device: keypoints %s, %d pairs, best %d with %d inliers, coarse error %.3f m %.3f deg" % (seed, coarse["keypoints"], len(coarse["pairs"]), coarse["best_hypothesis"], coarse["inliers"], dt, np.rad2deg(dr)))
    assert dt < 0.5 and dr < np.deg2rad(5.0) and coarse["refit"] == 1
    # 4: refined — the pose align reaches from the truth, within twice the termination tolerances
    from_truth = sga.Problem(ttree, src, T_TRUE).align(setting, T_TRUE)
    tol_t, tol_r = 2 * setting.translation_eps, 2 * setting.rotation_eps
    dt, dr = global_ref.pose_error(refined.T_target_source, from_truth.T_target_source)
    print("seed %d refined against align from the truth: %.2e m %.2e rad (allowed %.1e, %.1e)" % (seed, dt, dr, tol_t, tol_r))
    assert dt <= tol_t and dr <= tol_r
    # 5: the keypoints are the restatement's outside its band, so the counts are equal up to the band (the clouds are given here, not
    # chosen: a voxel grid's centroids leave 0.5 % and 1.4 % of these two in the band, most of them through a neighbour's near-tie)
    for cloud, tree, k, n_dev in ((src, stree, ks, coarse["keypoints"][0]), (tgt, ttree, kt, coarse["keypoints"][1])):
        got = cloud.iss_keypoints(SALIENT, NON_MAX, tree=tree)
        is_kp = np.zeros(cloud.size(), bool)
        is_kp[got["indices"]] = True
        assert np.array_equal(is_kp[~k["band"]], k["keypoint"][~k["band"]])
        assert n_dev == got["count"] and abs(n_dev - len(k["indices"])) <= (k["band"] & (is_kp | k["keypoint"])).sum()
    # 6: far fewer pairs than points, and they name points of the clouds
    assert len(coarse["pairs"]) < 0.1 * min(src.size(), tgt.size())
    assert coarse["pairs"][:, 0].max() < src.size() and coarse["pairs"][:, 1].max() < tgt.size() and np.all(np.diff(coarse["pairs"][:, 0]) > 0)


def test_global_align_without_keypoints_is_unchanged():
    target, source = terrain_pair()
    setting = sga.make_setting("GICP")
    a, ra = sga.global_align(target, source, VOXEL, k=20, seed=1, setting=setting, viewpoint=ABOVE, keypoints=None)
    b, rb = sga.global_align(target, source, VOXEL, k=20, seed=1, setting=setting, viewpoint=ABOVE)
    assert set(a) == set(b) and "keypoints" not in a
    assert all(np.asarray(a[w]).tobytes() == np.asarray(b[w]).tobytes() for w in a)
    assert ra.T_target_source.tobytes() == rb.T_target_source.tobytes() and ra.iterations == rb.iterations
    with pytest.raises(ValueError):
        sga.global_align(target, source, VOXEL, keypoints=False)
    c, _ = sga.global_align(target, source, VOXEL, k=20, seed=1, refine=False, viewpoint=ABOVE, keypoints=dict(salient_radius=SALIENT, non_max_radius=NON_MAX))
    d, _ = sga.global_align(target, source, VOXEL, k=20, seed=1, refine=False, viewpoint=ABOVE, keypoints=True)
    assert c["keypoints"] == d["keypoints"] and c["pairs"].tobytes() == d["pairs"].tobytes() and c["T"].tobytes() == d["T"].tobytes()


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_keypoints(tmp_path):
    """include/small_gicp_amd.hpp: IssParams, Keypoints, PointCloud::iss_keypoints and Features::selected
    (tests/cpp/test_cpp_cloud_keypoints.cpp, compiled with g++ as test_cloud_outliers_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_keypoints"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_keypoints.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts = np.ascontiguousarray(synthetic.bumpy_terrain(20000, 4), dtype=F32)
    (tmp_path / "p.f32").write_bytes(pts.tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32"), "1.5", "0.75"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    out = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines()}
    # the same chain through Python gives the same numbers
    cloud, tree = sga.preprocess_points(pts, 0.25, 10)
    got = cloud.iss_keypoints(1.5, 0.75, tree=tree, return_saliency=True)
    k = out["KEYPOINTS"]  # points n count c first i last j salient s nms . tree . keep .
    assert got["count"] > 10
    assert [int(k[1]), int(k[3]), int(k[5]), int(k[7]), int(k[9])] == [cloud.size(), got["count"], got["indices"][0], got["indices"][-1], int((got["saliency"] > 0).sum())]
    assert k[10:] == ["nms", "1", "tree", "1", "keep", "1"], k
    assert out["SELECT"] == ["rows", str(2 * got["count"]), "dim", "33", "equal", "1"]
    assert out["REFUSE"] == ["gamma", "1", "index", "1"]

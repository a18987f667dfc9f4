"""Outliers removed on the device (csrc/cloud_outliers.hip: sga_cloud_remove_outliers) against the fp64
restatement of tests/outliers_ref.py, which never goes through the library.

Inputs: two jittered planes (sigma = 0.02 m) plus uniform scatter, shuffled, fp32, fixed seeds (outliers_ref.planes_with_scatter); their
records are known exactly — uploaded relative to a named origin (tests/test_cloud_merge_gpu.py: upload_relative).

The comparison rule.  The device's distances are the search's fp32 squared distances, which carry a few ulp: at most ~2.5e-7 relative on
d, mean and threshold.  Values are compared at 1e-6 relative (4 x).  A point with |d_i - threshold| <= 1e-5 threshold may fall either
way; at most 2 such points per cloud are allowed, and every test asserts that cap ON THE REFERENCE before it compares (if it ever fails:
another seed, never a looser comparison).  Reference figures for the six main cases, from the restatement on the CPU:
    seed 1  n 3000  k 10  std_mul 1     94 removed  0 band points        seed 4  n 4000 (no scatter)  k 10  std_mul 1   624 removed  1 band point
    seed 2  n 3000  k 20  std_mul 2     87 removed  0                    seed 1  n 3000  k 5  radius 0.5 m              171 removed  0
    seed 3  n  730  k 63  std_mul 1     42 removed  0                    seed 1  n 3000  k 3  radius 1.0 m               95 removed  0
Both search routes are forced through sga_set_knn_wave_max; on the lane route k = 10 and 20 keep their list in registers and every other
k in LDS, so the route tests take k from both groups.  Everything but the band points is exact: kept equals the restatement's list, kept is ascending, and output record j is input record
kept[j] bit for bit in point, normal and covariance."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import outliers_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import api
from conftest import ROOT
from test_cloud_merge_gpu import attributes, records, upload_relative

pytestmark = pytest.mark.gpu

F32 = np.float32
RTOL = 1e-6
WAVE_DEFAULT = 81920
ZERO = np.zeros(3)
CASES = [  # (seed, points per plane, scatter, k, std_mul, radius)
    (1, 1450, 100, 10, 1.0, None),
    (2, 1450, 100, 20, 2.0, None),
    (3, 340, 50, 63, 1.0, None),
    (4, 2000, 0, 10, 1.0, None),
    (1, 1450, 100, 5, 1.0, 0.5),
    (1, 1450, 100, 3, 1.0, 1.0),
]


# ---- inputs and references, computed once -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points(seed, n_plane=1450, n_scatter=100, n=None):
    p = ref.planes_with_scatter(seed, n_plane, n_scatter)
    p = p if n is None else np.ascontiguousarray(p[:n])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference(seed, n_plane, n_scatter, n, k, std_mul, radius):
    return ref.restate(points(seed, n_plane, n_scatter, n), k, std_mul, radius)


def attributes_for(n, seed=99):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    nrm = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)
    a = rng.normal(size=(n, 3, 3)) * 0.05
    return nrm, api.sym6_from_mats(a @ a.transpose(0, 2, 1) + 1e-4 * np.eye(3)).astype(F32)


# ---- the comparison -----------------------------------------------------------------------------------------------------------------------
def close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b)) | (np.abs(a - b) <= RTOL * np.abs(b))))


def run(cloud, k, std_mul=1.0, radius=None, tree=None):
    out, kept, st = cloud.without_outliers(k, std_mul, radius, tree, return_kept=True, return_stats=True)
    return out, kept, st


def check(got, want, rel, nrm=None, cov6=None, origin=ZERO, what=""):
    """the call's results `got` = (out, kept, stats) against the restatement `want` of the records `rel`"""
    out, kept, st = got
    edge = ref.band(want)
    assert len(edge) <= ref.MAX_BAND_POINTS, (what, "the reference has %d points in the band" % len(edge))
    fin = np.isfinite(want["stat"])
    rel_err = np.abs(st["stat"][fin] - want["stat"][fin]) / np.maximum(want["stat"][fin], 1e-300)
    print("%s n %d: removed %d (reference %d), band %d, stat rel err max %.2e, mean %.9g (%.9g) stddev %.9g (%.9g) threshold %.9g (%.9g)"
          % (what, len(rel), len(rel) - len(kept), len(rel) - len(want["kept"]), len(edge), rel_err.max() if len(rel_err) else 0.0, st["mean"], want["mean"], st["stddev"], want["stddev"], st["threshold"], want["threshold"]))
    assert st["stat"].dtype == np.float64 and close(st["stat"], want["stat"]), what
    assert close(st["mean"], want["mean"]) and close(st["stddev"], want["stddev"]) and close(st["threshold"], want["threshold"]), what
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0), what  # ascending
    assert np.all(np.isin(np.setxor1d(kept, want["kept"]), edge)), (what, np.setxor1d(kept, want["kept"]))
    assert st["kept"] == len(kept) == out.size(), what
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


class Route:
    """every call inside takes the wave-per-query route (True) or the lane-per-query route (False)"""

    def __init__(self, wave):
        self.wave = wave

    def __enter__(self):
        sga.load().sga_set_knn_wave_max(C.c_longlong(1 << 40 if self.wave else 0))

    def __exit__(self, *exc):
        sga.load().sga_set_knn_wave_max(C.c_longlong(WAVE_DEFAULT))


# ---- results ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: "seed%d-n%d-k%d-%s" % (c[0], 2 * c[1] + c[2], c[3], "std%g" % c[4] if c[5] is None else "r%g" % c[5]))
def test_results_match_the_restatement(case):
    seed, n_plane, n_scatter, k, std_mul, radius = case
    rel = points(seed, n_plane, n_scatter)
    want = reference(seed, n_plane, n_scatter, None, k, std_mul, radius)
    nrm, cov6 = attributes_for(len(rel)) if seed == 1 else (None, None)
    cloud = upload_relative(rel, nrm, cov6, ZERO)
    check(run(cloud, k, std_mul, radius), want, rel, nrm, cov6, what=str(case))
    assert len(want["kept"]) < len(rel)  # something is removed: the test is about a filter
    # the optional outputs are optional, and the module function takes an array
    assert cloud.without_outliers(k, std_mul, radius).size() == len(want["kept"]) or len(ref.band(want)) > 0
    assert sga.remove_outliers(rel, k, std_mul, radius).size() == cloud.without_outliers(k, std_mul, radius).size()


@pytest.mark.parametrize("k, radius", [(10, None), (20, None), (7, None), (5, 0.5), (10, 1.0), (20, 1.5)])  # the lane route keeps k = 10 / 20 in registers
def test_both_routes_match_and_agree(k, radius):
    rel = points(1)
    want = reference(1, 1450, 100, None, k, 1.0, radius)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(cloud)
    got = {}
    for wave in (True, False):
        with Route(wave):
            got[wave] = run(cloud, k, 1.0, radius, tree)
        check(got[wave], want, rel, what="wave route" if wave else "lane route")
    assert close(got[True][2]["stat"], got[False][2]["stat"])


@pytest.mark.parametrize("k, std_mul", [(1, 1.0), (63, 1.0), (10, 0.0)])
def test_k_extremes(k, std_mul):
    rel = points(1)
    cloud = upload_relative(rel, None, None, ZERO)
    for wave in (True, False):
        with Route(wave):
            got = run(cloud, k, std_mul)
        check(got, reference(1, 1450, 100, None, k, std_mul, None), rel, what="k %d std_mul %g wave %d" % (k, std_mul, wave))


@pytest.mark.parametrize("wave", [True, False], ids=["wave", "lane"])
@pytest.mark.parametrize("n", [1, 2, 10, 11, 64, 65, 2048, 2049, 4097])  # k, k + 1 with k = 10; a wave; the compaction's tile edges
def test_boundary_sizes(n, wave):
    rel = points(5, 2100, 100, n)
    cloud = upload_relative(rel, None, None, ZERO)
    with Route(wave):
        got = run(cloud, 10, 1.0)
        rad = run(cloud, 10, 1.0, 1.0) if n <= 65 else None
    check(got, reference(5, 2100, 100, n, 10, 1.0, None), rel, what="n %d" % n)
    if n <= 2:  # d_0 = 0, or d_0 == d_1 from one symmetric distance: the arithmetic is exact and every point sits ON the threshold
        assert got[0].size() == n and got[2]["stddev"] == 0.0 and got[2]["threshold"] == got[2]["mean"] == got[2]["stat"][0]
    if rad is not None:
        check(rad, reference(5, 2100, 100, n, 10, 1.0, 1.0), rel, what="radius, n %d" % n)
        if n <= 10:  # no point has k others: d = +inf, everything goes
            assert np.all(np.isinf(rad[2]["stat"])) and rad[0].size() == 0 and rad[2]["threshold"] == 1.0


def test_a_far_device_frame_has_the_same_keep_set():
    # coordinates on a 2^-10 m lattice: shifted by (1e6, -2e6, 5e5) m and stored about the origin the library chooses (a multiple of 128 m)
    # the records are the near cloud's up to an exact translation, so distances — and with them every figure — are the same bits
    near = (np.round(points(1).astype(np.float64) * 1024.0) / 1024.0).astype(F32)
    want = ref.restate(near, 10, 1.0)
    assert len(ref.band(want)) == 0
    shift = np.array([1e6, -2e6, 5e5])
    far = sga.PointCloud(near.astype(np.float64) + shift)  # float64 points: sga_cloud_create_f64
    assert far.origin().any()
    rec, _ = records(far)
    assert np.array_equal(rec.astype(np.float64) + far.origin(), near.astype(np.float64) + shift)  # the records are exact
    a = run(upload_relative(near, None, None, ZERO), 10, 1.0)
    b = run(far, 10, 1.0)
    check(a, want, near, what="near")
    check(b, want, rec, origin=far.origin(), what="far")
    assert np.array_equal(a[1], b[1]) and a[2]["stat"].tobytes() == b[2]["stat"].tobytes()


def test_callers_tree_equals_a_temporary_tree_and_the_command_count_does_not_grow():
    rel = points(1)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(cloud)
    before = sga.cloud_outliers_launches()
    with_tree = run(cloud, 10, 1.0, tree=tree)
    count_3000 = sga.cloud_outliers_launches() - before
    temporary = run(cloud, 10, 1.0)
    assert np.array_equal(with_tree[1], temporary[1]) and with_tree[2]["stat"].tobytes() == temporary[2]["stat"].tobytes()
    assert [with_tree[2][w] for w in ("mean", "stddev", "threshold", "kept")] == [temporary[2][w] for w in ("mean", "stddev", "threshold", "kept")]
    big = upload_relative(np.concatenate([rel, rel + F32(30.0), rel - F32(30.0)]), None, None, ZERO)
    big_tree = sga.KdTree(big)
    before = sga.cloud_outliers_launches()
    out = big.without_outliers(10, 1.0, tree=big_tree)
    count_9000 = sga.cloud_outliers_launches() - before
    assert 0 < out.size() < 9000
    assert count_3000 == count_9000 and 1 <= count_3000 <= 4, (count_3000, count_9000)
    before = sga.cloud_outliers_launches()  # radius mode without stats has no threshold step
    cloud.without_outliers(5, radius=0.5, tree=tree)
    assert sga.cloud_outliers_launches() - before == count_3000 - 1
    before_crop = sga.cloud_crop_launches()
    cloud.without_outliers(10, 1.0, tree=tree)
    assert sga.cloud_crop_launches() == before_crop  # the compaction's commands are counted here, not as a crop's


@pytest.mark.parametrize("radius", [None, 0.5])
def test_two_calls_give_the_same_bits(radius):
    cloud = upload_relative(points(2), None, None, ZERO)
    for wave in (True, False):
        with Route(wave):
            a, b = run(cloud, 10, 1.0, radius), run(cloud, 10, 1.0, radius)
        assert a[2]["stat"].tobytes() == b[2]["stat"].tobytes() and np.array_equal(a[1], b[1])
        assert np.array([a[2][w] for w in ("mean", "stddev", "threshold")]).tobytes() == np.array([b[2][w] for w in ("mean", "stddev", "threshold")]).tobytes()


def test_stream_ordered_context_and_a_tree_from_another_context():
    rel = points(1)
    want = reference(1, 1450, 100, None, 10, 1.0, None)
    plain = run(upload_relative(rel, None, None, ZERO), 10, 1.0)
    ctx, other = sga.Context(0), sga.Context(0)
    ctx.set_stream_ordered(True)
    other.set_stream_ordered(True)
    try:
        cloud = upload_relative(rel, None, None, ZERO, ctx)
        got = run(cloud, 10, 1.0)
        check(got, want, rel, what="stream-ordered")
        assert got[2]["stat"].tobytes() == plain[2]["stat"].tobytes() and np.array_equal(got[1], plain[1])
        theirs = upload_relative(rel, None, None, ZERO, other)
        tree = sga.KdTree(theirs)  # returns with its kernels in flight on the other context's stream
        got = run(cloud, 10, 1.0, tree=tree)
        check(got, want, rel, what="a tree of another context")
        assert got[2]["stat"].tobytes() == plain[2]["stat"].tobytes()
    finally:
        ctx.set_stream_ordered(False)
        other.set_stream_ordered(False)


def test_refusals():
    rel = points(1)
    cloud = upload_relative(rel, None, None, ZERO)
    before = sga.cloud_outliers_launches()
    bad = rel.copy()
    bad[17, 1] = np.nan
    with pytest.raises(sga.SgaError, match="contains non-finite coordinates"):
        upload_relative(bad, None, None, ZERO).without_outliers()
    with pytest.raises(sga.SgaError, match="index was built over a cloud of 2999 points, got 3000"):
        cloud.without_outliers(tree=sga.KdTree(upload_relative(rel[:2999], None, None, ZERO)))
    with pytest.raises(sga.SgaError, match="device frames differ"):
        cloud.without_outliers(tree=sga.KdTree(upload_relative(rel, None, None, np.array([128.0, 0.0, 0.0]))))
    assert sga.cloud_outliers_launches() == before  # nothing was enqueued
    out, kept, st = sga.PointCloud(np.zeros((0, 3), F32)).without_outliers(return_kept=True, return_stats=True)
    assert out.size() == 0 and len(kept) == 0 and len(st["stat"]) == 0 and out._has() == (False, False)
    assert (st["mean"], st["stddev"], st["threshold"], st["kept"]) == (0.0, 0.0, 0.0, 0)
    assert sga.cloud_outliers_launches() == before
    # fields of the other mode are not judged
    f = api._outlier_filter(10, 1.0)
    f.radius = float("nan")
    assert cloud.without_outliers(f).size() == cloud.without_outliers(10, 1.0).size()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def test_odometry_with_the_filter_is_the_hand_built_pipeline_and_without_it_unchanged():
    from small_gicp_amd import odometry, synthetic

    scans = [synthetic.with_isolated_returns(synthetic.kitti_like_scan(f)[0], 0.01, seed=4242 + f)[0] for f in range(3)]
    before = sga.cloud_outliers_launches()
    off = odometry.OnlineOdometry()
    poses_off = [off.estimate(s) for s in scans]
    off.close()
    assert sga.cloud_outliers_launches() == before  # off by default: no call is made
    res = odometry.run_synthetic(3, outliers=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(poses_off, res["estimated"]))
    assert sga.cloud_outliers_launches() == before
    on = odometry.OnlineOdometry(outlier_k=10)
    poses_on = [on.estimate(s) for s in scans]
    on.close()
    assert sga.cloud_outliers_launches() > before
    # by hand: voxel grid, filter, tree, covariances, registration against the previous scan from the identity
    ctx = sga.Context(0)
    ctx.set_stream_ordered(True)
    setting = api.make_setting("GICP", max_correspondence_distance=1.0)
    T_world, target, poses, removed = np.eye(4), None, [], []
    for s in scans:
        down = api.voxelgrid_sampling(api.PointCloud(s, ctx=ctx), 0.25)
        cloud = down.without_outliers(10, 1.0)
        removed.append(down.size() - cloud.size())
        tree = api.KdTree(cloud)
        api.estimate_covariances(cloud, tree, 20)
        if target is not None:
            T_world = T_world @ api.Problem(target, tree, np.eye(4)).align(setting, np.eye(4)).T_target_source
        target = tree
        poses.append(T_world.copy())
    ctx.set_stream_ordered(False)
    print("points removed per downsampled scan:", removed)
    assert all(r > 0 for r in removed)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(poses_on, poses))
    assert any(a.tobytes() != b.tobytes() for a, b in zip(poses_on, poses_off))  # the filter did take part


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_without_outliers(tmp_path):
    """include/small_gicp_amd.hpp: OutlierFilter and PointCloud::without_outliers against a host loop
    (tests/cpp/test_cpp_cloud_outliers.cpp, compiled with g++ as test_cloud_crop_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_outliers"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_outliers.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts = synthetic_thinned()
    (tmp_path / "p.f32").write_bytes(pts.tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    out = [r for r in rows if r[0] == "OUTLIERS"]
    assert len(out) == 2 and [r[1] for r in out] == ["0", "1"]
    for r in out:  # OUTLIERS mode kept m of n equal e band b relerr x gathered g tree t
        assert 0 < int(r[3]) < int(r[5]) and r[7] == "1" and int(r[9]) <= ref.MAX_BAND_POINTS and float(r[11]) <= RTOL and r[13] == "1" and r[15] == "1", r
    assert [r for r in rows if r[0] == "REFUSE"] == [["REFUSE", "equal", "1"]]


def synthetic_thinned():
    pts, _ = sga.synthetic.kitti_like_scan(0)
    return np.ascontiguousarray(sga.synthetic.with_isolated_returns(pts[::6], 0.01)[0], dtype=F32)  # every sixth point, with scatter

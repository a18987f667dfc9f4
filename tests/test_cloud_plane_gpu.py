"""Plane segmentation on the device (csrc/cloud_plane.hip) against the fp64 restatement of tests/plane_ref.py,
which never goes through the library.

The condition of every case: the restatement finds an EMPTY band in its input — no (hypothesis, record) pair within 1e-12 of the
threshold, no hypothesis whose collinearity or angle test hangs within 1e-12, no record within 1e-9 of the threshold about the final
plane (plane_ref's docstring).  That is asserted first; it is a condition on the input, not a tolerance (if it ever fails: another
seed).  Then EVERY entry of scores, the best hypothesis, its inliers, the number scored, the refit flag and the final inlier set are
compared for equality; the plane within 1e-10 rad and 1e-9 m — the distance measured at the plane's own anchor in the caller's frame,
where the two planes are compared and not 256 km away from it — and rmse within 1e-12 relative."""
import functools
import os
import subprocess

import numpy as np
import pytest

import plane_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import odometry, synthetic
from test_cloud_merge_gpu import attributes, records, upload_relative

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = (0.0, 0.0, 0.0)
FAR = (256000.0, -128000.0, 1000.0)
DROPPED = ref.DROPPED
POINT_TILE, HYP_TILE = 1024, 32  # csrc/cloud_plane.hip: kPlPointTile, kPlHypTile


# ---- inputs (fp32 records, fixed seeds) and references, computed once -------------------------------------------------------------------
def frozen(p):
    p = np.ascontiguousarray(p, dtype=F32).reshape(-1, 3)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def noisy_plane(n, seed=None):
    """n points: 70 % on a 10 m x 8 m patch of a tilted plane with 0.02 m of Gaussian noise, 30 % uniform in the box around it"""
    g = np.random.default_rng(2000 + n if seed is None else seed)
    on = n - (3 * n) // 10
    local = np.column_stack([g.uniform(-5, 5, on), g.uniform(-4, 4, on), 0.02 * g.standard_normal(on)])
    Q, _ = np.linalg.qr(g.standard_normal((3, 3)))
    p = np.concatenate([local @ Q.T + np.array([1.0, -2.0, 0.5]), g.uniform(-5, 5, (n - on, 3))])
    return frozen(g.permutation(p))


@functools.lru_cache(maxsize=None)
def wall_and_floor():
    """a 3000-point wall x = 4 and a 1500-point floor z = 0, 5 mm of noise, shuffled"""
    g = np.random.default_rng(5)
    wall = np.stack([4.0 + 0.005 * g.standard_normal(3000), g.uniform(-2.0, 2.0, 3000), g.uniform(0.0, 3.0, 3000)], axis=1)
    floor = np.stack([g.uniform(0.0, 4.0, 1500), g.uniform(-2.0, 2.0, 1500), 0.005 * g.standard_normal(1500)], axis=1)
    return frozen(g.permutation(np.concatenate([wall, floor])))


@functools.lru_cache(maxsize=None)
def with_non_finite():
    p = np.array(noisy_plane(1500, seed=31))
    g = np.random.default_rng(32)
    rows = g.choice(len(p), 90, replace=False)
    p[rows[:30]] = np.nan
    p[rows[30:50], 1] = np.inf
    p[rows[50:70], 2] = -np.inf
    p[rows[70:90], 0] = np.nan
    return frozen(p)


@functools.lru_cache(maxsize=None)
def box_faces():
    """three faces of a box with 4000, 2500 and 1200 points (1 cm of noise) and 600 outliers, shuffled"""
    g = np.random.default_rng(41)
    a = np.column_stack([g.uniform(0, 6, 4000), g.uniform(0, 5, 4000), 0.01 * g.standard_normal(4000)])
    b = np.column_stack([0.01 * g.standard_normal(2500), g.uniform(0, 5, 2500), g.uniform(0.2, 4, 2500)])
    c = np.column_stack([g.uniform(0.2, 6, 1200), 5.0 + 0.01 * g.standard_normal(1200), g.uniform(0.2, 4, 1200)])
    out = g.uniform(0.3, 4.7, (600, 3)) + np.array([0.5, 0.0, 0.0])
    return frozen(g.permutation(np.concatenate([a, b, c, out])))


@functools.lru_cache(maxsize=None)
def want(maker, args=(), threshold=0.05, iterations=100, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, origin=ZERO):
    return ref.segment_plane(maker(*args), threshold, iterations, seed, axis, max_angle, min_inliers, refit, origin)


def upload(rel, origin=ZERO, nrm=None, cov6=None):
    return upload_relative(rel, nrm, cov6, np.asarray(origin, dtype=np.float64)) if len(rel) else sga.PointCloud(np.zeros((0, 3), F32))


def compare(got, w, n, origin=ZERO, what=""):
    print("%s: n %d  scored %d (%d)  best %d (%d)  hypothesis inliers %d (%d)  inliers %d (%d)  refit %d (%d)  rmse %.6g  band %d shaky %d final band %d" % (
        what, n, got["scored"], w["scored"], got["best_hypothesis"], w["best_hypothesis"], got["hypothesis_inliers"], w["hypothesis_inliers"], got["inliers"], w["inliers"], got["refit"], w["refit"], got["rmse"],
        int(w["band"].sum()), int(w["shaky"].sum()), w["final_band"]))
    assert int(w["band"].sum()) == 0 and not w["shaky"].any() and w["final_band"] == 0 and not w["refit_shaky"], what
    assert got["scores"].dtype == np.uint32 and np.array_equal(got["scores"], w["scores"]), what
    assert got["scored"] == w["scored"], what
    if w["best_hypothesis"] >= 0:
        assert (got["best_hypothesis"], got["hypothesis_inliers"]) == (w["best_hypothesis"], w["hypothesis_inliers"]), what
    if not w["found"]:
        assert got["inliers"] == 0 and not got["plane"].any() and got["rmse"] == 0.0 and got["refit"] == 0, what
        if "cloud" in got:
            assert got["cloud"].size() == 0 and len(got["kept"]) == 0
        return
    assert (got["inliers"], got["refit"]) == (w["inliers"], w["refit"]), what
    assert np.array_equal(got["kept"], np.flatnonzero(w["inlier_mask"])), what  # the final inlier SET
    at = w["anchor"] + np.asarray(origin, dtype=np.float64)
    angle, offset = ref.plane_error(got["plane"], w["plane"], at)
    print("    plane %s: %.3e rad, %.3e m from the restatement's; rmse %.3e relative" % (np.array2string(got["plane"], precision=6), angle, offset, abs(got["rmse"] - w["rmse"]) / max(w["rmse"], 1e-300)))
    assert angle < 1e-10 and offset < 1e-9, what
    assert rmse_agrees(got["rmse"], w), what


def rmse_agrees(rmse, w):
    """rmse within 1e-12 relative of the restatement's — wherever rmse is a number.  When the plane passes through its inliers exactly
    (three points, or a hand-made flat patch) the true rmse is 0 and both sides return the rounding of their distances: a distance is
    three products of a unit normal with differences of at most `reach` metres and two sums, each rounded once, so it carries up to 5 u
    reach (u = 2^-53), the refitted anchor and normal another few u reach.  Below 1e3 u reach no digit of rmse is significant on either
    side and a relative comparison compares noise: there both have to be below 16 u reach."""
    reach = float(np.max(np.abs(w["records64"][w["inlier_mask"]] - w["anchor"]))) if w["inlier_mask"].any() else 0.0
    u = 2.0**-53
    if w["rmse"] > 1e3 * u * reach:
        return abs(rmse - w["rmse"]) <= 1e-12 * w["rmse"]
    return rmse <= 16 * u * reach and w["rmse"] <= 16 * u * reach


def run(maker, args=(), threshold=0.05, iterations=100, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, origin=ZERO, what=""):
    rel = maker(*args)
    cloud = upload(rel, origin)
    w = want(maker, args, threshold, iterations, seed, None if axis is None else tuple(axis), max_angle, min_inliers, refit, tuple(origin))
    got = cloud.segment_plane(threshold, iterations, seed, axis, max_angle, min_inliers, refit, keep="plane", return_kept=True, return_scores=True)
    compare(got, w, len(rel), origin, what or "%s%s H %d" % (maker.__name__, args, iterations))
    return cloud, got, w


# ---- sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, POINT_TILE - 1, POINT_TILE, POINT_TILE + 1, 5000])
def test_sizes_around_a_wave_a_workgroup_and_the_point_tile(n):
    cloud, got, w = run(noisy_plane, (n,), iterations=100)
    if n < 3:
        assert (got["scores"] == DROPPED).all() and got["scored"] == 0 and got["inliers"] == 0
    if n >= 63:
        assert w["found"] and w["inliers"] > n // 2


@pytest.mark.parametrize("iterations", [1, 63, 64, 65, HYP_TILE - 1, HYP_TILE, HYP_TILE + 1, 1000])
def test_iterations_around_a_wave_and_the_hypothesis_tile(iterations):
    run(noisy_plane, (1500,), iterations=iterations)


# ---- nothing to find ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line():
    t = np.arange(300.0)
    return frozen(np.column_stack([0.25 * t, -0.5 * t, 0.125 * t]))  # exact in fp32: every cross product is exactly zero


@functools.lru_cache(maxsize=None)
def identical():
    return frozen(np.tile([[1.5, -2.25, 0.75]], (200, 1)))


@pytest.mark.parametrize("maker", [line, identical])
def test_points_on_a_line_or_all_identical_have_no_plane(maker):
    cloud, got, w = run(maker, iterations=64)
    assert got["scored"] == 0 and got["inliers"] == 0 and (got["scores"] == DROPPED).all() and not got["plane"].any()
    rest = cloud.segment_plane(0.05, 64, keep="rest", return_kept=True)
    assert rest["cloud"].size() == len(maker()) and np.array_equal(rest["kept"], np.arange(len(maker()))) and rest["inliers"] == 0


def test_min_inliers_above_the_best_score():
    cloud, got, w = run(noisy_plane, (1500,), iterations=100, min_inliers=1400)
    assert not w["found"] and 3 <= w["hypothesis_inliers"] < 1400 and got["scored"] > 0
    rest = cloud.segment_plane(0.05, 100, min_inliers=1400, keep="rest", return_kept=True)
    assert rest["inliers"] == 0 and rest["cloud"].size() == 1500 and np.array_equal(records(rest["cloud"])[0], noisy_plane(1500))


# ---- the axis constraint ------------------------------------------------------------------------------------------------------------------
def test_the_axis_constraint_picks_the_floor_not_the_wall():
    _, free, wf = run(wall_and_floor, threshold=0.02, iterations=300)
    assert abs(free["plane"][0]) > 0.999 and free["inliers"] >= 2950
    _, held, wh = run(wall_and_floor, threshold=0.02, iterations=300, axis=(0.0, 0.0, 1.0), max_angle=float(np.radians(10.0)))
    assert held["plane"][2] > 0.999 and 1450 <= held["inliers"] <= 1600 and abs(held["plane"][3]) < 0.01
    assert held["scored"] == wh["scored"] < free["scored"]
    _, down, _ = run(wall_and_floor, threshold=0.02, iterations=300, axis=(0.0, 0.0, -3.0), max_angle=float(np.radians(10.0)))
    assert down["plane"][2] < -0.999 and down["inliers"] == held["inliers"] and np.array_equal(down["scores"], held["scores"])  # the normal is turned towards the axis


# ---- non-finite records -------------------------------------------------------------------------------------------------------------------
def test_non_finite_records_are_never_in_the_plane_and_always_in_the_rest():
    cloud, got, w = run(with_non_finite, iterations=200)
    bad = np.flatnonzero(~np.isfinite(with_non_finite()).all(axis=1))
    assert len(bad) == 90 and w["found"] and (w["scores"] == DROPPED).sum() > 0  # (triples with such a record are dropped)
    assert not np.isin(bad, got["kept"]).any()
    rest = cloud.segment_plane(0.05, 200, keep="rest", return_kept=True)
    assert np.isin(bad, rest["kept"]).all() and len(rest["kept"]) + len(got["kept"]) == len(with_non_finite())
    assert np.array_equal(rest["cloud"].xyz(), with_non_finite()[rest["kept"]], equal_nan=True)


# ---- a distant origin ---------------------------------------------------------------------------------------------------------------------
def test_an_origin_256_km_away_changes_nothing_but_d():
    _, near, _ = run(noisy_plane, (1500,), iterations=100)
    _, far, _ = run(noisy_plane, (1500,), iterations=100, origin=FAR)
    assert np.array_equal(near["scores"], far["scores"]) and np.array_equal(near["kept"], far["kept"])
    assert np.array_equal(near["plane"][:3], far["plane"][:3]) and near["rmse"] == far["rmse"]
    shift = float(near["plane"][:3] @ np.asarray(FAR))
    print("d %.12g -> %.12g, -n.origin %.12g, off by %.3e" % (near["plane"][3], far["plane"][3], -shift, abs(far["plane"][3] - (near["plane"][3] - shift))))
    assert abs(far["plane"][3] - (near["plane"][3] - shift)) < 1e-9


# ---- the compaction -----------------------------------------------------------------------------------------------------------------------
def test_keep_returns_the_plane_s_points_or_the_rest():
    rel = noisy_plane(5000)
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=rel.shape).astype(F32)
    cov6 = rng.uniform(0.1, 1.0, (len(rel), 6)).astype(F32)
    cloud = upload(rel, FAR, nrm, cov6)
    w = want(noisy_plane, (5000,), 0.05, 100, 0, None, 0.0, 3, True, FAR)
    kept = {}
    for keep, mask in (("plane", w["inlier_mask"]), ("rest", ~w["inlier_mask"])):
        got = cloud.segment_plane(0.05, 100, keep=keep, return_kept=True)
        idx = np.flatnonzero(mask)
        assert np.array_equal(got["kept"], idx) and got["cloud"].size() == len(idx) and 0 < len(idx) < len(rel) and np.all(np.diff(got["kept"]) > 0)
        sel = cloud.selected(idx)
        assert records(got["cloud"])[0].tobytes() == records(sel)[0].tobytes() and np.array_equal(records(got["cloud"])[0], rel[idx])
        for a, b in zip(attributes(got["cloud"]), attributes(sel)):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(got["cloud"].origin(), cloud.origin())
        kept[keep] = got["kept"]
    assert np.array_equal(np.sort(np.concatenate([kept["plane"], kept["rest"]])), np.arange(len(rel)))
    assert "kept" not in cloud.segment_plane(0.05, 100, keep="plane")


# ---- other paths --------------------------------------------------------------------------------------------------------------------------
def test_without_refit_the_triple_s_plane_is_returned():
    cloud, got, w = run(noisy_plane, (1500,), iterations=100, refit=False)
    assert got["refit"] == 0 and got["inliers"] == got["hypothesis_inliers"] == w["hypothesis_inliers"]
    tri = ref.draws(0, [got["best_hypothesis"]], 1500)[0]
    a = noisy_plane(1500)[tri[0]].astype(np.float64)
    assert abs(float(got["plane"][:3] @ a) + got["plane"][3]) < 1e-12  # the plane passes through the triple's first record
    _, fitted, _ = run(noisy_plane, (1500,), iterations=100)
    assert fitted["refit"] == 1 and fitted["rmse"] < got["rmse"]


def test_two_calls_return_the_same_bytes():
    cloud = upload(noisy_plane(5000))
    a = cloud.segment_plane(0.05, 1000, seed=3, keep="plane", return_kept=True, return_scores=True)
    b = cloud.segment_plane(0.05, 1000, seed=3, keep="plane", return_kept=True, return_scores=True)
    for name in ("plane", "scores", "kept"):
        assert a[name].tobytes() == b[name].tobytes(), name
    assert all(a[k] == b[k] for k in ("inliers", "rmse", "hypothesis_inliers", "best_hypothesis", "scored", "refit"))
    assert np.float64(a["rmse"]).tobytes() == np.float64(b["rmse"]).tobytes()
    c = cloud.segment_plane(0.05, 1000, seed=4, return_scores=True)
    assert not np.array_equal(a["scores"], c["scores"])


def test_launches_and_waits():
    cloud = upload(noisy_plane(1500))

    def counted(fn):
        before = (sga.segment_plane_launches(), sga.segment_plane_waits())
        fn()
        return tuple(a - b for a, b in zip((sga.segment_plane_launches(), sga.segment_plane_waits()), before))

    assert counted(lambda: cloud.segment_plane(0.05, 100, refit=False)) == (4, 1)
    assert counted(lambda: cloud.segment_plane(0.05, 100, refit=True)) == (5, 2)
    assert counted(lambda: cloud.segment_plane(0.05, 100, refit=False, keep="plane")) == (7, 2)
    assert counted(lambda: cloud.segment_plane(0.05, 100, refit=True, keep="rest", return_kept=True)) == (7, 2)
    assert counted(lambda: cloud.segment_plane(0.05, 100, min_inliers=1400)) == (4, 1)  # no plane: the first wait alone
    assert counted(lambda: cloud.segment_plane(0.05, 100, min_inliers=1400, keep="plane")) == (4, 1)
    assert counted(lambda: cloud.segment_plane(0.05, 100, min_inliers=1400, keep="rest")) == (6, 2)  # ... and the compaction of the whole cloud
    two = upload(noisy_plane(2))
    assert counted(lambda: two.segment_plane(0.05, 100)) == (0, 0)
    assert counted(lambda: two.segment_plane(0.05, 100, keep="plane")) == (0, 0)
    assert counted(lambda: two.segment_plane(0.05, 100, keep="rest")) == (2, 1)
    assert counted(lambda: sga.PointCloud(np.zeros((0, 3), F32)).segment_plane(0.05, 100, keep="rest")) == (0, 0)


# ---- several planes -----------------------------------------------------------------------------------------------------------------------
def test_segment_planes_finds_the_faces_of_a_box_in_order():
    rel = box_faces()
    w = ref.segment_planes(rel, 4, 0.04, 300, seed=11, min_inliers=800)
    assert w["clean"] and len(w["planes"]) == 3
    got = sga.segment_planes(upload(rel), 4, 0.04, 300, seed=11, min_inliers=800)
    sizes = [p["inliers"] for p in got["planes"]]
    print("box faces: planes %d, inliers %s (restatement %s), rest %d" % (len(got["planes"]), sizes, [p["inliers"] for p in w["planes"]], len(got["rest_indices"])))
    assert len(got["planes"]) == 3 and sizes == [p["inliers"] for p in w["planes"]]
    assert 4000 <= sizes[0] <= 4400 and 2500 <= sizes[1] <= 2800 and 1200 <= sizes[2] <= 1400  # the faces, in the order of their sizes
    assert np.array_equal(got["labels"], w["labels"]) and np.array_equal(got["rest_indices"], w["rest_indices"])
    for p, q in zip(got["planes"], w["planes"]):
        angle, offset = ref.plane_error(p["plane"], q["plane"], q["anchor"])
        assert angle < 1e-10 and offset < 1e-9 and p["best_hypothesis"] == q["best_hypothesis"]
    assert got["rest"].size() == len(w["rest_indices"]) and np.array_equal(got["rest"].xyz(), rel[w["rest_indices"]])
    fourth = got["rest"].segment_plane(0.04, 300, seed=11 + 3, min_inliers=800)
    assert fourth["inliers"] == 0 and 0 < fourth["hypothesis_inliers"] < 800


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_segment_plane_and_segment_planes(tmp_path):
    """include/small_gicp_amd.hpp: PlaneParams, PointCloud::segment_plane and segment_planes report what Python reports on the same file
    (tests/cpp/test_cpp_cloud_plane.cpp, compiled with g++ as test_cloud_cluster_gpu.py compiles its program)."""
    from conftest import ROOT

    exe = tmp_path / "test_cpp_cloud_plane"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_plane.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts = np.ascontiguousarray(box_faces())
    (tmp_path / "p.f32").write_bytes(pts.tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    cloud = sga.PointCloud(pts)
    py = cloud.segment_plane(0.05, 300, seed=7)
    (r,) = [r for r in rows if r[0] == "PLANE"]
    assert [int(r[2]), int(r[4]), int(r[6]), int(r[8]), int(r[10])] == [py["best_hypothesis"], py["hypothesis_inliers"], py["inliers"], py["scored"], py["refit"]]
    assert [float(v) for v in r[12:16]] == py["plane"].tolist() and float(r[17]) == py["rmse"]  # %.17g round-trips a double
    (k,) = [r for r in rows if r[0] == "KEEP"]
    assert int(k[2]) == py["inliers"] and int(k[2]) + int(k[4]) == len(pts) and k[6] == "1" and k[8] == "1", k
    many = sga.segment_planes(cloud, 6, 0.05, 300, seed=7, min_inliers=200)
    (m,) = [r for r in rows if r[0] == "PLANES"]
    count = int(m[2])
    assert count == len(many["planes"]) >= 3 and [int(v) for v in m[4:4 + count]] == [q["inliers"] for q in many["planes"]]
    assert int(m[5 + count]) == len(many["rest_indices"]) and m[7 + count] == "1", m
    assert [r for r in rows if r[0] == "REFUSE"] == [["REFUSE", "equal", "1"]]


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_the_ground_of_a_street_scan_and_the_objects_on_it():
    """odometry.run_synthetic_ground(2): the device's plane is the restatement's, the ground it removes is the generator's (z = -1.8 m in
    the sensor frame, 0.03 m one noise sigma of margin around the threshold), and what is left falls into objects."""
    threshold = 0.1
    frames = odometry.run_synthetic_ground(2)
    assert [fr["frame"] for fr in frames] == [0, 1]
    for fr in frames:
        pts, _ = synthetic.kitti_like_scan(fr["frame"])
        pts = np.ascontiguousarray(pts[:, :3], dtype=F32)
        w = ref.segment_plane(pts, threshold, 256, 0, (0.0, 0.0, 1.0), float(np.radians(15.0)))
        assert int(w["band"].sum()) == 0 and not w["shaky"].any() and w["final_band"] == 0 and not w["refit_shaky"]
        assert (fr["best_hypothesis"], fr["hypothesis_inliers"], fr["scored"], fr["inliers"], fr["refit"]) == (w["best_hypothesis"], w["hypothesis_inliers"], w["scored"], w["inliers"], w["refit"])
        assert np.array_equal(fr["kept"], np.flatnonzero(~w["inlier_mask"]))
        angle, offset = ref.plane_error(fr["plane"], w["plane"], w["anchor"])
        assert angle < 1e-10 and offset < 1e-9 and abs(fr["rmse"] - w["rmse"]) <= 1e-12 * w["rmse"]
        # against the generator
        height = pts[:, 2].astype(np.float64) + 1.8
        in_plane = np.ones(len(pts), bool)
        in_plane[fr["kept"]] = False
        tilt = float(np.arccos(min(1.0, fr["plane"][2])))
        print("frame %d: %d points, best of 256 hypotheses %d with %d inliers, refit plane %s (%.2e rad from z, d %.4f), ground %d (%.1f %%), rmse %.4f; rest %d -> %d at 0.25 m, %d objects, largest %.1f %%" % (
            fr["frame"], len(pts), fr["best_hypothesis"], fr["hypothesis_inliers"], np.array2string(fr["plane"], precision=5), tilt, fr["plane"][3], fr["ground"], 100.0 * fr["ground_share"], fr["rmse"],
            fr["rest"].size(), fr["rest_points"], fr["objects"], 100.0 * fr["largest_share"]))
        assert in_plane[np.abs(height) <= threshold - 0.03].all()
        assert not in_plane[np.abs(height) > threshold + 0.03].any()
        assert tilt < np.radians(1.0) and abs(fr["plane"][3] - 1.8) < 0.02
        assert fr["objects"] > 1 and fr["largest_share"] < 0.5

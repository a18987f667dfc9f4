"""Every route of the linearization (csrc/linearize.hip: enum class Route, plan_pass) against a float64 sum over its own pairs.

A pass takes one of seven routes, each a different kernel or pair of kernels that computes H, b, e and the inlier count; within a route
the points per lane, the fused row-sum tail, the one- or multi-workgroup row reduction and the grid-stride loop of the factor kernels
vary with the size.  Every case below reaches one plan on purpose, asserts with Problem.last_plan() that it did, and then checks:

  1. the sums over exactly the GPU's pairs (pb.factors()) against tests/factor_ref.py (float64, pinned to the oracle on the CPU);
  2. the inlier count, exactly: the GPU's pairs the reference's rejector accepts (rejector.hpp: reject iff sq_dist > max_dist_sq);
  3. H exactly symmetric;
  4. the pairs themselves against scipy's cKDTree in float64 (fp32 target, fp64-transformed queries): at the minimum distance in fp64
     arithmetic (ties aside), within a derived fp32 rounding bound of it in fp32 arithmetic; a point without a pair has nothing within
     the rejector's reach;
  5. the error at the linearization pose and at a trial pose, from the quadratic error model and from error_kernel.

The rejector is wide (1 m on a scene with ~0.5 m spacing): nearly every point is an inlier, so a dropped or doubled point changes the count
or leaves a point without a pair that has a neighbour.
"""
import os
import re

import numpy as np
import pytest

import factor_ref as fr
import small_gicp_amd as sga
from conftest import ROOT

gpu = pytest.mark.gpu  # every test here but the last (a CPU check of the matrix's coverage)

SPACING_REF = 0.5486  # linearize.hip SGA_SPACING_REF: plan_pass scales its motion thresholds by the target's spacing / this
MAXD = 1.0
MAX_SQ = MAXD * MAXD
# fp64 arithmetic: H relative to max|H|, b on the bscale of test_gpu_parity.py's C1 test (|J^T M| ~ sqrt(H_ii e)), e and the error passes
# relative to e.  Observed on the MI355X (printed with -s): at most 1.6e-14 (H), 3.3e-14 (b), 1.2e-15 (e), 1.5e-14 (error passes) from
# 8 192 points on, and 1e-13 / 2e-12 (b / error) at one point, whose e is the square of a 3 cm residual.
FP64_REL = 1e-10
# fp32 arithmetic, same scales.  Observed on the MI355X from 63 points on: at most 2.6e-7 (H, GICP + Cauchy at 65 points), 9.0e-6 (b),
# 1.3e-6 (e) and 6.0e-6 (error passes); the bounds are about 4x those.  Below ~10 000 points the rounding of the fp32 query dominates b,
# e and the error passes (a 3 cm residual of a point 21 m from the origin: 2 eps32 |q| / |r| = 9e-5 relative for one point): there the
# bound is 4x its root-sum-square estimate, rounding_scale() (observed at one point: 1.7e-4 (e) against an estimate of 6e-4).
FP32_H, FP32_B, FP32_E, FP32_ERR = 1e-6, 4e-5, 5e-6, 2.5e-5
EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
KINDS = {"ICP": fr.ICP, "PLANE_ICP": fr.PLANE_ICP, "GICP": fr.GICP}
ROBUST = {None: fr.ROBUST_NONE, "HUBER": fr.ROBUST_HUBER, "CAUCHY": fr.ROBUST_CAUCHY}
C = 0.7
ROUTES = sga.Problem.ROUTES


# ---- the plan each case means to reach (plan_pass restated for these cases) ---------------------------------------------------------
def expected_plan(route, n, fp64, warm=False, grid=False, chunk=0):
    pts = 4 if n >= (131072 if fp64 else 750000) and route != "certify" else 1
    tiles = max(1, -(-n // (256 * pts)))
    blocks = min(tiles, 2048)
    tail = route not in ("fused_lane", "fused_queue") and n > 0 and blocks <= 32
    rows = blocks
    if route == "fused_lane":
        rows = -(-n // 64)
    elif route == "fused_queue":
        rows = -(-(-(-n // 64)) // chunk)
    groups = min(64, max(8, rows // 128)) if rows > 256 else 1
    return {"route": route, "warm": warm, "grid": grid, "pts": pts, "tail": tail, "chunk_tiles": chunk, "reduce_rows": 0 if tail else rows, "reduce_groups": 0 if tail else groups}


def warm_chunk(n, chunk):
    """plan_pass: a warm queue-fed pass caps the tiles per wave so that small clouds keep ~4 waves per SIMD"""
    return min(chunk, max(1, (-(-n // 64) + 4095) // 4096))


# ---- data ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def restore_modes():
    lim = sga.get_warm_limit()
    yield
    sga.set_warm_limit(lim)
    sga.set_grid_mode(1, 65536)
    sga.set_search_mode(2, 4, 4)
    sga.set_error_model(True)


class Scene:
    pass


@pytest.fixture(scope="module")
def scene():
    from scipy.spatial import cKDTree

    target, source, T_gt = sga.synthetic.registration_pair(1_000_000)
    s = Scene()
    sga.set_grid_mode(1, 65536)
    s.tgt = sga.PointCloud(target)
    sga.estimate_normals_covariances(s.tgt, None, 10)
    s.tree = sga.KdTree(s.tgt)
    s.tp = s.tgt.xyz().astype(np.float64)
    s.tn = s.tgt.normals()[:, :3]
    s.tc = s.tgt.covs()
    s.source = source
    s.T = T_gt
    s.kd = cKDTree(s.tp)
    s.src = {}
    s.nn = {}
    return s


def source(s, n):
    """the first n source points with covariances (k = 10), and their fp32 values and covariances as the device holds them"""
    if n not in s.src:
        c = sga.PointCloud(s.source[:n])
        sga.estimate_covariances(c, None, 10)
        s.src[n] = (c, c.xyz().astype(np.float64), c.covs())
    return s.src[n]


def nearest(s, T, n):
    """float64 nearest neighbours (two, for the tie rule) of the first n source points at pose T, one query per pose, reused"""
    key = np.asarray(T).tobytes()
    if key not in s.nn or len(s.nn[key][0]) < n:
        q = fr.transform(T, s.source[: max(n, 1)].astype(np.float64))
        _, idx = s.kd.query(q, k=2, workers=16)
        d2 = ((s.tp[idx] - q[:, None, :]) ** 2).sum(2)
        s.nn[key] = (q, idx, d2)
    q, idx, d2 = s.nn[key]
    return q[:n], idx[:n], d2[:n]


def unit(s):
    sp = s.tree.spacing()
    if sp == 0:  # the build hands the spacing over as a late note: a result of the target collects it
        sga.Problem(s.tree, source(s, 1)[0]).linearize(sga.make_setting("ICP").factor, s.T)
        sp = s.tree.spacing()
    assert sp > 0
    return sp / SPACING_REF


def step(T, d):
    """T followed by a pure translation of length d (a translation moves every source point by exactly d)"""
    S = T.copy()
    S[:3, 3] += np.array([0.6, -0.48, 0.64]) * d
    return S


def trial(T):
    S = np.eye(4)
    a = 1e-3
    S[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    S[:3, 3] = [2e-3, -1e-3, 1.5e-3]
    return T @ S


def rounding_scale(src_pts, tgt_pts, tgt_nrm, corr, T, kind, robust, maha):
    """Root-sum-square estimate of what rounding the fp32 query q = T p (2 eps32 |q| per point) does to b (per entry) and to e"""
    si = np.flatnonzero(corr >= 0)
    ti = corr[si]
    q = fr.transform(T, np.asarray(src_pts)[si])
    r = np.asarray(tgt_pts, dtype=np.float64)[ti] - q
    M = maha[si] if kind == fr.GICP else fr.mahalanobis(kind, T, None, None, tgt_nrm, si, ti)
    Mr = np.einsum("nij,nj->ni", M, r)
    w = fr.robust_weight(robust, C, 0.5 * np.einsum("ni,ni->n", r, Mr))
    dq = 2 * EPS32 * np.linalg.norm(q, axis=1)
    Mn = np.linalg.norm(M, axis=(1, 2))
    de = np.sqrt(((w * np.linalg.norm(Mr, axis=1) * dq) ** 2).sum())
    lever = np.concatenate([np.repeat(np.linalg.norm(np.asarray(src_pts)[si], axis=1)[:, None], 3, 1), np.ones((len(si), 3))], 1)
    db = np.sqrt((((w * Mn * dq)[:, None] * lever) ** 2).sum(0))
    return db, de


# ---- the checks every pass makes ----------------------------------------------------------------------------------------------------
def check_pass(label, pb, setting, T, res, tgt_pts, tgt_nrm, tgt_cov, src_pts, src_cov, fp64, kind, robust, nn=None, max_sq=MAX_SQ):
    H, b, e, n = res
    corr, _ = pb.factors()
    kind_i, rob_i = KINDS[kind], ROBUST[robust]
    ref = fr.linearize(src_pts, tgt_pts, corr, T, kind_i, rob_i, C, src_cov, tgt_cov, tgt_nrm)
    if fp64:
        tH = tB = tE = tErr = FP64_REL
    else:
        db, de = rounding_scale(src_pts, tgt_pts, tgt_nrm, corr, T, kind_i, rob_i, ref.maha)
        tH = FP32_H
        tB = max(FP32_B, 4 * (db / (np.sqrt(np.abs(np.diag(ref.H)) * max(ref.e, 1e-30)) + 1e-30)).max())
        tE = max(FP32_E, 4 * de / max(abs(ref.e), 1e-300))
        tErr = max(FP32_ERR, tE)
    # 3. symmetry
    assert np.array_equal(H, H.T), label
    # 1. sums over the GPU's own pairs
    scale = max(np.abs(ref.H).max(), 1e-300)
    bscale = np.sqrt(np.abs(np.diag(ref.H)) * max(ref.e, 1e-30)) + 1e-30
    rH = np.abs(H - ref.H).max() / scale
    rb = (np.abs(b - ref.b) / bscale).max()
    re_ = abs(e - ref.e) / max(abs(ref.e), 1e-300)
    # 2. inlier count: every pair the GPU kept is one the reference keeps (fp32: a pair within 1e-6 of the threshold counts either way)
    d2 = fr.sq_dist(src_pts, tgt_pts, corr, T)
    paired = corr >= 0
    if fp64:
        assert n == int((d2[paired] <= max_sq).sum()) == int(paired.sum()), (label, n, int(paired.sum()), int((d2[paired] <= max_sq).sum()))
    else:
        lo, hi = int((d2[paired] <= max_sq * (1 - 1e-6)).sum()), int((d2[paired] <= max_sq * (1 + 1e-6)).sum())
        assert n == int(paired.sum()) and lo <= n <= hi, (label, n, int(paired.sum()), lo, hi)
    # 4. the pairs: nearest in float64 (fp64), or within the fp32 rounding of the nearest
    if nn is not None:
        q, idx, dk = nn
        dmin = np.sqrt(dk.min(1))
        p_abs = np.linalg.norm(src_pts, axis=1) + np.linalg.norm(q, axis=1) + np.abs(T[:3, 3]).sum()
        # fp32: the query is rounded (transform in fp32: a few ulps of the coordinates), the distances compared in fp32
        delta = (8 * EPS64 if fp64 else 8 * EPS32) * p_abs
        slack = 2.5 * delta + (4 * EPS64 if fp64 else 4 * EPS32) * dmin
        dg = np.sqrt(d2)
        bad = paired & ~(dg <= dmin + slack)
        assert not bad.any(), (label, int(bad.sum()), np.flatnonzero(bad)[:5], dg[bad][:5], dmin[bad][:5])
        reach = np.sqrt(max_sq) if max_sq > 0 else np.inf
        lost = ~paired & (dmin < reach * (1 - (1e-12 if fp64 else 1e-6)) - slack)
        assert not lost.any(), (label, int(lost.sum()), np.flatnonzero(lost)[:5], dmin[lost][:5])
    assert rH <= tH and rb <= tB and re_ <= tE, (label, rH, rb, re_, (tH, tB, tE))
    # 5. error passes: the quadratic model and error_kernel, at the linearization pose and at a trial pose
    errs = []
    for Tq in (T, trial(T)):
        er = fr.error(src_pts, tgt_pts, corr, Tq, kind_i, rob_i, C, ref.maha, tgt_nrm)
        for model in (True, False):
            sga.set_error_model(model)
            eg = pb.error(setting.factor, Tq)
            errs.append(abs(eg - er) / max(abs(er), 1e-300))
        sga.set_error_model(True)
    assert max(errs) <= tErr, (label, errs, tErr)
    print("%-46s n=%7d inliers=%7d  H %.1e  b %.1e  e %.1e  err %.1e  (bounds %.0e %.0e %.0e %.0e)" % (label, len(corr), n, rH, rb, re_, max(errs), tH, tB, tE, tErr))


def run_case(s, label, n, kind, robust, fp64, poses, plans, setup=None, pair_check=True):
    """linearize the first n source points along `poses`; the pass at poses[k] must follow plans[k] (None: not checked)"""
    cloud, sp, sc = source(s, n)
    st = sga.make_setting(kind, robust_kernel=robust, robust_c=C, math_mode="fp64" if fp64 else "fp32", max_correspondence_distance=MAXD)
    pb = sga.Problem(s.tree, cloud)
    if setup:
        setup(pb)
    for k, T in enumerate(poses):
        res = pb.linearize(st.factor, T)
        plan = pb.last_plan()
        want = plans[k]
        if want is not None:
            assert plan == want, (label, k, plan, want)
            check_pass("%s pass %d" % (label, k), pb, st, T, res, s.tp, s.tn, s.tc, sp, sc, fp64, kind, robust, nearest(s, T, n) if pair_check else None)
    return pb


# ---- the matrix ---------------------------------------------------------------------------------------------------------------------
FUSED_LANE_N = [1, 63, 65, 16_384, 16_385, 524_325]
FACTORS5 = [("ICP", None), ("PLANE_ICP", None), ("GICP", None), ("GICP", "HUBER"), ("GICP", "CAUCHY")]


@gpu
@pytest.mark.parametrize("kind,robust", FACTORS5)
@pytest.mark.parametrize("n", FUSED_LANE_N)
def test_fused_lane_cold(scene, n, kind, robust):
    s = scene
    plan = expected_plan("fused_lane", n, False, grid=True)
    run_case(s, "fused_lane cold %s/%s" % (kind, robust), n, kind, robust, False, [s.T], [plan])


@gpu
def test_fused_lane_warm_lpt(scene):
    """524 325 points: 8 193 search tiles, so the cold pass records the tiles' durations and the warm pass starts them longest first"""
    s = scene
    n = 524_325
    source(s, n)
    u = unit(s)
    run_case(s, "fused_lane warm", n, "GICP", None, False, [s.T, step(s.T, 0.05 * u)],
             [expected_plan("fused_lane", n, False, grid=True), expected_plan("fused_lane", n, False, warm=True, grid=True)])


@gpu
@pytest.mark.parametrize("chunk", [1, 4, 16])
@pytest.mark.parametrize("n", [65, 16_385, 300_037])
def test_fused_queue(scene, n, chunk):
    s = scene
    u = unit(s)
    sga.set_search_mode(2, 4, chunk)
    d = 0.01 * u  # <= 0.02 unit: queue-fed; > 0.002 unit: not the certify route (which 300 037 points would take)
    kinds = FACTORS5 if n != 300_037 or chunk == 4 else [("GICP", None)]
    for kind, robust in kinds:
        c = warm_chunk(n, chunk)
        run_case(s, "fused_queue chunk %d %s/%s" % (chunk, kind, robust), n, kind, robust, False, [s.T, step(s.T, d)],
                 [None, expected_plan("fused_queue", n, False, warm=True, grid=True, chunk=c)])


@gpu
@pytest.mark.parametrize("grid_mode", [1, 0])
@pytest.mark.parametrize("n", [262_144, 524_325])
def test_certify(scene, n, grid_mode):
    s = scene
    u = unit(s)
    sga.set_grid_mode(grid_mode)
    for kind, robust in [("ICP", None), ("GICP", None), ("GICP", "HUBER")]:
        T1, T2 = step(s.T, 0.0015 * u), step(s.T, 0.0025 * u)  # each step moves by at most 0.0015 unit
        run_case(s, "certify grid %d %s/%s" % (grid_mode, kind, robust), n, kind, robust, False, [s.T, T1, T2],
                 [None, expected_plan("certify", n, False, warm=True, grid=grid_mode != 0), expected_plan("certify", n, False, warm=True, grid=grid_mode != 0)])


@gpu
@pytest.mark.parametrize("kind", ["ICP", "GICP"])
@pytest.mark.parametrize("n", [8_193, 131_109, 524_325, 750_037])
def test_queue(scene, n, kind):
    """fp32: the queue-fed search always (set_search_mode(1)), cold; fp64: a warm pass after a small step (fp64 never fuses)"""
    s = scene
    u = unit(s)
    sga.set_search_mode(1, 4, 4)
    run_case(s, "queue fp32 cold %s" % kind, n, kind, None, False, [s.T], [expected_plan("queue", n, False, grid=True, chunk=4)])
    if n == 524_325:
        return
    sga.set_search_mode(2, 4, 4)
    c = warm_chunk(n, 4)
    run_case(s, "queue fp64 warm %s" % kind, n, kind, None, True, [s.T, step(s.T, 0.01 * u)],
             [expected_plan("lane", n, True, grid=True), expected_plan("queue", n, True, warm=True, grid=True, chunk=c)])


@gpu
@pytest.mark.parametrize("kind,robust", [("ICP", None), ("PLANE_ICP", None), ("GICP", None), ("ICP", "HUBER")])
@pytest.mark.parametrize("n", [1, 8_192, 8_193, 131_071, 131_109])
def test_lane(scene, n, kind, robust):
    """fp64 cold passes; fp32 with a host rejector (which the fused kernels do not serve)"""
    s = scene
    run_case(s, "lane fp64 %s/%s" % (kind, robust), n, kind, robust, True, [s.T], [expected_plan("lane", n, True, grid=True)])
    if n in (1, 8_193, 131_109):
        def host(pb):
            pb.set_rejector(lambda T, idx, d2: (idx < 0) | (d2 > MAX_SQ))

        run_case(s, "lane fp32 host rejector %s/%s" % (kind, robust), n, kind, robust, False, [s.T], [expected_plan("lane", n, False, grid=False)], setup=host)


@gpu
@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("kind", ["ICP", "GICP"])
@pytest.mark.parametrize("n", [8_193, 750_037])
def test_grid(scene, n, kind, fp64):
    s = scene
    sga.set_grid_mode(4)
    run_case(s, "grid %s %s" % ("fp64" if fp64 else "fp32", kind), n, kind, None, fp64, [s.T], [expected_plan("grid", n, fp64, grid=True)])


def _slot_rows(idx, counts):
    """flat map: (voxel << 32) | point -> row of the voxel-major point list of download(); -1 stays -1"""
    offs = np.concatenate([[0], np.cumsum(counts.astype(np.int64))[:-1]])
    out = np.full(len(idx), -1, np.int64)
    ok = idx >= 0
    out[ok] = offs[idx[ok] >> 32] + (idx[ok] & 0xFFFFFFFF)
    return out


@pytest.fixture(scope="module")
def maps(scene):
    s = scene
    out = {}
    vm = sga.GaussianVoxelMap(1.0)
    vm.insert(s.tgt)
    _, means, c6, _ = vm.download()
    cov = np.zeros((len(c6), 3, 3))
    cov[:] = sga.api.mats_from_sym6(c6.astype(np.float64))
    out["GICP"] = (vm, means.astype(np.float64), None, cov, lambda idx: idx)
    fm = sga.IncrementalVoxelMap(0.5)
    fm.insert(s.tgt)
    _, counts, pts = fm.download()
    out["ICP"] = (fm, pts.astype(np.float64), None, None, lambda idx, c=counts: _slot_rows(idx, c))
    nm = sga.IncrementalVoxelMapNormal(0.5)
    nm.insert(s.tgt)
    _, ncounts, npts, nrm = nm.download()
    out["PLANE_ICP"] = (nm, npts.astype(np.float64), nrm.astype(np.float64), None, lambda idx, c=ncounts: _slot_rows(idx, c))
    return out


@gpu
@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("kind", ["GICP", "ICP", "PLANE_ICP"])
@pytest.mark.parametrize("n", [8_193, 131_109, 750_037])
def test_factors_voxel_maps(scene, maps, n, kind, fp64):
    """a Gaussian voxel map (GICP) and flat maps (ICP; PLANE_ICP over the map that keeps normals): the search is inside the factor kernel,
    over the map's voxels (not a global nearest neighbour), so only the sums, the count, symmetry and the error passes are checked"""
    s = scene
    m, tp, tn, tc, rows = maps[kind]
    cloud, sp, sc = source(s, n)
    st = sga.make_setting(kind, math_mode="fp64" if fp64 else "fp32", max_correspondence_distance=MAXD)
    pb = sga.Problem(m, cloud)
    res = pb.linearize(st.factor, s.T)
    assert pb.last_plan() == expected_plan("factors", n, fp64), (pb.last_plan(), expected_plan("factors", n, fp64))

    class Mapped:  # pb.factors() in the map's row numbering
        def factors(self):
            c, mm = pb.factors()
            return rows(c), mm

        def error(self, f, T):
            return pb.error(f, T)

    check_pass("factors %s %s" % ("fp64" if fp64 else "fp32", kind), Mapped(), st, s.T, res, tp, tn, tc, sp, sc, fp64, kind, None)


def test_route_enum_is_covered():
    """(CPU) every enumerator of enum class Route has a case in this matrix: a new route cannot arrive without one"""
    src = open(os.path.join(ROOT, "small_gicp_amd", "csrc", "linearize.hip")).read()
    body = re.search(r"enum class Route \{(.*?)\};", src, re.S).group(1)
    names = re.findall(r"^\s*k(\w+),", body, re.M)
    snake = [re.sub(r"(?<!^)([A-Z])", r"_\1", nm).lower() for nm in names]
    assert tuple(snake) == ROUTES, (snake, ROUTES)  # Problem.ROUTES names the enum values in order
    here = open(__file__).read()
    missing = [r for r in snake if 'expected_plan("%s"' % r not in here]
    assert not missing, missing



# ---- the fp64 rejector threshold ----------------------------------------------------------------------------------------------------
def edge_pairs(max_sq=0.01):
    """Source points whose squared distance to their target point lies on both sides of the DOUBLE max_sq, within float rounding of it
    (float(0.01) = 0.0099999998): (target (m, 3), source (m, 3), d2 (m,)) as float32 points and the float64 d2 the reference computes.
    Target point k sits at (0, 0, k); its source point at (x, y, k), x near 0.1 and y small, so that d2 = x^2 + y^2 is exact in float64
    and can be placed to ~1e-15."""
    offsets = [-5e-10, -2e-10, -1e-10, -1e-12, 1e-12, 1e-10, 3e-10]
    tgt, src, d2 = [], [], []
    for k, off in enumerate(offsets * 3):
        D = max_sq + off
        x = np.float32(np.sqrt(D - 5e-9))
        while float(x) ** 2 > D - 1e-9:
            x = np.nextafter(x, np.float32(0))
        y = np.float32(np.sqrt(D - float(x) ** 2))
        for _ in range(64):  # nearest float y
            best = min((y, np.nextafter(y, np.float32(1)), np.nextafter(y, np.float32(0))), key=lambda v: abs(float(x) ** 2 + float(v) ** 2 - D))
            if best == y:
                break
            y = best
        z = np.float32(k)
        tgt.append([0.0, 0.0, z])
        src.append([x, y, z])
        d = float(x) ** 2 + float(y) ** 2
        assert (d <= max_sq) == (off < 0) and abs(d - max_sq) > 1e-14, (off, d)
        d2.append(d)
    return np.array(tgt, np.float32), np.array(src, np.float32), np.array(d2)


@gpu
def test_fp64_rejector_threshold_is_double():
    """fp64 arithmetic classifies a pair as the reference does (rejector.hpp:24, sq_dist > max_dist_sq in double) on every route fp64 can
    reach — lane (cold), queue (warm), grid, and the factor kernel over a flat map — and KdTree.batch_knn_search(max_sq_dist) does too;
    fp32 arithmetic keeps its fp32 semantics (the float distance against float(max_dist_sq); a pair within 1e-6 of it goes either way)."""
    tp, spts, d2 = edge_pairs()
    inl_ref = d2 <= 0.01
    assert inl_ref.sum() == 12 and (~inl_ref).sum() == 9
    sga.set_grid_mode(4, 16)  # the grid is built with the index: before the tree
    tree = sga.KdTree(sga.PointCloud(tp))
    src = sga.PointCloud(spts)
    st64 = sga.make_setting("ICP", math_mode="fp64", max_correspondence_distance=0.1)
    st32 = sga.make_setting("ICP", math_mode="fp32", max_correspondence_distance=0.1)
    T = np.eye(4)

    def verdict(pb, st, label):
        _, _, _, n = pb.linearize(st.factor, T)
        corr = pb.factors()[0]
        return label, n, corr >= 0, pb.last_plan()["route"]

    got = []
    sga.set_grid_mode(1)
    pb = sga.Problem(tree, src)
    got.append(verdict(pb, st64, "lane") + ("lane",))
    got.append(verdict(pb, st64, "queue warm") + ("queue",))  # no motion since the last pass: warm, queue-fed
    sga.set_grid_mode(4)
    got.append(verdict(sga.Problem(tree, src), st64, "grid") + ("grid",))
    fm = sga.IncrementalVoxelMap(1.0)
    fm.insert(sga.PointCloud(tp))
    got.append(verdict(sga.Problem(fm, src), st64, "flat map") + ("factors",))
    for label, n, ok, route, want in got:
        assert route == want, (label, route)
        assert n == inl_ref.sum() and (ok == inl_ref).all(), (label, n, np.flatnonzero(ok != inl_ref), d2[ok != inl_ref] - 0.01)
    # the kNN of the reference's signature: double queries, double distances, the double threshold
    idx, dk = tree.batch_knn_search(spts.astype(np.float64), 1, max_sq_dist=0.01)
    found = idx[:, 0] >= 0
    assert (found == inl_ref).all(), (np.flatnonzero(found != inl_ref), d2[found != inl_ref] - 0.01)
    assert np.abs(dk[found, 0] - d2[found]).max() <= 1e-17
    # fp32: the float distance against float(0.01); outside the 1e-6 band the verdict is fixed
    sga.set_grid_mode(1)
    _, n32, ok32, _ = verdict(sga.Problem(tree, src), st32, "fp32")
    clear = np.abs(d2 - 0.01) > 1e-6 * 0.01
    assert (ok32[clear] == inl_ref[clear]).all() and n32 == ok32.sum()
    # a posed case: T s is no longer exact in fp32, so the walks measure from a query up to 2^-24 |q| per axis away from the double one
    # the factor kernel tests (40 m: ~1e-6 m, 5e-5 of d2 at d = 0.1 m — far beyond the fp32 nudge).  The routes re-decide the pair in
    # double; the per-point export (sga_linearize_per_point) reports the pairs of its own fp64 pass.
    Tp, tp2, sp2, d2p = posed_edge_pairs()
    inl_p = d2p <= 0.01
    assert 0 < inl_p.sum() < len(d2p)
    sga.set_grid_mode(4, 16)
    tree_p = sga.KdTree(sga.PointCloud(tp2))
    src_p = sga.PointCloud(sp2)
    got = []
    sga.set_grid_mode(1)
    pb = sga.Problem(tree_p, src_p)
    _, _, _, n = pb.linearize(st64.factor, Tp)
    got.append(("posed lane", n, pb.factors()[0] >= 0, pb.last_plan()["route"], "lane"))
    _, _, _, n = pb.linearize(st64.factor, Tp)
    got.append(("posed queue warm", n, pb.factors()[0] >= 0, pb.last_plan()["route"], "queue"))
    sga.set_grid_mode(4)
    pb = sga.Problem(tree_p, src_p)
    _, _, _, n = pb.linearize(st64.factor, Tp)
    got.append(("posed grid", n, pb.factors()[0] >= 0, pb.last_plan()["route"], "grid"))
    sga.set_grid_mode(1)
    for label, n, ok, route, want in got:
        assert route == want, (label, route)
        assert n == inl_p.sum() and (ok == inl_p).all(), (label, n, inl_p.sum(), np.flatnonzero(ok != inl_p)[:8], (d2p[ok != inl_p] / 0.01 - 1)[:8])
    okp = sga.Problem(tree_p, src_p).linearize_per_point(st64.factor, Tp)[0]
    assert (okp == inl_p).all(), ("posed per-point export", okp.sum(), inl_p.sum(), np.flatnonzero(okp != inl_p)[:8], (d2p[okp != inl_p] / 0.01 - 1)[:8])


def posed_edge_pairs(max_sq=0.01, seed=7):
    """(T, target (m, 3) float32, source (m, 3) float32, d2 (m,)): source points whose transformed positions q = T s (in double, as fp64
    passes form them) lie 20 - 45 m from the origin, each with one target point at d2 = (1 + delta) max_sq, |delta| <= 3e-5, from q; the
    pairs sit on a 1 m lattice, so each q's nearest target is its own.  d2 is the float64 distance the reference's rejector compares."""
    rng = np.random.default_rng(seed)
    a = np.deg2rad(20.0)
    k = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = [0.3, -0.2, 0.5]
    g = np.stack(np.meshgrid(np.arange(6), np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 3) + [20.0, -30.0, 5.0]
    Ti = np.linalg.inv(T)
    s = (g @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    q = s.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    u = rng.normal(size=q.shape)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    t = (q + u * np.sqrt(max_sq * (1 + rng.uniform(-3e-5, 3e-5, len(q))))[:, None]).astype(np.float32)
    d2 = ((t.astype(np.float64) - q) ** 2).sum(1)
    assert np.abs(d2 - max_sq).min() > 1e-12  # clear of the few-ulp differences of the device's double transform
    return T, t, s, d2

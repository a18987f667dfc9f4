"""The per-pair outputs of a linearization pass against float64 restatements (tests/factor_ref.py: per_pair, mahalanobis).

test_route_matrix.py, test_batch_gpu.py, test_batch_maps_gpu.py and test_projective_gpu.py check the SUMS of a pass on every route.  A
pass leaves three more outputs that callers read and the hot loop never does:

  (a) the cached Mahalanobis matrices (sga_problem_get_factors, factors()[1], factors_torch) on every route, after fp32 and fp64 passes;
  (b) the state machine behind them (maha_valid, last_math, lin_factor, lin_T, maha / maha64) along nine sequences of calls;
  (c) the per-point export (sga_linearize_per_point) per pair: kd-trees, flat maps, a host rejector, pairs that tie in fp32;
  (d) the enqueue-only forms sga_linearize_async / sga_error_async, plain and framed, and the refusal of a mixed arithmetic.

Every case asserts with last_plan() which route ran.  The scene is small (20 000 points, sources of 1 - 4 097 points; one certify case
at its minimum size of 262 144), the rejector reaches 1 m (MAXD of the route matrix) and robust_c = 0.7.

A framed problem (both clouds ~1 000 km from the origin) is restated in its DEVICE frames — records = xyz64() - origin(), the pose of
frames.hip's pose_to_device restated operation by operation — and the per-pair systems are carried to the caller's twist convention with
the adjoint A of the source origin (H = A^T H' A, b = A^T b', magnitudes with |A|): a restatement in the caller's coordinates would
itself lose 2e-10 m of every residual at 2e6 m, a hundred times FP64_REL.

The Mahalanobis bound, per pair:  |m6 - M_ref| <= 0.5 spacing32(M_ref) + MAHA_C eps cond2(A) max|M_ref|,  A = C_t + R C_s R^T,
M_ref = inv(A) in float64 from the fp32 covariances the device holds, eps = 2^-24 after an fp32 pass and 2^-53 after an fp64 pass (the
export is fp32 either way: the first term).  Measured on the MI355X (printed with -s by test_zz_report) over all cases: worst
(err - 0.5 spacing32) / (eps cond2 max|M|) = MAHA_WORST = 2.163 after an fp32 pass (the certify case; 1.08 - 1.24 on the other routes at
4 097 points) and 0 after an fp64 pass (its error disappears in the fp32 export); MAHA_C = 16 is 4x that, rounded up to a power of two.
The largest cond2(A) of these scenes is 1.0e3 (plane-regularised covariances).

Other residuals of that run, against their bounds: per-point export H 6.2e-13, b 9.4e-14, e 1.3e-14 of the pair's magnitudes and its column
sums 1.3e-14 on check_pass's scales (bound FP64_REL = 1e-10 each); linearize_async at most 0.12 of the fp32 pass bounds and 3.4e-4 of
FP64_REL in fp64, plain and framed; error_async 0.094 of the fp32 bound, 1.6e-5 of FP64_REL in fp64.  Before the export formed its residual
as hi + lo (linearize.hip: exact_residual), b_i of PLANE_ICP missed FP64_REL at 4 097 points (7.9e-10 of |J|^T |M| |r|): a source point
1e-5 m off its target's plane, where the rounding of q = R p + t 50 m from the origin (1e-14 m) is 1e-9 of n . r.
"""
import numpy as np
import pytest
import torch

import factor_ref as fr
import small_gicp_amd as sga
import test_route_matrix as rm
from test_route_matrix import FP64_REL, KINDS, ROBUST, check_pass, expected_plan, step, trial

pytestmark = pytest.mark.gpu

MAHA_WORST = 2.163  # measured on the MI355X (see above)
MAHA_C = 16.0  # 4 x MAHA_WORST, rounded up to a power of two
EPS32, EPS64 = rm.EPS32, rm.EPS64
MAXD, C = rm.MAXD, rm.C
SHIFT = np.array([1_000_064.0, -2_000_000.0, 128.0])  # test_batch_gpu.SHIFT: multiples of 128 m, about 1 000 km
SIZES = [1, 63, 64, 65, 257, 4097]
FACTORS5 = rm.FACTORS5
SENT = -7.25  # guard value behind the payload of a device buffer
WORST = {}  # label -> the worst residual / bound seen (test_zz_report prints them)


def note(key, value):
    WORST[key] = max(WORST.get(key, 0.0), float(value))


@pytest.fixture(autouse=True)
def restore_modes():
    lim = sga.get_warm_limit()
    yield
    sga.set_warm_limit(lim)
    sga.set_grid_mode(1, 65536)
    sga.set_search_mode(2, 4, 4)
    sga.set_error_model(True)


# ---- data ---------------------------------------------------------------------------------------------------------------------------
class Cloud:
    """a device cloud with what the restatements read: caller coordinates (float64), the records of its device frame, normals, covariances"""

    def __init__(self, points, normals):
        self.cloud = sga.PointCloud(points)
        if normals:
            sga.estimate_normals_covariances(self.cloud, None, 10)
        else:
            sga.estimate_covariances(self.cloud, None, 10)
        self.origin = np.asarray(self.cloud.origin(), dtype=np.float64)
        self.p = self.cloud.xyz64()
        self.rec = self.p - self.origin  # exact: fp32 records, an origin of multiples of 128 m
        self.n = self.cloud.normals()[:, :3] if normals else None
        self.c = self.cloud.covs()


def pose_to_device(T, o_s, o_t):
    """frames.hip pose_to_device, operation by operation: t' = (R o_s) + (t - o_t), the products added left to right"""
    R, out = T[:3, :3], T.copy()
    out[:3, 3] = ((R[:, 0] * o_s[0] + R[:, 1] * o_s[1]) + R[:, 2] * o_s[2]) + (T[:3, 3] - o_t)
    return out


def adjoint(o):
    """A with J = J' A for the source origin o (J = [R skew(p), -R], p = p' + o): H = A^T H' A, b = A^T b' (frames.hip system_to_caller)"""
    A = np.eye(6)
    A[3:, :3] = -np.array([[0, -o[2], o[1]], [o[2], 0, -o[0]], [-o[1], o[0], 0]], dtype=np.float64)
    return A


def conj(T, s):
    S, Si = np.eye(4), np.eye(4)
    S[:3, 3], Si[:3, 3] = s, -s
    return S @ T @ Si


class World:
    pass


@pytest.fixture(scope="module")
def world():
    target, source, T = sga.synthetic.registration_pair(20_000)
    w = World()
    w.T = {False: T, True: conj(T, SHIFT)}
    sga.set_grid_mode(1, 65536)
    w.tgt = {False: Cloud(target, True), True: Cloud(target.astype(np.float64) + SHIFT, True)}
    w.tree = {f: sga.KdTree(c.cloud) for f, c in w.tgt.items()}
    assert not w.tgt[False].origin.any() and np.abs(w.tgt[True].origin).max() > 9e5 and np.array_equal(w.tgt[True].rec, w.tgt[False].rec)
    sga.set_grid_mode(4, 16)  # the grid is built with the index
    w.tgt_grid = Cloud(target, True)
    w.tree_grid = sga.KdTree(w.tgt_grid.cloud)
    sga.set_grid_mode(1, 65536)
    w.source = source
    w.src = {}
    w.maps = {}
    return w


def src_of(w, n, framed=False):
    if (n, framed) not in w.src:
        pts = w.source[:n]
        w.src[n, framed] = Cloud(pts.astype(np.float64) + SHIFT if framed else pts, False)
    return w.src[n, framed]


def unit_of(w):
    tree = w.tree[False]
    if tree.spacing() == 0:  # the build hands the spacing over as a late note: a result of the target collects it
        sga.Problem(tree, src_of(w, 1).cloud).linearize(sga.make_setting("ICP").factor, w.T[False])
    assert tree.spacing() > 0
    return tree.spacing() / rm.SPACING_REF


def maps_of(w):
    """the Gaussian map (GICP), the flat map (ICP) and the flat map with normals (PLANE_ICP) of the target: (map, rows of points, normals,
    covariances, factors() index -> row), as test_route_matrix.py's `maps`"""
    if not w.maps:
        t = w.tgt[False].cloud
        vm = sga.GaussianVoxelMap(1.0)
        vm.insert(t)
        _, means, c6, _ = vm.download()
        w.maps["GICP"] = (vm, means.astype(np.float64), None, sga.api.mats_from_sym6(c6.astype(np.float64)), lambda idx: idx)
        fm = sga.IncrementalVoxelMap(0.5)
        fm.insert(t)
        _, counts, pts = fm.download()
        w.maps["ICP"] = (fm, pts.astype(np.float64), None, None, lambda idx, c=counts: rm._slot_rows(idx, c))
        nm = sga.IncrementalVoxelMapNormal(0.5)
        nm.insert(t)
        _, ncounts, npts, nrm = nm.download()
        w.maps["PLANE_ICP"] = (nm, npts.astype(np.float64), nrm.astype(np.float64), None, lambda idx, c=ncounts: rm._slot_rows(idx, c))
    return w.maps


def setting(kind, robust=None, fp64=False, maxd=MAXD, **kw):
    return sga.make_setting(kind, robust_kernel=robust, robust_c=C, math_mode="fp64" if fp64 else "fp32", max_correspondence_distance=maxd, **kw)


def ran(pb, route, warm=None, n=None, fp64=False):
    """the last pass of pb took `route` (named as expected_plan names it), warm or cold"""
    plan = pb.last_plan()
    want = expected_plan(route, n if n is not None else pb.source.size(), fp64, warm=bool(warm), chunk=1)
    assert plan["route"] == want["route"], (plan, route)
    if warm is not None:
        assert plan["warm"] == want["warm"], (plan, warm)


# ---- (a) the Mahalanobis matrices ----------------------------------------------------------------------------------------------------
def sym6(M):
    return np.stack([M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], M[:, 1, 1], M[:, 1, 2], M[:, 2, 2]], 1)


def check_maha(label, corr, m6, T, kind, fp64, src_cov, tgt_cov):
    """m6 (n, 6) float32 of factors() against inv(C_t[corr] + R C_s R^T): corr in rows of tgt_cov, T the pose of the LAST linearization,
    kind its factor, fp64 its arithmetic.  Returns the number of pairs."""
    assert m6.dtype == np.float32 and m6.shape == (len(corr), 6), (label, m6.dtype, m6.shape)
    if KINDS[kind] != fr.GICP:
        assert not m6.any(), (label, "a factor without a mahalanobis matrix exports zeros", np.flatnonzero(m6.any(1))[:5])
        return 0
    ok = corr >= 0
    assert not m6[~ok].any(), (label, "outlier rows are zero", np.flatnonzero(m6.any(1) & ~ok)[:5])
    si = np.flatnonzero(ok)
    if len(si) == 0:
        return 0
    R = np.asarray(T, dtype=np.float64)[:3, :3]
    A = fr._cov3(tgt_cov)[corr[si]] + R @ fr._cov3(src_cov)[si] @ R.T
    M = np.linalg.inv(A)
    cond = np.linalg.cond(A)
    assert cond.max() <= 1e4, (label, "input condition", cond.max())
    ref = sym6(M)
    err = np.abs(m6[si].astype(np.float64) - ref)
    half = 0.5 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    scale = ((EPS64 if fp64 else EPS32) * cond * np.abs(M).max((1, 2)))[:, None]
    ratio = np.maximum(err - half, 0.0) / scale
    note("maha fp64" if fp64 else "maha fp32", ratio.max())
    note("maha cond2", cond.max())
    k = np.unravel_index(np.argmax(ratio), ratio.shape)
    print("%-58s pairs %6d  cond2 %.1e  maha (err - half ulp32) / (eps cond max|M|) %.3f" % (label, len(si), cond.max(), ratio.max()))
    assert (err <= half + MAHA_C * scale).all(), (label, ratio.max(), si[k[0]], k[1], m6[si[k[0]]], ref[k[0]])
    return len(si)


def kd_case(w, label, n, kind, robust, fp64, route, warm, framed=False, tree=None, tgt=None, prep=None, second=None):
    """one pass (two with `second`, the pose of the second) of the first n source points against the kd-tree; the last must take `route`;
    then (a).  Returns the problem."""
    tgt = tgt or w.tgt[framed]
    src = src_of(w, n, framed)
    st = setting(kind, robust, fp64)
    pb = sga.Problem(tree or w.tree[framed], src.cloud)
    if prep:
        prep(pb)
    T = w.T[framed]
    pb.linearize(st.factor, T)
    if second is not None:
        T = second
        pb.linearize(st.factor, T)
    ran(pb, route, warm, n, fp64)
    corr, m6 = pb.factors()
    check_maha("%s %s/%s n=%d%s" % (label, kind, robust, n, " framed" if framed else ""), corr, m6, T, kind, fp64, src.c, tgt.c)
    return pb


@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("kind,robust", FACTORS5)
def test_maha_fused_routes(world, kind, robust, framed):
    """fp32: fused_lane (cold), fused_queue (warm after a small step), queue (the queue-fed search always, cold)"""
    w = world
    u = unit_of(w)
    for n in SIZES:
        kd_case(w, "fused_lane cold", n, kind, robust, False, "fused_lane", False, framed)
        kd_case(w, "fused_queue warm", n, kind, robust, False, "fused_queue", True, framed, second=step(w.T[framed], 0.01 * u))
    sga.set_search_mode(1, 4, 4)
    for n in SIZES:
        kd_case(w, "queue cold", n, kind, robust, False, "queue", False, framed)


@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("kind,robust", FACTORS5)
def test_maha_lane_queue_fp64_and_host_rejector(world, kind, robust, framed):
    """fp64: lane (cold), queue (warm); fp32 with a host rejector: lane"""
    w = world
    u = unit_of(w)

    def host(pb):
        pb.set_rejector(lambda T, idx, d2: (idx < 0) | (d2 > MAXD * MAXD))

    for n in SIZES:
        kd_case(w, "lane fp64", n, kind, robust, True, "lane", False, framed)
        kd_case(w, "queue fp64 warm", n, kind, robust, True, "queue", True, framed, second=step(w.T[framed], 0.01 * u))
        kd_case(w, "lane fp32 host rejector", n, kind, robust, False, "lane", False, framed, prep=host)


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("kind,robust", FACTORS5)
def test_maha_grid(world, kind, robust, fp64):
    w = world
    sga.set_grid_mode(4)
    for n in SIZES:
        kd_case(w, "grid %s" % ("fp64" if fp64 else "fp32"), n, kind, robust, fp64, "grid", False, tree=w.tree_grid, tgt=w.tgt_grid)


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("kind,robust", [("GICP", None), ("GICP", "HUBER"), ("GICP", "CAUCHY"), ("ICP", None), ("PLANE_ICP", None)])
def test_maha_voxel_maps(world, kind, robust, fp64):
    """the factors route: a Gaussian map with GICP (its matrices from the voxels' covariances), a flat map with ICP, a flat map with
    normals with PLANE_ICP (zeros)"""
    w = world
    m, _, _, tc, rows = maps_of(w)[kind]
    for n in SIZES:
        src = src_of(w, n)
        pb = sga.Problem(m, src.cloud)
        pb.linearize(setting(kind, robust, fp64).factor, w.T[False])
        ran(pb, "factors", False, n, fp64)
        corr, m6 = pb.factors()
        pairs = check_maha("factors %s %s/%s n=%d" % ("fp64" if fp64 else "fp32", kind, robust, n), rows(corr), m6, w.T[False], kind, fp64, src.c, tc)
        if kind == "GICP" and n == 4097:
            assert pairs > 100, pairs


@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("robust", [None, "HUBER"])
def test_maha_projective(world, robust, fp64):
    w = world
    ps = sga.ProjectiveSearch(w.tgt[False].cloud, 2048, 512)
    for n in SIZES:
        src = src_of(w, n)
        pb = sga.Problem(ps, src.cloud, w.T[False])
        pb.linearize(setting("GICP", robust, fp64).factor, w.T[False])
        ran(pb, "factors", False, n, fp64)
        corr, m6 = pb.factors()
        pairs = check_maha("projective %s GICP/%s n=%d" % ("fp64" if fp64 else "fp32", robust, n), corr, m6, w.T[False], "GICP", fp64, src.c, w.tgt[False].c)
        if n == 4097:
            assert pairs > 100, pairs


def batch_members(w):
    """(framed, n) of the kd batch: sizes 1, 65, 4097 and the framed 4097-point pair"""
    return [(False, 1), (False, 65), (False, 4097), (True, 4097)]


@pytest.mark.parametrize("kind", ["GICP", "ICP", "PLANE_ICP"])
def test_maha_batched_round(world, kind):
    """BatchProblem.linearize marks the matrices invalid and leaves the device-frame pose: every member's factors() rebuilds them from it"""
    w = world
    st = setting(kind)
    members = batch_members(w)
    pbs = [sga.Problem(w.tree[f], src_of(w, n, f).cloud) for f, n in members]
    bp = sga.BatchProblem(pbs)
    u = unit_of(w)
    Ts = [step(w.T[f], 0.003 * u * k) for k, (f, n) in enumerate(members)]
    _, _, _, ninl = bp.linearize(st.factor, Ts)
    for k, (f, n) in enumerate(members):
        ran(pbs[k], "fused_lane", False, n)
        corr, m6 = pbs[k].factors()
        assert int(ninl[k]) == int((corr >= 0).sum())
        check_maha("batch kd %s member %d" % (kind, k), corr, m6, Ts[k], kind, False, src_of(w, n, f).c, w.tgt[f].c)
    del bp
    if kind == "PLANE_ICP":
        return
    mkind = kind  # the map batch: a Gaussian map (GICP) or a flat map (ICP)
    m, _, _, tc, rows = maps_of(w)[mkind]
    sizes = [1, 65, 4097]
    pbs = [sga.Problem(m, src_of(w, n).cloud) for n in sizes]
    bp = sga.BatchProblem(pbs)
    Ts = [step(w.T[False], 0.003 * u * k) for k in range(len(sizes))]
    bp.linearize(st.factor, Ts)
    for k, n in enumerate(sizes):
        ran(pbs[k], "factors", False, n)
        corr, m6 = pbs[k].factors()
        check_maha("batch map %s member %d" % (kind, k), rows(corr), m6, Ts[k], kind, False, src_of(w, n).c, tc)
    del bp


@pytest.mark.parametrize("robust", [None, "HUBER"])
def test_maha_certify(robust):
    """the certify route at its minimum size (kSplitMinPoints = 262 144 source points) against a target of the same size; the float64
    side is the per-pair arrays over the pass's own pairs (no kd-tree query)"""
    n = 262_144
    target, source, T = sga.synthetic.registration_pair(n)
    tgt, src = Cloud(target, True), Cloud(source, False)
    tree = sga.KdTree(tgt.cloud)
    st = setting("GICP", robust)
    pb = sga.Problem(tree, src.cloud)
    pb.linearize(st.factor, T)
    assert tree.spacing() > 0
    T1 = step(T, 0.0015 * tree.spacing() / rm.SPACING_REF)
    pb.linearize(st.factor, T1)
    ran(pb, "certify", True, n)
    corr, m6 = pb.factors()
    pairs = check_maha("certify GICP/%s" % robust, corr, m6, T1, "GICP", False, src.c, tgt.c)
    assert pairs > n // 2, pairs


def test_maha_factors_torch_and_single_outputs(world):
    """factors_torch() bytes equal factors() after an fp64 GICP pass (export_factors_kernel<double>) as after an fp32 one; and
    sga_problem_get_factors with only one of its outputs gives that output unchanged"""
    import ctypes as Ct

    w = world
    src = src_of(w, 4097)
    for fp64 in (False, True):
        for robust in (None, "HUBER"):
            pb = sga.Problem(w.tree[False], src.cloud)
            pb.linearize(setting("GICP", robust, fp64).factor, w.T[False])
            hi, hm = pb.factors()
            ti, tm = pb.factors_torch()
            assert (hi >= 0).sum() > 100 and np.abs(hm).max() > 0
            assert ti.cpu().numpy().tobytes() == hi.tobytes() and tm.cpu().numpy().tobytes() == hm.tobytes(), (fp64, robust)
            check_maha("factors_torch %s/%s" % ("fp64" if fp64 else "fp32", robust), ti.cpu().numpy(), tm.cpu().numpy(), w.T[False], "GICP", fp64, src.c, w.tgt[False].c)
            only_i = np.full(4097, -5, np.int64)
            sga.api.check(sga.load().sga_problem_get_factors(pb.ctx.h, pb.h, only_i.ctypes.data_as(Ct.POINTER(Ct.c_int64)), None))
            only_m = np.full((4097, 6), -5.0, np.float32)
            sga.api.check(sga.load().sga_problem_get_factors(pb.ctx.h, pb.h, None, only_m.ctypes.data_as(Ct.POINTER(Ct.c_float))))
            assert np.array_equal(only_i, hi) and only_m.tobytes() == hm.tobytes(), (fp64, robust)


# ---- (b) the state machine -----------------------------------------------------------------------------------------------------------
class Pair:
    """the 4097-point GICP pair and the check of (a) against the pose, arithmetic and factor of the last linearization"""

    def __init__(self, w, framed=False):
        self.w, self.framed = w, framed
        self.src, self.tgt = src_of(w, 4097, framed), w.tgt[framed]
        self.T0 = w.T[framed]
        self.T1 = step(self.T0, 0.01 * unit_of(w))

    def problem(self):
        return sga.Problem(self.w.tree[self.framed], self.src.cloud)

    def check(self, label, pb, T, kind="GICP", fp64=False):
        corr, m6 = pb.factors()
        pairs = check_maha("state " + label, corr, m6, T, kind, fp64, self.src.c, self.tgt.c)
        assert kind != "GICP" or pairs > 100, (label, pairs)
        return corr, m6


@pytest.mark.parametrize("framed", [False, True])
def test_state_fp32_cold_then_warm(world, framed):
    """1. lin fp32 @T0 -> factors -> lin fp32 @T1 (warm) -> factors"""
    p = Pair(world, framed)
    pb, st = p.problem(), setting("GICP")
    pb.linearize(st.factor, p.T0)
    ran(pb, "fused_lane", False)
    p.check("1 cold", pb, p.T0)
    pb.linearize(st.factor, p.T1)
    ran(pb, "fused_queue", True)
    p.check("1 warm", pb, p.T1)
    p.check("1 warm, asked again", pb, p.T1)


def test_state_stored_then_recomputed(world):
    """2. lin fp32 HUBER @T0 (matrices stored by the factor stage) -> factors -> lin fp32, no robust kernel, @T1 (rebuilt on demand)"""
    p = Pair(world)
    pb = p.problem()
    pb.linearize(setting("GICP", "HUBER").factor, p.T0)
    p.check("2 stored", pb, p.T0)
    pb.linearize(setting("GICP").factor, p.T1)
    ran(pb, "fused_queue", True)
    p.check("2 recomputed", pb, p.T1)
    pb.linearize(setting("GICP", "CAUCHY").factor, p.T0)
    p.check("2 stored again", pb, p.T0)


def test_state_fp64_then_fp32(world):
    """3. lin fp64 @T0 -> factors -> lin fp32 @T1 -> factors: no stale maha64 is exported; and back"""
    p = Pair(world)
    pb = p.problem()
    for robust in (None, "HUBER"):
        pb.linearize(setting("GICP", robust, True).factor, p.T0)
        p.check("3 fp64 %s" % robust, pb, p.T0, fp64=True)
        pb.linearize(setting("GICP", robust, False).factor, p.T1)
        p.check("3 fp32 after fp64 %s" % robust, pb, p.T1, fp64=False)
    pb.linearize(setting("GICP", None, True).factor, p.T1)
    p.check("3 fp64 after fp32", pb, p.T1, fp64=True)


def test_state_factor_kind_changes(world):
    """4. lin GICP -> lin ICP -> factors (zeros) -> lin GICP -> factors"""
    p = Pair(world)
    pb = p.problem()
    pb.linearize(setting("GICP", "HUBER").factor, p.T0)
    pb.linearize(setting("ICP").factor, p.T1)
    p.check("4 ICP after GICP", pb, p.T1, kind="ICP")
    pb.linearize(setting("PLANE_ICP", None, True).factor, p.T1)
    p.check("4 PLANE_ICP", pb, p.T1, kind="PLANE_ICP", fp64=True)
    pb.linearize(setting("GICP").factor, p.T0)
    p.check("4 GICP again", pb, p.T0)


@pytest.mark.parametrize("fp64", [False, True])
def test_state_error_passes_do_not_move_the_matrices(world, fp64):
    """5. lin -> error (model) -> set_error_model(False), error at trial(T) -> factors: the matrices stay those of the linearization"""
    p = Pair(world)
    pb, st = p.problem(), setting("GICP", None, fp64)
    pb.linearize(st.factor, p.T0)
    em = pb.error(st.factor, trial(p.T0))
    sga.set_error_model(False)
    ek = pb.error(st.factor, trial(p.T0))  # the error kernel: rebuilds the matrices it reads, from the pose of the linearization
    assert em > 0 and ek > 0
    p.check("5 after error passes", pb, p.T0, fp64=fp64)


def test_state_async_and_per_point(world):
    """6. linearize_async -> factors.  7. linearize_per_point @T -> factors: both outputs equal those of a twin after linearize(fp64) @T
    (the header: "runs one linearization at T")"""
    p = Pair(world)
    for fp64 in (False, True):
        pb = p.problem()
        buf = torch.full((32,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        pb.linearize_async(setting("GICP", None, fp64).factor, p.T1, buf.data_ptr())
        pb.ctx.synchronize()
        p.check("6 async %s" % ("fp64" if fp64 else "fp32"), pb, p.T1, fp64=fp64)
    for robust in (None, "HUBER"):
        pb, twin = p.problem(), p.problem()
        pb.linearize(setting("GICP", robust).factor, p.T0)  # an fp32 pass at another pose first
        pb.linearize_per_point(setting("GICP", robust).factor, p.T1)
        twin.linearize(setting("GICP", robust, True).factor, p.T1)
        corr, m6 = p.check("7 per-point %s" % robust, pb, p.T1, fp64=True)
        tc, tm = twin.factors()
        assert np.array_equal(corr, tc) and m6.tobytes() == tm.tobytes(), (robust, int((corr != tc).sum()))


def test_state_batched_round_then_lone_pass(world):
    """8. batched round -> each member's factors() -> a lone pass on one member -> factors"""
    w = world
    members = batch_members(w)
    pbs = [sga.Problem(w.tree[f], src_of(w, n, f).cloud) for f, n in members]
    bp = sga.BatchProblem(pbs)
    st = setting("GICP")
    Ts = [w.T[f] for f, _ in members]
    bp.linearize(st.factor, Ts)
    for k, (f, n) in enumerate(members):
        check_maha("state 8 member %d" % k, *pbs[k].factors(), Ts[k], "GICP", False, src_of(w, n, f).c, w.tgt[f].c)
    u = unit_of(w)
    for k in (2, 3):  # a lone pass, fp64 and robust, on the plain and on the framed 4097-point member
        f, n = members[k]
        T1 = step(Ts[k], 0.01 * u)
        pbs[k].linearize(setting("GICP", "HUBER", True).factor, T1)
        check_maha("state 8 lone pass on member %d" % k, *pbs[k].factors(), T1, "GICP", True, src_of(w, n, f).c, w.tgt[f].c)
    bp.linearize(st.factor, Ts)  # and a round after it
    for k, (f, n) in enumerate(members):
        check_maha("state 8 second round member %d" % k, *pbs[k].factors(), Ts[k], "GICP", False, src_of(w, n, f).c, w.tgt[f].c)
    del bp


@pytest.mark.parametrize("robust", [None, "HUBER"])
def test_state_after_a_whole_registration(world, robust):
    """9. a whole registration through sga.optimize with recording callbacks -> factors at the recorded pose of the last linearize"""
    p = Pair(world)
    pb = p.problem()
    st = setting("GICP", robust, max_iterations=10)
    poses = []

    def lin(T):
        poses.append(T.copy())
        return pb.linearize(st.factor, T)

    T_init = step(p.T0, 0.2)
    res = sga.optimize(st, T_init, lin, lambda T: pb.error(st.factor, T))
    assert len(poses) >= 2 and res.iterations >= 1
    p.check("9 after optimize %s (%d passes)" % (robust, len(poses)), pb, poses[-1])


# ---- (c) the per-point export --------------------------------------------------------------------------------------------------------
def per_pair_caller(src, tgt_rec, tgt_nrm, tgt_cov, corr, T, kind, robust, o_s=None, o_t=None):
    """fr.per_pair in the device frames, carried to the caller's twist convention (the module docstring): corr in rows of tgt_rec"""
    o_s = src.origin if o_s is None else o_s
    o_t = np.zeros(3) if o_t is None else o_t
    framed = o_s.any() or o_t.any()
    Td = pose_to_device(T, o_s, o_t) if framed else T
    pp = fr.per_pair(src.rec, tgt_rec, corr, Td, KINDS[kind], ROBUST[robust], C, src.c, tgt_cov, tgt_nrm)
    if o_s.any():
        A = adjoint(o_s)
        aA = np.abs(A)
        pp.H, pp.b = np.einsum("ji,njk,kl->nil", A, pp.H, A), pp.b @ A
        pp.Hmag, pp.bmag = np.einsum("ji,njk,kl->nil", aA, pp.Hmag, aA), pp.bmag @ aA
    return pp


def check_export(label, out, corr, pp, twin_res=None):
    """the per-point export `out` against the pairs `corr` (a twin's fp64 pass) and their restatement pp; its column sums against the
    twin's own sums on check_pass's scales"""
    ok, H, b, e = out
    assert np.array_equal(ok, corr >= 0), (label, int(ok.sum()), int((corr >= 0).sum()), np.flatnonzero(ok != (corr >= 0))[:8])
    assert not H[~ok].any() and not b[~ok].any() and not e[~ok].any(), (label, "outlier rows are zero")
    si = pp.idx
    assert np.array_equal(si, np.flatnonzero(ok))
    if len(si) == 0:
        return
    tiny = 1e-300
    rH = (np.abs(H[si] - pp.H) / (pp.Hmag + tiny)).max()
    rb = (np.abs(b[si] - pp.b) / (pp.bmag + tiny)).max()
    re_ = (np.abs(e[si] - pp.e) / (pp.e + tiny)).max()
    note("per-point H", rH), note("per-point b", rb), note("per-point e", re_)
    print("%-58s pairs %6d  per-point H %.1e  b %.1e  e %.1e  (bound %.0e)" % (label, len(si), rH, rb, re_, FP64_REL))
    k = int(np.argmax((np.abs(b[si] - pp.b) / (pp.bmag + tiny)).max(1)))
    assert rH <= FP64_REL and rb <= FP64_REL and re_ <= FP64_REL, (label, rH, rb, re_, si[k], b[si[k]], pp.b[k])
    if twin_res is not None:
        Ht, bt, et, nt = twin_res
        assert nt == len(si)
        Hs, bs, es = H.sum(0), b.sum(0), e.sum()
        scale = max(np.abs(Ht).max(), tiny)
        bscale = np.sqrt(np.abs(np.diag(Ht)) * max(et, 1e-30)) + 1e-30
        sH, sb, se = np.abs(Hs - Ht).max() / scale, (np.abs(bs - bt) / bscale).max(), abs(es - et) / max(abs(et), tiny)
        note("per-point sums", max(sH, sb, se))
        assert sH <= FP64_REL and sb <= FP64_REL and se <= FP64_REL, (label, sH, sb, se)


@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("kind,robust", FACTORS5)
def test_per_point_kd(world, kind, robust, framed):
    w = world
    tgt = w.tgt[framed]
    T = w.T[framed]
    for n in (1, 65, 4097):
        src = src_of(w, n, framed)
        pb, twin = sga.Problem(w.tree[framed], src.cloud), sga.Problem(w.tree[framed], src.cloud)
        res = twin.linearize(setting(kind, robust, True).factor, T)
        ran(twin, "lane", False, n, True)
        corr, tm = twin.factors()
        out = pb.linearize_per_point(setting(kind, robust).factor, T)
        ran(pb, "lane", False, n, True)
        pp = per_pair_caller(src, tgt.rec, tgt.n, tgt.c, corr, T, kind, robust, o_t=tgt.origin)
        check_export("per-point kd %s/%s n=%d%s" % (kind, robust, n, " framed" if framed else ""), out, corr, pp, res)
        pc, pm = pb.factors()
        assert np.array_equal(pc, corr) and pm.tobytes() == tm.tobytes()  # the state the export leaves is the pass's
        if n == 4097:
            assert len(pp.idx) > 100


@pytest.mark.parametrize("kind", ["ICP", "PLANE_ICP"])
def test_per_point_flat_maps(world, kind):
    w = world
    m, tp, tn, _, rows = maps_of(w)[kind]
    for n in (1, 65, 4097):
        src = src_of(w, n)
        pb, twin = sga.Problem(m, src.cloud), sga.Problem(m, src.cloud)
        res = twin.linearize(setting(kind, None, True).factor, w.T[False])
        ran(twin, "factors", False, n, True)
        corr = rows(twin.factors()[0])
        out = pb.linearize_per_point(setting(kind).factor, w.T[False])
        pp = per_pair_caller(src, tp, tn, None, corr, w.T[False], kind, None)
        check_export("per-point flat map %s n=%d" % (kind, n), out, corr, pp, res)


@pytest.mark.parametrize("kind,robust", FACTORS5)
def test_per_point_with_a_host_rejector(world, kind, robust):
    """The rejector keeps the even targets; max_correspondence_distance = 0.05 is ignored while a callback is set (small_gicp_amd.h).
    The export describes the pairs the pass kept: ok is exactly corr >= 0, and the kept rows match the restatement."""
    w = world
    tgt = w.tgt[False]
    for n in (65, 4097):
        src = src_of(w, n)
        pb = sga.Problem(w.tree[False], src.cloud)
        pb.set_rejector(lambda T, idx, d2: idx % 2 == 1)
        st = setting(kind, robust, maxd=0.05)
        out = pb.linearize_per_point(st.factor, w.T[False])
        ran(pb, "lane", False, n, True)
        corr, m6 = pb.factors()
        kept = corr[corr >= 0]
        assert len(kept) >= n // 4 and (kept % 2 == 0).all(), (n, len(kept))  # far more than a 5 cm rejector would keep
        d2 = fr.sq_dist(src.p, tgt.p, corr, w.T[False])
        assert (d2[corr >= 0] > 0.05 ** 2).sum() > len(kept) // 2
        pp = per_pair_caller(src, tgt.rec, tgt.n, tgt.c, corr, w.T[False], kind, robust)
        check_export("per-point host rejector %s/%s n=%d" % (kind, robust, n), out, corr, pp)
        check_maha("per-point host rejector %s/%s n=%d" % (kind, robust, n), corr, m6, w.T[False], kind, True, src.c, tgt.c)
        pb.set_rejector(None)


def tied_pairs():
    """64 isolated groups along z, 8 m apart: source point k at (0, 0, 8 k); the pose is the pure translation (10 + 2^-28, -(10 + 2^-28), 0),
    so the fp32 query is (10, -10, 8 k) exactly while the double query lies 2^-28 beyond it in x and y.  Groups 0 - 31 have their two target
    points at x = 10 -+ 1 (equidistant from the fp32 query; in double the HIGHER one, x = 11, is nearer by 2^-27), groups 32 - 63 at
    y = -10 -+ 1 (in double the LOWER one, y = -11, is nearer).  Covariances differ from point to point, so a wrong pair shows in M too.
    (The issue's 32 groups per family: "all 64 pairs".)  Returns target (128, 3), source (64, 3) float32, their covariances, T and the
    float64 brute-force nearest target of every source point."""
    rng = np.random.default_rng(5)
    z = 8.0 * np.arange(64)
    src = np.stack([np.zeros(64), np.zeros(64), z], 1).astype(np.float32)
    tgt = np.zeros((128, 3))
    tgt[:, 2] = np.repeat(z, 2)
    tgt[:, 0], tgt[:, 1] = 10.0, -10.0
    sign = np.tile([-1.0, 1.0], 64)
    fam_x = np.repeat(np.arange(64) < 32, 2)
    tgt[fam_x, 0] += sign[fam_x]
    tgt[~fam_x, 1] += sign[~fam_x]
    tgt = tgt.astype(np.float32)

    def covs(m):
        B = rng.normal(size=(m, 3, 3))
        return (0.01 * B @ B.transpose(0, 2, 1) + 0.02 * np.eye(3)).astype(np.float32)

    T = np.eye(4)
    T[:3, 3] = [10.0 + 2.0 ** -28, -(10.0 + 2.0 ** -28), 0.0]
    q = fr.transform(T, src)
    d2 = ((tgt.astype(np.float64)[None] - q[:, None]) ** 2).sum(2)
    best = d2.argmin(1)
    part = np.sort(d2, 1)
    assert (part[:, 1] - part[:, 0] > 2.0 ** -28).all() and (part[:, 1] < 1.0 + 1e-6).all()  # a unique double minimum, a runner-up 2^-27 away
    assert (best[:32] % 2 == 1).all() and (best[32:] % 2 == 0).all()  # x family: the higher coordinate; y family: the lower
    qf = (src + T[:3, 3].astype(np.float32)).astype(np.float32)
    d2f = ((tgt[None] - qf[:, None]) ** 2).sum(2, dtype=np.float32)
    assert (np.sort(d2f, 1)[:, 0] == np.sort(d2f, 1)[:, 1]).all()  # tied in fp32
    return tgt, src, covs(128), covs(64), T, best


def test_per_point_on_pairs_tied_in_fp32():
    """The fp64 pass re-decides between the walk's two candidates in double (factor_stage.hpp); the export must describe the pairs of that
    pass, not the walk's fp32 winners.  First the inputs: an fp32 and an fp64 pass disagree on at least 8 pairs, and the fp64 pass's
    pairs are the float64 brute-force nearest for all 64.  A wrong pair flips the sign of b_i."""
    tp, sp, tc, sc, T, best = tied_pairs()
    tgt_cloud = sga.PointCloud(tp, None, tc)
    src_cloud = sga.PointCloud(sp, None, sc)
    tree = sga.KdTree(tgt_cloud)
    src = World()
    src.rec = src.p = sp.astype(np.float64)
    src.origin, src.c = np.zeros(3), src_cloud.covs()
    tgt_c = tgt_cloud.covs()
    p32, p64 = sga.Problem(tree, src_cloud), sga.Problem(tree, src_cloud)
    _, _, _, n32 = p32.linearize(setting("ICP", maxd=2.0).factor, T)
    _, _, _, n64 = p64.linearize(setting("ICP", None, True, maxd=2.0).factor, T)
    c32, c64 = p32.factors()[0], p64.factors()[0]
    assert n32 == n64 == 64 and (c32 >= 0).all()
    print("tied pairs: fp32 and fp64 passes disagree on %d of 64" % int((c32 != c64).sum()))
    assert (c32 != c64).sum() >= 8, int((c32 != c64).sum())
    assert np.array_equal(c64, best), np.flatnonzero(c64 != best)
    for kind, robust in [("ICP", None), ("GICP", None), ("GICP", "HUBER"), ("GICP", "CAUCHY")]:
        pb, twin = sga.Problem(tree, src_cloud), sga.Problem(tree, src_cloud)
        res = twin.linearize(setting(kind, robust, True, maxd=2.0).factor, T)
        corr, tm = twin.factors()
        assert np.array_equal(corr, best), (kind, robust)
        out = pb.linearize_per_point(setting(kind, robust, maxd=2.0).factor, T)
        pp = per_pair_caller(src, tp.astype(np.float64), None, tgt_c, corr, T, kind, robust)
        check_export("per-point tied pairs %s/%s" % (kind, robust), out, corr, pp, res)
        pc, pm = pb.factors()
        check_maha("per-point tied pairs %s/%s" % (kind, robust), pc, pm, T, kind, True, src.c, tgt_c)
        assert np.array_equal(pc, best) and pm.tobytes() == tm.tobytes(), (kind, robust)
    # the host rejector is shown hint[], the walk's fp32 winner, while the fp64 pass may keep the runner-up: reported, not asserted
    shown = []
    pr = sga.Problem(tree, src_cloud)
    pr.set_rejector(lambda Tc, idx, d2: shown.append(idx.copy()) or np.zeros(len(idx), bool))
    pr.linearize(setting("ICP", None, True).factor, T)
    kept = pr.factors()[0]
    print("tied pairs: an fp64 pass with a host rejector keeps another target than the callback saw for %d of 64 source points" % int((shown[-1] != kept).sum()))
    pr.set_rejector(None)


# ---- (d) the enqueue-only forms ------------------------------------------------------------------------------------------------------
def check_sums(label, res, corr, src, tgt, T, fp64, kind, robust):
    """check_pass's items 1 - 3 (the sums over the pass's own pairs, the count, the symmetry of H) for a system in the CALLER's frame,
    restated in the device frames and carried over with the adjoint (the module docstring); fp32 bounds as check_pass derives them"""
    H, b, e, n = res
    kind_i, rob_i = KINDS[kind], ROBUST[robust]
    Td = pose_to_device(T, src.origin, tgt.origin) if (src.origin.any() or tgt.origin.any()) else T
    ref = fr.linearize(src.rec, tgt.rec, corr, Td, kind_i, rob_i, C, src.c, tgt.c, tgt.n)
    A = adjoint(src.origin)
    Hr, br = A.T @ ref.H @ A, A.T @ ref.b
    bscale = np.sqrt(np.abs(np.diag(Hr)) * max(ref.e, 1e-30)) + 1e-30
    if fp64:
        tH = tB = tE = FP64_REL
    else:
        db, de = rm.rounding_scale(src.rec, tgt.rec, tgt.n, corr, Td, kind_i, rob_i, ref.maha)
        tH = rm.FP32_H
        tB = max(rm.FP32_B, 4 * ((np.abs(A).T @ db) / bscale).max())
        tE = max(rm.FP32_E, 4 * de / max(abs(ref.e), 1e-300))
    assert np.array_equal(H, H.T), label
    d2 = fr.sq_dist(src.rec, tgt.rec, corr, Td)
    paired = corr >= 0
    if fp64:
        assert n == int((d2[paired] <= MAXD * MAXD).sum()) == int(paired.sum()), (label, n, int(paired.sum()))
    else:
        lo, hi = int((d2[paired] <= MAXD * MAXD * (1 - 1e-6)).sum()), int((d2[paired] <= MAXD * MAXD * (1 + 1e-6)).sum())
        assert n == int(paired.sum()) and lo <= n <= hi, (label, n, int(paired.sum()), lo, hi)
    rH = np.abs(H - Hr).max() / max(np.abs(Hr).max(), 1e-300)
    rb = (np.abs(b - br) / bscale).max()
    re_ = abs(e - ref.e) / max(abs(ref.e), 1e-300)
    key = "async %s %s" % ("fp64" if fp64 else "fp32", "framed" if src.origin.any() else "plain")
    note(key + " H", rH / tH), note(key + " b", rb / tB), note(key + " e", re_ / tE)
    print("%-58s inliers %5d  H %.1e  b %.1e  e %.1e  (bounds %.0e %.0e %.0e)" % (label, n, rH, rb, re_, tH, tB, tE))
    assert rH <= tH and rb <= tB and re_ <= tE, (label, rH, rb, re_, (tH, tB, tE))


@pytest.mark.parametrize("framed", [False, True])
@pytest.mark.parametrize("fp64", [False, True])
@pytest.mark.parametrize("kind,robust", [("ICP", None), ("PLANE_ICP", None), ("GICP", None), ("GICP", "HUBER")])
def test_linearize_async(world, kind, robust, fp64, framed):
    """After ctx.synchronize() the 30 doubles unpack to the system of the pass in the caller's frame: check_pass's items 1 - 3 over
    pb.factors(); [28] is the count, [29] zero, the guards untouched.  With zero origins the 30 values equal a twin's sga_linearize to the
    last bit (the same kernels and row order; only the width of the output differs); a framed problem changes frame on the device
    (frames.hip: frame_accumulator_kernel) where sga_linearize does it on the host: within the pass bounds."""
    w = world
    tgt, T = w.tgt[framed], w.T[framed]
    st = setting(kind, robust, fp64)
    for n in (1, 65, 4097):
        src = src_of(w, n, framed)
        pb, twin = sga.Problem(w.tree[framed], src.cloud), sga.Problem(w.tree[framed], src.cloud)
        buf = torch.full((32,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        pb.linearize_async(st.factor, T, buf.data_ptr())
        pb.ctx.synchronize()
        ran(pb, "lane" if fp64 else "fused_lane", False, n, fp64)
        acc = buf.cpu().numpy()
        assert acc[30] == SENT and acc[31] == SENT, acc[28:]
        res = sga.unpack_accumulator(acc[:30])
        corr, _ = pb.factors()
        assert acc[28] == float((corr >= 0).sum()) == res[3] and acc[29] == 0.0, acc[28:]
        label = "linearize_async %s %s/%s n=%d%s" % ("fp64" if fp64 else "fp32", kind, robust, n, " framed" if framed else "")
        check_sums(label, res, corr, src, tgt, T, fp64, kind, robust)
        Ht, bt, et, nt = twin.linearize(st.factor, T)
        if not framed:
            check_pass(label, pb, st, T, res, tgt.p, tgt.n, tgt.c, src.p, src.c, fp64, kind, robust)
            assert np.array_equal(res[0], Ht) and np.array_equal(res[1], bt) and res[2] == et and res[3] == nt, (label, np.abs(res[0] - Ht).max(), res[2] - et)
        else:
            assert nt == res[3]
            check_sums(label + " (sga_linearize)", (Ht, bt, et, nt), twin.factors()[0], src, tgt, T, fp64, kind, robust)


@pytest.mark.parametrize("kind,robust,fp64", [("GICP", None, False), ("GICP", None, True), ("GICP", "HUBER", False), ("ICP", None, False)])
def test_error_async(world, kind, robust, fp64):
    """sga_error_async at the linearization pose and at a trial pose: the value of pb.error with the error model off, bit for bit (both go
    through error_dispatch), and fr.error over the pass's pairs and matrices within check_pass's bound for the error passes"""
    w = world
    src, tgt, T = src_of(w, 4097), w.tgt[False], w.T[False]
    st = setting(kind, robust, fp64)
    pb = sga.Problem(w.tree[False], src.cloud)
    pb.linearize(st.factor, T)
    corr, _ = pb.factors()
    kind_i, rob_i = KINDS[kind], ROBUST[robust]
    ref = fr.linearize(src.p, tgt.p, corr, T, kind_i, rob_i, C, src.c, tgt.c, tgt.n)
    if fp64:
        tErr = FP64_REL
    else:
        _, de = rm.rounding_scale(src.p, tgt.p, tgt.n, corr, T, kind_i, rob_i, ref.maha)
        tErr = max(rm.FP32_ERR, rm.FP32_E, 4 * de / max(abs(ref.e), 1e-300))
    for Tq in (T, trial(T)):
        buf = torch.full((3,), SENT, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        pb.error_async(st.factor, Tq, buf.data_ptr())
        pb.ctx.synchronize()
        out = buf.cpu().numpy()
        assert out[1] == SENT and out[2] == SENT
        sga.set_error_model(False)
        ek = pb.error(st.factor, Tq)
        sga.set_error_model(True)
        assert out[0] == ek, (out[0], ek)
        er = fr.error(src.p, tgt.p, corr, Tq, kind_i, rob_i, C, ref.maha, tgt.n)
        r = abs(out[0] - er) / max(abs(er), 1e-300)
        note("error_async %s" % ("fp64" if fp64 else "fp32"), r / tErr)
        print("error_async %s %s/%s  residual %.1e (bound %.0e)" % ("fp64" if fp64 else "fp32", kind, robust, r, tErr))
        assert r <= tErr, (kind, robust, fp64, r, tErr)


def test_error_async_refuses_another_arithmetic(world):
    """fp32 linearize, then fp64 error_async with GICP: error 1, "another arithmetic", before any launch (error_dispatch returns ahead of
    problem_ensure_maha and the kernel); the buffer and its guards stay as they were"""
    w = world
    pb = sga.Problem(w.tree[False], src_of(w, 4097).cloud)
    pb.linearize(setting("GICP").factor, w.T[False])
    buf = torch.full((3,), SENT, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(sga.SgaError, match=r"error 1: .*another arithmetic"):
        pb.error_async(setting("GICP", None, True).factor, w.T[False], buf.data_ptr())
    pb.ctx.synchronize()
    assert (buf.cpu().numpy() == SENT).all()
    check_maha("after the refusal", *pb.factors(), w.T[False], "GICP", False, src_of(w, 4097).c, w.tgt[False].c)


def test_zz_report():
    """(prints with -s) the worst residuals of this run against their bounds"""
    for k in sorted(WORST):
        print("worst %-28s %.3e" % (k, WORST[k]))
    for k in ("maha fp32", "maha fp64"):
        if k in WORST:
            assert WORST[k] <= MAHA_C

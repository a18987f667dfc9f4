"""Batched registration on the device (csrc/batch.hip, linearize.hip: batch_search_linearize_kernel, reduce_rows.hpp: batch_reduce_rows_kernel,
optimizer.hip: sga_align_batch): several independent pairs linearized by one search + factor launch and one row reduction per round.

  * every batched linearization against a float64 sum over its own pairs: checks 1 - 5 of tests/test_route_matrix.py's header
    (its check_pass, its bounds FP32_H / FP32_B / FP32_E and rounding_scale: the batch kernel does the lone kernel's per-pair
    arithmetic), for every pair of a batch of mixed sizes, two targets of different depth, a geo-referenced pair, all three
    factors, both rejectors, all pairs active and a mask;
  * a pair's sums and result do not depend on the company it keeps, bit for bit;
  * align against the oracle and against Problem.align (test_gpu_parity.py::test_align_matches_golden's assertions and values);
  * the batched odometry driver against the sequential one;
  * the scope limits on a live device.
"""
import ctypes as C

import numpy as np
import pytest

import factor_ref as fr
import small_gicp_amd as sga
import test_route_matrix as rm
from conftest import pose_error

pytestmark = pytest.mark.gpu

POSE_TOL_T, POSE_TOL_R = 1e-4, 1e-4  # the project's north-star tolerance (test_gpu_parity.py)
SIZES = [1, 63, 64, 65, 1000, 11_000, 70_000]  # a one-point pair, a partial last tile, exactly one tile, one tile + 1, ..., a pair larger than all others together
SHIFT = np.array([1_000_064.0, -2_000_000.0, 128.0])  # multiples of 128 m (common.hpp: kOriginQuantum): the geo-referenced pair's origin


class Target:
    def __init__(self, points64, k=10):
        from scipy.spatial import cKDTree

        self.cloud = sga.PointCloud(points64)
        sga.estimate_normals_covariances(self.cloud, None, k)
        self.tree = sga.KdTree(self.cloud)
        self.tp = self.cloud.xyz64()
        self.tn = self.cloud.normals()[:, :3]
        self.tc = self.cloud.covs()
        self.kd = cKDTree(self.tp)


class Source:
    def __init__(self, points64, k=10):
        self.cloud = sga.PointCloud(points64)
        sga.estimate_covariances(self.cloud, None, k)
        self.sp = self.cloud.xyz64()
        self.sc = self.cloud.covs()


def conj(T, s):
    """the rigid motion T between frames both shifted by s"""
    S = np.eye(4)
    S[:3, 3] = s
    Si = np.eye(4)
    Si[:3, 3] = -s
    return S @ T @ Si


@pytest.fixture(scope="module")
def world():
    """two targets of different tree depth and a geo-referenced one; per batch slot (target, source, pose)"""
    ta, sa, T = sga.synthetic.registration_pair(200_000)
    tb, sb, _ = sga.synthetic.registration_pair(20_000, target_seed=3, source_seed=4)
    A, B = Target(ta.astype(np.float64)), Target(tb.astype(np.float64))
    G = Target(ta[:120_000].astype(np.float64) + SHIFT)
    assert np.abs(G.cloud.origin() - SHIFT).max() < 128.0 and np.abs(G.cloud.origin()).max() > 9e5
    slots = []
    for k, n in enumerate(SIZES):
        if n == 70_000:  # the large pair is the geo-referenced one: its pose enters the kernel between ITS two device frames
            slots.append((G, Source(sa[:n].astype(np.float64) + SHIFT), conj(T, SHIFT)))
        else:
            tgt, pts = (A, sa) if k % 2 == 0 else (B, sb)
            slots.append((tgt, Source(pts[:n].astype(np.float64)), T))
    return slots


def nearest(tgt, src, T):
    q = fr.transform(T, src.sp)
    _, idx = tgt.kd.query(q, k=2, workers=16)
    idx = idx.reshape(len(q), 2)
    return q, idx, ((tgt.tp[idx] - q[:, None, :]) ** 2).sum(2)


@pytest.fixture(autouse=True)
def restore_modes():
    yield
    sga.set_error_model(True)


@pytest.mark.parametrize("kind", ["ICP", "PLANE_ICP", "GICP"])
@pytest.mark.parametrize("maxd", [1.0, None])
def test_batched_linearize_against_fp64_sums(world, kind, maxd):
    """checks 1 - 5 of test_route_matrix.py for every pair; then a masked round at another pose: the masked pairs' outputs and
    problem state stay untouched, the others are checked again."""
    st = sga.make_setting(kind, max_correspondence_distance=maxd)
    max_sq = np.inf if maxd is None else maxd * maxd
    problems = [sga.Problem(t.tree, s.cloud) for t, s, _ in world]
    depths = {int(np.ceil(np.log2(max(2, len(t.tp))))) for t, _, _ in world}
    assert len(depths) >= 2  # targets of different tree depth share one launch (the LDS stack follows the deepest)
    bp = sga.BatchProblem(problems)
    Ts = [T for _, _, T in world]
    H, b, e, n = bp.linearize(st.factor, Ts)
    for k, (t, s, T) in enumerate(world):
        rm.check_pass("batch %s/%s pair %d" % (kind, maxd, k), problems[k], st, T, (H[k], b[k], e[k], int(n[k])), t.tp, t.tn, t.tc, s.sp, s.sc, False, kind, None, nearest(t, s, T), max_sq)
        assert problems[k].last_plan()["route"] == "fused_lane"
    # the masked round: first, last and one in the middle left out, sentinels in their outputs
    B = len(world)
    active = np.ones(B, bool)
    active[[0, 3, B - 1]] = False
    T2 = [rm.step(T, 0.03) for T in Ts]
    corr_before = {k: problems[k].factors()[0].copy() for k in np.flatnonzero(~active)}
    sent = (np.full((B, 6, 6), -7.5), np.full((B, 6), -7.5), np.full(B, -7.5), np.full(B, 12345, np.uint64))
    H2, b2, e2, n2 = bp.linearize(st.factor, T2, active, out=tuple(a.copy() for a in sent))
    for k, (t, s, _) in enumerate(world):
        if not active[k]:
            assert np.array_equal(H2[k], sent[0][k]) and np.array_equal(b2[k], sent[1][k]) and e2[k] == -7.5 and n2[k] == 12345
            assert np.array_equal(problems[k].factors()[0], corr_before[k])
        else:
            rm.check_pass("batch masked %s/%s pair %d" % (kind, maxd, k), problems[k], st, T2[k], (H2[k], b2[k], e2[k], int(n2[k])), t.tp, t.tn, t.tc, s.sp, s.sc, False, kind, None, nearest(t, s, T2[k]), max_sq)
    del bp


def test_geo_referenced_pair_equals_its_twin_at_the_origin(world):
    """The 70 000-point pair 1 000 km from the origin next to the same pair at the origin, in one batch: the device records are the same
    (the shift is a multiple of 128 m), the poses agree to the rounding of t' = R o_s + t - o_t (1e-9 m in double, at most an ulp of
    the fp32 pose, 1e-5 m at 100 m: 7e-4 of a 3 cm residual's error term), so e agrees to 1e-3 and the inliers to 2."""
    tG, sG, TG = world[-1]
    twin_t = Target(tG.tp - SHIFT)
    twin_s = Source(sG.sp - SHIFT)
    st = sga.make_setting("GICP")
    pbs = [sga.Problem(tG.tree, sG.cloud), sga.Problem(twin_t.tree, twin_s.cloud)]
    bp = sga.BatchProblem(pbs)
    H, b, e, n = bp.linearize(st.factor, [TG, conj(TG, -SHIFT)])
    print("geo e %.9g twin e %.9g inliers %d %d" % (e[0], e[1], n[0], n[1]))
    assert abs(e[0] - e[1]) <= 1e-3 * abs(e[1]) and abs(int(n[0]) - int(n[1])) <= 2 and n[1] > 60_000
    # H_tt does not depend on the frame
    assert np.abs(H[0][3:, 3:] - H[1][3:, 3:]).max() <= 1e-3 * np.abs(H[1][3:, 3:]).max()
    del bp


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error"))


def test_a_pair_does_not_depend_on_its_company(world):
    """H, b, e, inliers and the final result of one pair, bit for bit: alone, first and last of a batch of 16, beside pairs that
    converge earlier or later, and in a second run of the same batch.  (Rows are indexed by the pair's local tile and added in a fixed order.)"""
    tgt, src, T = world[5]  # the 11 000-point pair
    others = [world[k % len(world)] for k in range(15)]
    st = sga.make_setting("GICP")
    # initial poses at different distances from the optimum: the neighbours finish in different rounds
    inits = [rm.step(w[2], 0.02 * (k % 5)) for k, w in enumerate(others)]
    init = rm.step(T, 0.1)

    def run(pos):
        ws = list(others)
        ins = list(inits)
        if pos is not None:
            ws.insert(pos, (tgt, src, T))
            ins.insert(pos, init)
        else:
            ws, ins, pos = [(tgt, src, T)], [init], 0
        pbs = [sga.Problem(t.tree, s.cloud) for t, s, _ in ws]
        bp = sga.BatchProblem(pbs)
        lin = bp.linearize(st.factor, [w[2] for w in ws])
        res = bp.align(st, ins)
        del bp
        return tuple(a[pos].copy() for a in lin), res[pos], [r.iterations for r in res]

    lin1, res1, _ = run(None)
    lin_first, res_first, its = run(0)
    lin_last, res_last, _ = run(15)
    lin_again, res_again, _ = run(15)
    assert len(set(its)) > 1, its  # the company did finish in different rounds
    for lin, res in ((lin_first, res_first), (lin_last, res_last), (lin_again, res_again)):
        assert all(np.array_equal(x, y) for x, y in zip(lin, lin1))
        assert _same(res, res1), (res, res1)
    assert res1.converged


def _oracle_cloud(orc, cloud, tree=True):
    nr = cloud.normals()[:, :3] if cloud._has()[0] else None
    return orc.Cloud(cloud.xyz().astype(np.float64), nr, cloud.covs()[:, :3, :3], tree=tree)


def test_align_batch_matches_oracle_and_lone_path(orc, c1_f32):
    """C1 (GICP, PLANE_ICP, ICP: one batch each, the C1 pair at three initial poses) and eight KITTI-shaped pairs (GICP) in one batch:
    pose within 1e-4 m / 1e-4 rad of the oracle's align on the identical inputs, iterations and converged equal to the oracle's and to
    Problem.align's on the pair alone, inliers within 2, error within 1e-4 relative (test_align_matches_golden's assertions)."""
    d = c1_f32
    tgt = sga.PointCloud(d["tp"], d["tn"], d["tc"])
    src = sga.PointCloud(d["sp"], d["sn"], d["sc"])
    tree = sga.KdTree(tgt)

    def compare(label, res, lone, ref):
        dt, dr = pose_error(res.T_target_source, ref.T_target_source)
        print("%-22s dt %.2e dr %.2e iterations %d / lone %d / oracle %d inliers %d / %d error rel %.1e" % (label, dt, dr, res.iterations, lone.iterations, ref.iterations, res.num_inliers, ref.num_inliers, abs(res.error - ref.error) / abs(ref.error)))
        assert dt < POSE_TOL_T and dr < POSE_TOL_R, (label, dt, dr)
        assert res.iterations == ref.iterations == lone.iterations and res.converged == ref.converged == lone.converged, label
        assert abs(res.num_inliers - ref.num_inliers) <= 2, label
        assert abs(res.error - ref.error) <= 1e-4 * abs(ref.error), label

    inits = [np.eye(4), rm.step(np.eye(4), 0.05), rm.step(np.eye(4), -0.04)]
    for name, kind in (("GICP", orc.GICP), ("PLANE_ICP", orc.PLANE_ICP), ("ICP", orc.ICP)):
        st = sga.make_setting(name)
        os_ = orc.default_setting(factor_kind=kind, num_threads=1)
        pbs = [sga.Problem(tree, src) for _ in inits]
        bp = sga.BatchProblem(pbs)
        res = bp.align(st, inits)
        del bp
        for k, T0 in enumerate(inits):
            lone = sga.Problem(tree, src).align(st, T0)
            compare("C1 %s init %d" % (name, k), res[k], lone, orc.align(d["otc"], d["osc"], os_, T0))
    # eight KITTI-shaped pairs, preprocessed as test_scan_to_scan_odometry_matches_oracle does: 0.25 m voxel grid, covariances k = 20
    frames = []
    for f in range(9):
        pts, _ = sga.synthetic.kitti_like_scan(f)
        cloud = sga.voxelgrid_sampling(sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32)), 0.25)
        ktree = sga.KdTree(cloud)
        sga.estimate_covariances(cloud, ktree, 20)
        frames.append((cloud, ktree, _oracle_cloud(orc, cloud)))
    st = sga.make_setting("GICP")
    os_ = orc.default_setting(factor_kind=orc.GICP, num_threads=8)
    pbs = [sga.Problem(frames[i - 1][1], frames[i][1], np.eye(4)) for i in range(1, 9)]
    bp = sga.BatchProblem(pbs)
    res = bp.align(st)
    del bp
    for i in range(1, 9):
        lone = sga.Problem(frames[i - 1][1], frames[i][1], np.eye(4)).align(st, np.eye(4))
        compare("KITTI pair %d" % i, res[i - 1], lone, orc.align(frames[i - 1][2], frames[i][2], os_))


def test_align_batch_convenience_function(c1_f32):
    d = c1_f32
    tgt = sga.PointCloud(d["tp"], d["tn"], d["tc"])
    src = sga.PointCloud(d["sp"], d["sn"], d["sc"])
    tree = sga.KdTree(tgt)
    res = sga.align_batch([tree, tree], [src, src])
    lone = sga.Problem(tree, src).align(sga.make_setting("GICP"))
    assert len(res) == 2 and _same(res[0], res[1]) and res[0].iterations == lone.iterations
    dt, dr = pose_error(res[0].T_target_source, lone.T_target_source)
    assert dt < POSE_TOL_T and dr < POSE_TOL_R
    assert sga.align_batch([], []) == []


@pytest.mark.parametrize("batch", [1, 4, 8])
def test_batched_odometry_matches_sequential(batch):
    """9 synthetic frames: the per-frame relative poses of the batched driver within 1e-4 m / 1e-4 rad of odometry.run_synthetic's, and the
    same mean iteration count (batch = 4 and 8 end on a group smaller than / equal to the batch; bit-identity is not required: the sum order differs)."""
    from small_gicp_amd import odometry

    seq = _sequential()
    got = odometry.run_synthetic_batched(9, batch=batch)
    assert len(got["relative_poses"]) == 8
    for i in range(1, 9):
        rel = np.linalg.inv(seq["estimated"][i - 1]) @ seq["estimated"][i]
        dt, dr = pose_error(got["relative_poses"][i - 1], rel)
        assert dt < POSE_TOL_T and dr < POSE_TOL_R, (batch, i, dt, dr)
    assert got["mean_iterations"] == seq["mean_iterations"], (got["iterations"], seq["mean_iterations"])


_SEQ = {}


def _sequential():
    from small_gicp_amd import odometry

    if not _SEQ:
        _SEQ.update(odometry.run_synthetic(9))
    return _SEQ


def test_scope_limits_on_a_live_device(c1_f32):
    """Voxel-map target, fp64 arithmetic, a robust kernel, a host rejector, a problem of another context: each gives its status, and the
    member problems still work through the lone path afterwards."""
    lib = sga.load()
    INVALID, UNSUPPORTED = 1, 4
    d = c1_f32
    tgt = sga.PointCloud(d["tp"], d["tn"], d["tc"])
    src = sga.PointCloud(d["sp"], d["sn"], d["sc"])
    tree = sga.KdTree(tgt)
    st = sga.make_setting("GICP")
    want = sga.Problem(tree, src).align(st)
    vm = sga.GaussianVoxelMap(1.0)
    vm.insert(tgt)
    pv = sga.Problem(vm, src)
    with pytest.raises(sga.SgaError, match="error %d" % UNSUPPORTED):
        sga.BatchProblem([sga.Problem(tree, src), pv])
    other = sga.Context(0)
    po = sga.Problem(tree, src, ctx=other)
    pbs = [sga.Problem(tree, src), sga.Problem(tree, src)]
    out = C.c_void_p()
    hs = (C.c_void_p * 2)(pbs[0].h.value, po.h.value)
    assert lib.sga_batch_create(pbs[0].ctx.h, hs, 2, C.byref(out)) == INVALID and not out.value
    bp = sga.BatchProblem(pbs)
    n = C.c_size_t()
    assert lib.sga_batch_size(bp.h, C.byref(n)) == 0 and n.value == 2
    res = (sga._lib.ResultC * 2)()
    for kw in (dict(math_mode="fp64"), dict(robust_kernel="HUBER")):
        assert lib.sga_align_batch(bp.ctx.h, bp.h, None, C.byref(sga.make_setting("GICP", **kw)), res) == UNSUPPORTED
    assert lib.sga_align_batch(other.h, bp.h, None, C.byref(st), res) == INVALID  # the batch belongs to another context
    pbs[1].set_rejector(lambda T, idx, d2: d2 > 1.0)
    assert lib.sga_align_batch(bp.ctx.h, bp.h, None, C.byref(st), res) == UNSUPPORTED
    pbs[1].set_rejector(None)
    sga.set_error_model(False)
    assert lib.sga_align_batch(bp.ctx.h, bp.h, None, C.byref(st), res) == UNSUPPORTED
    sga.set_error_model(True)
    got = bp.align(st)
    assert _same(got[0], got[1]) and got[0].iterations == want.iterations
    del bp
    for pb in pbs + [po, pv]:  # the members, the foreign problem and the voxel-map problem through the lone path
        r = pb.align(st)
        assert r.converged and (pb is pv or pose_error(r.T_target_source, want.T_target_source)[0] < 1e-4)
    # an empty batch does nothing
    eb = sga.BatchProblem([])
    assert eb.align(st) == [] and len(eb) == 0

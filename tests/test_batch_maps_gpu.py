"""Batched registration against voxel-map targets (csrc/linearize.hip: batch_map_linearize_kernel, batch_round; csrc/batch.hip): B pairs whose
targets are all Gaussian voxel maps (VGICP) or all flat maps, linearized by one factor launch and one row reduction per round.

  * every batched linearization against a float64 sum over its own pairs: checks 1, 2, 3 and 5 of tests/test_route_matrix.py's header (its
    check_pass, FP32_* bounds and rounding_scale; no nearest-neighbour check: a map lookup is no global neighbour), for maps of different
    leaf size and search offsets in one launch, pairs sharing a map at different poses, all pairs active and a mask;
  * the correspondences are those of a lone pass over the same map and cloud at the same pose, element for element;
  * a pair's sums do not depend on the company it keeps, bit for bit;
  * a geo-referenced pair next to its twin at the origin;
  * align against Problem.align on each pair alone;
  * empty members, the refusals, an incremental map that grows.
"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
import test_route_matrix as rm
from conftest import pose_error

pytestmark = pytest.mark.gpu

POSE_TOL_T, POSE_TOL_R = 1e-4, 1e-4  # the project's north-star tolerance (test_gpu_parity.py)
SIZES = [1, 63, 64, 65, 1000, 11_000]  # a one-point pair, a partial tile, exactly one tile, one tile + 1, ..., a C5-sized pair
SHIFT = np.array([1_000_064.0, -2_000_000.0, 128.0])  # multiples of 128 m (common.hpp: kOriginQuantum): the geo-referenced pair's origin
INVALID, UNSUPPORTED = 1, 4


class Source:
    def __init__(self, points, k=10):
        self.cloud = sga.PointCloud(points)
        sga.estimate_covariances(self.cloud, None, k)
        self.sp = self.cloud.xyz64()
        self.sc = self.cloud.covs()


class Map:
    """a voxel map with its contents as check_pass wants them: rows of points (float64), normals, covariances, and the numbering of
    Problem.factors() -> those rows (Gaussian: the voxel id; flat: (voxel << 32) | slot -> the voxel-major point list of download())"""

    def __init__(self, cls, leaf, cloud, offsets):
        self.m = cls(leaf)
        self.m.insert(cloud)
        self.m.set_search_offsets(offsets)
        self.tn = self.tc = None
        if cls is sga.GaussianVoxelMap:
            _, means, c6, _ = self.m.download()
            self.tp = means.astype(np.float64)
            self.tc = np.zeros((len(c6), 3, 3))
            self.tc[:] = sga.api.mats_from_sym6(c6.astype(np.float64))
            self.rows = lambda idx: idx
        else:
            d = self.m.download()
            self.tp = d[2].astype(np.float64)
            if cls is sga.IncrementalVoxelMapNormal:
                self.tn = d[3].astype(np.float64)
            if cls is sga.IncrementalVoxelMapCov:
                self.tc = np.zeros((len(d[3]), 3, 3))
                self.tc[:] = sga.api.mats_from_sym6(d[3].astype(np.float64))
            self.rows = lambda idx, c=d[1]: rm._slot_rows(idx, c)


class Mapped:
    """Problem.factors() in the map's row numbering (test_route_matrix.py::test_factors_voxel_maps's local class, restated)"""

    def __init__(self, pb, rows):
        self.pb, self.rows = pb, rows

    def factors(self):
        c, mm = self.pb.factors()
        return self.rows(c), mm

    def error(self, f, T):
        return self.pb.error(f, T)


FLAT = {"ICP": sga.IncrementalVoxelMap, "PLANE_ICP": sga.IncrementalVoxelMapNormal, "GICP": sga.IncrementalVoxelMapCov}


@pytest.fixture(scope="module")
def world():
    """two target clouds of different size, the sources of SIZES cut from the two source clouds, and the maps built on demand"""
    ta, sa, T = sga.synthetic.registration_pair(20_000)
    tb, sb, _ = sga.synthetic.registration_pair(12_000, target_seed=3, source_seed=4)
    w = type("World", (), {})()
    w.T = T
    w.tgt = []
    for t in (ta, tb):
        c = sga.PointCloud(t)
        sga.estimate_normals_covariances(c, None, 10)
        w.tgt.append(c)
    w.src = [Source((sa if k % 2 == 0 else sb)[:n]) for k, n in enumerate(SIZES)]
    w.maps = {}

    def maps(family, kind):
        """(first map, second map): the second over the other cloud, with another leaf size and 7 search offsets instead of 1"""
        key = (family, kind if family == "flat" else None)
        if key not in w.maps:
            if family == "gaussian":
                w.maps[key] = (Map(sga.GaussianVoxelMap, 1.0, w.tgt[0], 1), Map(sga.GaussianVoxelMap, 0.7, w.tgt[1], 7))
            else:
                w.maps[key] = (Map(FLAT[kind], 0.5, w.tgt[0], 1), Map(FLAT[kind], 0.8, w.tgt[1], 7))
        return w.maps[key]

    def slots(family, kind):
        """per batch slot (map, source, pose): even slots share the first map, odd ones the second, every slot at a pose of its own"""
        m = maps(family, kind)
        return [(m[k % 2], w.src[k], rm.step(T, 0.01 * k)) for k in range(len(SIZES))]

    w.slots = slots
    return w


@pytest.fixture(autouse=True)
def restore_modes():
    yield
    sga.set_error_model(True)


def check(label, pb, st, T, res, m, s, kind, max_sq):
    rm.check_pass(label, Mapped(pb, m.rows), st, T, res, m.tp, m.tn, m.tc, s.sp, s.sc, False, kind, None, None, max_sq)


CASES = [("gaussian", "GICP", 1.0), ("gaussian", "GICP", None), ("gaussian", "ICP", 1.0), ("gaussian", "ICP", None), ("flat", "ICP", 1.0), ("flat", "PLANE_ICP", 1.0), ("flat", "GICP", 1.0)]


@pytest.mark.parametrize("family,kind,maxd", CASES)
def test_batched_map_linearize_against_fp64_sums(world, family, kind, maxd):
    """checks 1, 2, 3, 5 of test_route_matrix.py for every pair of a batch over two maps of different leaf size and offsets; the route
    reported; then a masked round at a stepped pose: the masked pairs' outputs and problem state stay untouched, the others are checked again."""
    st = sga.make_setting(kind, max_correspondence_distance=maxd)
    max_sq = np.inf if maxd is None else maxd * maxd
    sl = world.slots(family, kind)
    problems = [sga.Problem(m.m, s.cloud) for m, s, _ in sl]
    bp = sga.BatchProblem(problems)
    Ts = [T for _, _, T in sl]
    H, b, e, n = bp.linearize(st.factor, Ts)
    assert n[-1] > 1000  # the large pair does find the map
    for k, (m, s, T) in enumerate(sl):
        check("batch %s %s/%s pair %d" % (family, kind, maxd, k), problems[k], st, T, (H[k], b[k], e[k], int(n[k])), m, s, kind, max_sq)
        plan = problems[k].last_plan()
        assert plan == {"route": "factors", "warm": False, "grid": False, "pts": 1, "tail": False, "chunk_tiles": 0, "reduce_rows": -(-SIZES[k] // 64), "reduce_groups": 1}, plan
    B = len(sl)
    active = np.ones(B, bool)
    active[[0, 3, B - 1]] = False
    T2 = [rm.step(T, 0.03) for T in Ts]
    corr_before = {k: problems[k].factors()[0].copy() for k in np.flatnonzero(~active)}
    sent = (np.full((B, 6, 6), -7.5), np.full((B, 6), -7.5), np.full(B, -7.5), np.full(B, 12345, np.uint64))
    H2, b2, e2, n2 = bp.linearize(st.factor, T2, active, out=tuple(a.copy() for a in sent))
    for k, (m, s, _) in enumerate(sl):
        if not active[k]:
            assert np.array_equal(H2[k], sent[0][k]) and np.array_equal(b2[k], sent[1][k]) and e2[k] == -7.5 and n2[k] == 12345
            assert np.array_equal(problems[k].factors()[0], corr_before[k])
        else:
            check("batch masked %s %s/%s pair %d" % (family, kind, maxd, k), problems[k], st, T2[k], (H2[k], b2[k], e2[k], int(n2[k])), m, s, kind, max_sq)
    del bp


@pytest.mark.parametrize("family,kind", [("gaussian", "GICP"), ("flat", "ICP"), ("flat", "PLANE_ICP"), ("flat", "GICP")])
def test_correspondences_equal_the_lone_pass(world, family, kind):
    """factors()[0] after the batched round == a fresh Problem's after a lone linearize at the same pose (the same fp32 transform and
    lookup), and the inlier counts are equal.  Flat maps: sga_linearize_per_point keeps working on a member (its inliers are the round's)."""
    st = sga.make_setting(kind)
    sl = world.slots(family, kind)
    problems = [sga.Problem(m.m, s.cloud) for m, s, _ in sl]
    bp = sga.BatchProblem(problems)
    _, _, _, n = bp.linearize(st.factor, [T for _, _, T in sl])
    for k, (m, s, T) in enumerate(sl):
        lone = sga.Problem(m.m, s.cloud)
        _, _, _, nl = lone.linearize(st.factor, T)
        got, want = problems[k].factors()[0], lone.factors()[0]
        assert np.array_equal(got, want), (kind, k, int((got != want).sum()))
        assert int(n[k]) == int(nl), (kind, k, n[k], nl)
    if family == "flat":
        k = 4  # the 1000-point pair
        corr = problems[k].factors()[0]
        ok = problems[k].linearize_per_point(st.factor, sl[k][2])[0]
        assert abs(int(ok.sum()) - int((corr >= 0).sum())) <= 2  # (the export decides in fp64: a pair within rounding of the rejector's reach may differ)
    del bp


@pytest.mark.parametrize("family,kind", [("gaussian", "GICP"), ("flat", "GICP")])
def test_a_pair_does_not_depend_on_its_company(world, family, kind):
    """H, b, e and the inlier count of the 11 000-point pair, bit for bit: alone in a batch of one, first of six, last of six, and beside
    masked-out pairs (rows are indexed by the pair's local tile and added in a fixed order)."""
    st = sga.make_setting(kind)
    sl = world.slots(family, kind)
    me, others = sl[5], [sl[k] for k in (4, 3, 2, 1, 4)]

    def run(pos, mask=False):
        ws = list(others) if pos is not None else []
        pos = 0 if pos is None else pos
        ws.insert(pos, me)
        pbs = [sga.Problem(m.m, s.cloud) for m, s, _ in ws]
        bp = sga.BatchProblem(pbs)
        active = None
        if mask:
            active = np.zeros(len(ws), bool)
            active[[pos, 1]] = True
        out = bp.linearize(st.factor, [T for _, _, T in ws], active)
        del bp
        return tuple(np.array(a[pos]).copy() for a in out)

    alone = run(None)
    assert alone[3] > 1000
    for label, got in (("first", run(0)), ("last", run(5)), ("masked", run(5, True)), ("masked first", run(0, True))):
        assert all(np.array_equal(x, y) for x, y in zip(got, alone)), label


def conj(T, s):
    """the rigid motion T between frames both shifted by s"""
    S, Si = np.eye(4), np.eye(4)
    S[:3, 3], Si[:3, 3] = s, -s
    return S @ T @ Si


def test_geo_referenced_pair_equals_its_twin_at_the_origin(world):
    """A Gaussian map and its source 1 000 km from the origin next to the same pair at the origin, in one batch; the assertions and bounds of
    test_batch_gpu.py's test of the same name (e within 1e-3 relative, inliers within 2, H_tt within 1e-3 relative).  Leaf 2 m: voxel
    coordinates are the caller's and a map indexes 21 bits of them per axis (voxel_hash.hpp), so at -2 000 000 m a 1 m grid is out of range;
    the shift is a whole number of voxels, so both maps hold the same voxels."""
    tp = world.tgt[0].xyz64()
    sp = world.src[5].sp
    T = world.T
    st = sga.make_setting("GICP", max_correspondence_distance=2.0)
    clouds = []
    for s in (SHIFT, np.zeros(3)):
        t = sga.PointCloud(tp + s)
        sga.estimate_covariances(t, None, 10)
        m = sga.GaussianVoxelMap(2.0)
        m.insert(t)
        clouds.append((m, Source(sp + s)))
    assert np.abs(clouds[0][1].cloud.origin() - SHIFT).max() < 128.0
    pbs = [sga.Problem(m, s.cloud) for m, s in clouds]
    bp = sga.BatchProblem(pbs)
    H, b, e, n = bp.linearize(st.factor, [conj(T, SHIFT), T])
    print("geo e %.9g twin e %.9g inliers %d %d of %d" % (e[0], e[1], n[0], n[1], len(sp)))
    assert abs(e[0] - e[1]) <= 1e-3 * abs(e[1]) and abs(int(n[0]) - int(n[1])) <= 2 and n[1] > len(sp) // 2
    assert np.abs(H[0][3:, 3:] - H[1][3:, 3:]).max() <= 1e-3 * np.abs(H[1][3:, 3:]).max()  # H_tt does not depend on the frame
    del bp


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error"))


@pytest.fixture(scope="module")
def frames():
    """six KITTI-shaped scans, preprocessed as the odometry does: 0.25 m voxel grid, covariances k = 20"""
    out = []
    for f in range(6):
        pts, _ = sga.synthetic.kitti_like_scan(f)
        cloud = sga.voxelgrid_sampling(sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32)), 0.25)
        sga.estimate_covariances(cloud, sga.KdTree(cloud), 20)
        out.append(cloud)
    return out


@pytest.mark.parametrize("family", ["gaussian", "flat"])
def test_align_batch_matches_the_lone_path(frames, family):
    """VGICP (Gaussian map, leaf 1 m) and GICP on IncrementalVoxelMapCov, five consecutive scan pairs from the identity: BatchProblem.align
    and align_batch against Problem.align on each pair alone — pose within 1e-4 m / 1e-4 rad, converged equal, iterations within 1 (the
    lone kernel groups its fp32 partial sums differently: a termination test can flip on rounding) — and a pair's result is identical in
    a batch of one and of five."""
    st = sga.make_setting("GICP")

    def make(cloud):
        if family == "gaussian":
            m = sga.GaussianVoxelMap(1.0)
        else:
            m = sga.IncrementalVoxelMapCov(1.0)
            m.set_search_offsets(7)
        m.insert(cloud)
        return m

    maps = [make(frames[i]) for i in range(5)]
    srcs = [frames[i + 1] for i in range(5)]
    pbs = [sga.Problem(m, s, np.eye(4)) for m, s in zip(maps, srcs)]
    bp = sga.BatchProblem(pbs)
    res = bp.align(st)
    del bp
    conv = sga.align_batch(maps, srcs, None, st)
    one = sga.BatchProblem([sga.Problem(maps[2], srcs[2], np.eye(4))])
    alone = one.align(st)[0]
    del one
    assert _same(alone, res[2]), (alone, res[2])
    for k in range(5):
        lone = sga.Problem(maps[k], srcs[k], np.eye(4)).align(st, np.eye(4))
        dt, dr = pose_error(res[k].T_target_source, lone.T_target_source)
        print("%s pair %d: dt %.2e dr %.2e iterations batch %d / lone %d inliers %d / %d" % (family, k, dt, dr, res[k].iterations, lone.iterations, res[k].num_inliers, lone.num_inliers))
        assert lone.converged and lone.iterations < st.max_iterations, (k, lone)  # the premise: a pair the lone path converges on
        assert dt < POSE_TOL_T and dr < POSE_TOL_R, (k, dt, dr)
        assert res[k].converged == lone.converged and abs(res[k].iterations - lone.iterations) <= 1, (k, res[k], lone)
        assert _same(conv[k], res[k]), (k, conv[k], res[k])


def test_empty_members_and_a_growing_map(world):
    """An empty source and a map with nothing inserted each get zero sums and all -1 correspondences while their neighbours are correct;
    after an insert into the (incremental) map a batch over re-created problems finds it."""
    st = sga.make_setting("GICP")
    m, s, T = world.slots("gaussian", "GICP")[4]
    nothing = sga.GaussianVoxelMap(1.0)
    empty_src = sga.PointCloud(np.zeros((0, 3), np.float32), covs=np.zeros((0, 3, 3), np.float32))

    def build():
        pbs = [sga.Problem(m.m, s.cloud), sga.Problem(m.m, empty_src), sga.Problem(nothing, s.cloud), sga.Problem(m.m, s.cloud)]
        return pbs, sga.BatchProblem(pbs)

    pbs, bp = build()
    H, b, e, n = bp.linearize(st.factor, [T] * 4)
    for k in (1, 2):
        assert not H[k].any() and not b[k].any() and e[k] == 0.0 and n[k] == 0
    assert (pbs[2].factors()[0] == -1).all() and len(pbs[1].factors()[0]) == 0
    for k in (0, 3):
        check("beside empty members, pair %d" % k, pbs[k], st, T, (H[k], b[k], e[k], int(n[k])), m, s, "GICP", 1.0)
    assert np.array_equal(H[0], H[3]) and e[0] == e[3]
    del bp
    nothing.insert(world.tgt[0])
    pbs, bp = build()
    H2, b2, e2, n2 = bp.linearize(st.factor, [T] * 4)
    # the filled map is the first map's twin (leaf 1 m, one offset) up to the order its insert added the points of a voxel up in
    assert abs(int(n2[2]) - int(n[0])) <= 2 and abs(e2[2] - e[0]) <= 1e-5 * abs(e[0]) and n2[2] > 100
    m2 = Map.__new__(Map)
    m2.tn, m2.rows = None, (lambda idx: idx)
    _, means, c6, _ = nothing.download()
    m2.tp = means.astype(np.float64)
    m2.tc = np.zeros((len(c6), 3, 3))
    m2.tc[:] = sga.api.mats_from_sym6(c6.astype(np.float64))
    check("after the insert", pbs[2], st, T, (H2[2], b2[2], e2[2], int(n2[2])), m2, s, "GICP", 1.0)
    del bp


def test_refusals(world):
    """Mixed kinds are refused at creation (UNSUPPORTED); a factor the members' maps cannot serve, fp64 and a robust kernel are refused by
    the call with the lone path's status; the member problems still work through the lone path afterwards."""
    lib = sga.load()
    T = world.T
    s = world.src[4]
    g = world.slots("gaussian", "GICP")[0][0]
    f = world.slots("flat", "ICP")[0][0]
    tree = sga.KdTree(world.tgt[0])
    pk, pg, pf = sga.Problem(tree, s.cloud), sga.Problem(g.m, s.cloud), sga.Problem(f.m, s.cloud)
    for members in ([pk, pg], [pg, pk], [pg, pf], [pf, pg]):
        with pytest.raises(sga.SgaError, match="error %d" % UNSUPPORTED):
            sga.BatchProblem(members)
    res = (sga._lib.ResultC * 2)()
    Ts = [T, T]
    # a Gaussian batch: PLANE_ICP, fp64, Huber
    pbs = [pg, sga.Problem(g.m, s.cloud)]
    bp = sga.BatchProblem(pbs)
    with pytest.raises(sga.SgaError, match="error %d: PLANE_ICP needs a kd-tree index over a target with normals" % UNSUPPORTED):
        bp.linearize(sga.make_setting("PLANE_ICP").factor, Ts)
    for kw in (dict(math_mode="fp64"), dict(robust_kernel="HUBER")):
        assert lib.sga_align_batch(bp.ctx.h, bp.h, None, C.byref(sga.make_setting("GICP", **kw)), res) == UNSUPPORTED
    st = sga.make_setting("GICP")
    got = bp.align(st, Ts)
    del bp
    for pb, r in zip(pbs, got):
        lone = pb.align(st, T)
        assert lone.num_inliers > 0 and abs(lone.iterations - r.iterations) <= 1 and pose_error(lone.T_target_source, r.T_target_source)[0] < 1e-3
    # a flat batch over points-only maps: GICP (no covariances) and PLANE_ICP (no normals)
    pbs = [pf, sga.Problem(f.m, s.cloud)]
    bp = sga.BatchProblem(pbs)
    with pytest.raises(sga.SgaError, match="error %d: GICP needs covariances on both source and target" % INVALID):
        bp.linearize(st.factor, Ts)
    with pytest.raises(sga.SgaError, match="error %d: PLANE_ICP needs a kd-tree index over a target with normals" % UNSUPPORTED):
        bp.linearize(sga.make_setting("PLANE_ICP").factor, Ts)
    sti = sga.make_setting("ICP")
    for kw in (dict(math_mode="fp64"), dict(robust_kernel="HUBER")):
        assert lib.sga_align_batch(bp.ctx.h, bp.h, None, C.byref(sga.make_setting("ICP", **kw)), res) == UNSUPPORTED
    H, b, e, n = bp.linearize(sti.factor, Ts)
    del bp
    for k, pb in enumerate(pbs):
        Hl, bl, el, nl = pb.linearize(sti.factor, T)
        assert nl == n[k] > 50 and abs(el - e[k]) <= 1e-5 * abs(el)

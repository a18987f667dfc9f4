"""Which voxel or stored point a source point is paired with when the target is a voxel map (csrc/voxel_hash.hpp: voxel_lookup, voxel_nearest,
flat_nearest, called from csrc/factor_stage.hpp; csrc/problem.hip: voxel_knn_kernel) against tests/map_search_ref.py, the float64
restatement that tests/test_map_search_ref.py pins to the oracle and to the compiled reference on the CPU.

The pairs come from Problem.linearize + Problem.factors(), the k-NN lists from batch_knn_search.  The restatement receives exactly what
the device holds: records fl32(x - origin) (origin read through sga_index_origin), queries in that frame, the frame's origin.

  1. each of the 27 offsets on its own, in all eight octants            4. the last voxel the 21-bit key holds, and the one beyond
  2. order and ties (dyadic coordinates)                                 5. hash tables around the sizes where they grow
  3. queries on, one fp32 ulp below and above voxel faces; the          6. a posed random scene, every family, pattern, arithmetic, rejector
     double query 2^-40 below a face whose fp32 rounding lies on it     7. k-NN lists

In the designed cases (1 - 5) and in fp64 arithmetic every pair equals the restatement's.  In fp32 arithmetic on the random scene the
device's query is the rounded one: test_map_search_ref.query_bounds derives how far it can lie from the double query (delta) and how
far a distance can be off (bound); a query within delta of a face, with a runner-up within bound, or within bound of the rejector's
reach is FLAGGED and may take any candidate map_search_ref.admissible() allows; every other query matches exactly.  At most 0.5 % of a
case's queries may be flagged in fp32 arithmetic, none in fp64.

Observed on the MI355X (printed with -s), 4 096 queries per case: the 48 fp64 cases of the scene flag no query; of the 48 fp32 cases four
flag ONE query each (Gaussian map, 0.3 m rejector: leaf 0.5 with 7 offsets, leaf 1.0 with 1, 7 and 27 offsets — a pair within the bound of
the rejector's reach) and 44 flag none; of the six batched members three flag one query each (Gaussian leaf 1.0 / 7 offsets and leaf
0.5 / 27 offsets, flat with normals leaf 1.0 / 1 offset).  No flagged query took another answer than the restatement's: 0 pairs differ,
so the worst observed error over its bound is 0.  No query of this seed lies within delta (at most 6.3e-6 m) of a face; about one in 4 096
is expected to.  With voxel_lookup still rounding the query to fp32 (before this file existed) test_double_query_below_a_face_in_fp64 failed
for one offset at all three leaves: voxels 2, 8, 20, 26 instead of 1, 7, 19, 25.
"""
import numpy as np
import pytest

import factor_ref as fr
import map_search_ref as ms
import small_gicp_amd as sga
import test_map_search_ref as cases
import test_route_matrix as rm
from small_gicp_amd import api

pytestmark = pytest.mark.gpu

KINDS = {"gaussian": (sga.GaussianVoxelMap, "GICP"), "flat": (sga.IncrementalVoxelMap, "ICP"), "flat_normal": (sga.IncrementalVoxelMapNormal, "PLANE_ICP"), "flat_cov": (sga.IncrementalVoxelMapCov, "GICP")}
COV6 = np.array([1e-2, 0, 0, 1e-2, 0, 1e-2])
DYADIC_T = np.array([0.25, -0.5, 2.0])


@pytest.fixture(autouse=True)
def restore_modes():
    yield
    sga.set_error_model(True)


# ---- what the device holds ---------------------------------------------------------------------------------------------------------------
def origin_of(m):
    o = np.zeros(3)
    api.check(sga.load().sga_index_origin(m.h, api._dp(o)))
    return o


def family_of(kind):
    return "gaussian" if kind == "gaussian" else "flat"


def map_from_case(case, kind, offsets):
    """the case's voxels through from_voxels (the double values go in: the library picks the frame)"""
    cls, _ = KINDS[kind]
    coords = case.coords.astype(np.int32)
    if kind == "gaussian":
        m = cls.from_voxels(case.leaf, coords, case.means(), np.tile(COV6, (len(coords), 1)))
        m.set_search_offsets(offsets)
        return m
    pts = case.points()
    if kind == "flat_cov":
        return cls.from_voxels(case.leaf, coords, case.counts(), pts, np.tile(COV6, (len(pts), 1)), search_offsets=offsets)
    normals = np.tile([0.0, 0.0, 1.0], (len(pts), 1)) if kind == "flat_normal" else None
    return cls.from_voxels(case.leaf, coords, case.counts(), pts, search_offsets=offsets, normals=normals)


def source_cloud(points):
    """a source with every attribute a factor may ask for; float64 points go in as they are (the library picks the frame)"""
    points = np.asarray(points)
    return sga.PointCloud(points, covs=np.tile(COV6, (len(points), 1)).astype(np.float32))


def device_queries(points, cloud, m, T):
    """(q (n, 3) float64 in the map's device frame, source records, R, t'): q = R fl32(p - o_s) + t' with t' = R o_s + t - o_t (pose_to_device),
    evaluated in double"""
    o_s, o_t = cloud.origin(), origin_of(m)
    p = (np.asarray(points, np.float64) - o_s).astype(np.float32).astype(np.float64)
    R = np.asarray(T, np.float64)[:3, :3]
    t = R @ o_s + np.asarray(T, np.float64)[:3, 3] - o_t
    return p @ R.T + t, p, R, t


def pairs(m, cloud, kind, T, mode, maxd=None):
    st = sga.make_setting(KINDS[kind][1], math_mode=mode, max_correspondence_distance=maxd)
    pb = sga.Problem(m, cloud)
    res = pb.linearize(st.factor, T)
    return pb.factors()[0], res, pb, st


def translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def check_designed(label, case, kind, offsets, mode, points=None, T=None):
    """the pairs of the case's queries (or of `points` under T) equal the restatement on the device's records AND the hand-written answer"""
    T = np.eye(4) if T is None else T
    points = case.queries if points is None else points
    m = map_from_case(case, kind, offsets)
    cloud = source_cloud(points)
    got, res, _, _ = pairs(m, cloud, kind, T, mode)
    q, _, _, _ = device_queries(points, cloud, m, T)
    org = origin_of(m)
    fam = family_of(kind)
    idx, _, _ = ms.nearest(case.coords, case.leaf, org, offsets, q, **case.contents(fam, org))
    assert np.array_equal(got, idx), (label, kind, offsets, mode, np.flatnonzero(got != idx)[:8], got[got != idx][:8], idx[got != idx][:8])
    if offsets in case.expect:
        want = case.expect[offsets][fam]
        assert np.array_equal(got, want), (label, kind, offsets, mode, np.flatnonzero(got != want)[:8])
    assert res[3] == (idx >= 0).sum() and np.array_equal(res[0], res[0].T)
    return got


MODES = ["fp32", "fp64"]
OFFSETS = [1, 7, 27]


# ---- 1. each offset on its own -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_each_offset_on_its_own(kind, offsets, mode):
    """216 sites, one occupied voxel at c + o each and one query in the middle of c: a pair exactly when o is in the pattern, and that voxel;
    at the identity and under a dyadic translation (exact in both arithmetics)"""
    case = cases.case_single_offsets()
    check_designed("single offsets", case, kind, offsets, mode)
    check_designed("single offsets, translated", case, kind, offsets, mode, points=case.queries - DYADIC_T, T=translation(DYADIC_T))


# ---- 2. order and ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", OFFSETS)
def test_order_and_ties(offsets):
    """equidistant means at +x and -x; the centre against an equidistant neighbour; two equidistant points in one voxel and in two; a voxel
    with 16 points; a voxel with none: both arithmetics give the hand-written answer"""
    g, f = cases.case_ties()
    got = {}
    for mode in MODES:
        got[mode] = (check_designed("ties", g, "gaussian", offsets, mode), check_designed("ties", f, "flat", offsets, mode))
        check_designed("ties, translated", f, "flat", offsets, mode, points=f.queries - DYADIC_T, T=translation(DYADIC_T))
    assert all(np.array_equal(a, b) for a, b in zip(got["fp32"], got["fp64"]))


# ---- 3. faces ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("leaf", cases.FACE_LEAVES)
def test_faces(leaf, offsets):
    """fp32 queries on a face, one ulp below and one above, +0.0 and -0.0, at the identity (the query is the fp32 value in both arithmetics)"""
    case = cases.case_faces(leaf, offsets)
    for kind in ("gaussian", "flat"):
        for mode in MODES:
            check_designed("faces", case, kind, offsets, mode, points=case.queries.astype(np.float32))


@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("leaf", [0.5, 1.0, 2.0])
def test_double_query_below_a_face_in_fp64(leaf, offsets):
    """fp64 arithmetic floors the DOUBLE query (incremental_voxelmap.hpp:100): 2^-40 below a face is the lower voxel, although the fp32
    rounding of the query lies on the face"""
    case, src, t = cases.case_cast(leaf, offsets)
    for kind in ("gaussian", "flat"):
        check_designed("cast", case, kind, offsets, "fp64", points=src, T=translation(t))


# ---- 4. the range edge ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", OFFSETS)
@pytest.mark.parametrize("sign", [1, -1])
def test_range_edge(sign, offsets):
    """float64 map and queries a million metres out (the device frame carries the offset): the last voxel of the key's range pairs; the
    voxel beyond offers nothing at the centre, and with 7 / 27 offsets finds the occupied voxel through the offset back"""
    case = cases.case_range_edge(sign)
    for kind in ("gaussian", "flat"):
        for mode in MODES:
            check_designed("range edge", case, kind, offsets, mode)
        m = map_from_case(case, kind, offsets)
        assert abs(origin_of(m)[0]) >= 1 << 19  # the frame does carry the offset


# ---- 5. table fill -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", cases.FILL_V)
def test_table_fill(V):
    """V voxels around the sizes where the hash table (at most half full) doubles; hits and misses that probe along clusters and across
    the table's end; 27 offsets; every distance exact in both arithmetics, ties common"""
    case = cases.case_table_fill(V)
    for kind in ("gaussian", "flat"):
        for mode in MODES:
            got = check_designed("table fill", case, kind, 27, mode)
        assert (got[:V] >= 0).all()  # a query inside an occupied voxel always has a pair


# ---- 6. a posed random scene ---------------------------------------------------------------------------------------------------------------
class Scene:
    pass


@pytest.fixture(scope="module")
def scene():
    s = Scene()
    target, source, s.T = cases.scene_clouds()
    s.tgt = sga.PointCloud(target)
    sga.estimate_normals_covariances(s.tgt, None, 10)
    s.points = source
    s.src = sga.PointCloud(source)
    sga.estimate_covariances(s.src, None, 10)
    s.sp, s.sc = s.src.xyz().astype(np.float64), s.src.covs()
    s.maps = {}
    s.restated = {}
    return s


def scene_map(s, kind, leaf):
    """(map, coords, restatement contents, rows of points / normals / covariances for factor_ref, factors() -> row): inserted once"""
    if (kind, leaf) not in s.maps:
        xyz, nrm, cov = s.tgt.xyz(), s.tgt.normals()[:, :3], s.tgt.covs()
        cloud = {"gaussian": lambda: sga.PointCloud(xyz, covs=cov), "flat": lambda: sga.PointCloud(xyz), "flat_normal": lambda: sga.PointCloud(xyz, normals=nrm), "flat_cov": lambda: sga.PointCloud(xyz, covs=cov)}[kind]()
        m = KINDS[kind][0](leaf)
        m.insert(cloud)
        assert not origin_of(m).any()
        tn = tc = None
        if kind == "gaussian":
            coords, means, c6, _ = m.download()
            kw, tp, rows = dict(means=means.astype(np.float64)), means.astype(np.float64), (lambda idx: idx)
            tc = np.zeros((len(c6), 3, 3))
            tc[:] = api.mats_from_sym6(c6.astype(np.float64))
        else:
            d = m.download()
            coords, counts, tp = d[0], d[1], d[2].astype(np.float64)
            kw, rows = cases.slots16(counts, tp), (lambda idx, c=counts: rm._slot_rows(idx, c))
            if kind == "flat_normal":
                tn = d[3].astype(np.float64)
            if kind == "flat_cov":
                tc = np.zeros((len(d[3]), 3, 3))
                tc[:] = api.mats_from_sym6(d[3].astype(np.float64))
        s.maps[(kind, leaf)] = (m, coords, kw, (tp, tn, tc), rows)
    return s.maps[(kind, leaf)]


def scene_restated(s, kind, leaf, offsets, T):
    key = (kind, leaf, offsets, np.asarray(T).tobytes())
    if key not in s.restated:
        m, coords, kw, _, _ = scene_map(s, kind, leaf)
        q, p, R, t = device_queries(s.points, s.src, m, T)
        s.restated[key] = (q, p, R, t) + ms.nearest(coords, leaf, np.zeros(3), offsets, q, **kw)
    return s.restated[key]


def compare_scene_pairs(label, s, kind, leaf, offsets, T, fp64, maxd, got, n):
    """the pairs and the inlier count against the restatement; -> (flagged, differing, worst (distance beyond the minimum) / bound)"""
    _, coords, kw, _, _ = scene_map(s, kind, leaf)
    q, p, R, t, idx, best, second = scene_restated(s, kind, leaf, offsets, T)
    max_sq = None if maxd is None else float(maxd) ** 2
    want = idx if max_sq is None else np.where(best <= max_sq, idx, -1)  # rejector.hpp: reject iff sq_dist > max_dist_sq
    delta, bound = cases.query_bounds(p, R, t, fp64)
    flagged, b = cases.flagged_queries(q, leaf, np.zeros(3), best, second, delta, bound, max_sq)
    assert flagged.sum() <= (0 if fp64 else cases.CAP_FP32 * len(q)), (label, int(flagged.sum()))
    clear = ~flagged
    bad = clear & (got != want)
    assert not bad.any(), (label, int(bad.sum()), np.flatnonzero(bad)[:8], got[bad][:8], want[bad][:8])
    differing, worst = 0, 0.0
    for i in np.flatnonzero(flagged):
        adm = ms.admissible(coords, leaf, np.zeros(3), offsets, q[i], delta[i], b[i], **kw)
        allowed = set()
        for cand, d2 in adm.items():
            if cand == -1:
                allowed.add(-1)
                continue
            if max_sq is None or np.sqrt(d2) <= np.sqrt(max_sq) + b[i]:
                allowed.add(cand)
            if max_sq is not None and np.sqrt(d2) >= np.sqrt(max_sq) - b[i]:
                allowed.add(-1)
        assert int(got[i]) in allowed, (label, int(i), int(got[i]), int(want[i]), sorted(allowed))
        if got[i] != want[i]:
            differing += 1
            if got[i] >= 0 and want[i] >= 0:
                worst = max(worst, (np.sqrt(adm[int(got[i])]) - np.sqrt(best[i])) / b[i])
    assert n == (got >= 0).sum() and abs(int(n) - int((want >= 0).sum())) <= differing, (label, n, int((got >= 0).sum()), int((want >= 0).sum()))
    return int(flagged.sum()), differing, worst


@pytest.mark.parametrize("leaf", cases.SCENE_LEAVES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_posed_scene(scene, kind, leaf):
    """a map inserted from 8 192 points, 4 096 source points under a rotation of 3 degrees and a translation of 3 m: the pairs, the inlier
    count, H symmetric and the sums over the GPU's own pairs (tests/factor_ref.py through test_route_matrix.check_pass), for 1 / 7 / 27
    offsets, both arithmetics, without a rejector and with 0.3 m"""
    s = scene
    m, _, _, (tp, tn, tc), rows = scene_map(s, kind, leaf)
    factor = KINDS[kind][1]
    for offsets in OFFSETS:
        m.set_search_offsets(offsets)
        for mode in MODES:
            for maxd in cases.SCENE_MAXD:
                label = "scene %s leaf %.1f offsets %d %s maxd %s" % (kind, leaf, offsets, mode, maxd)
                got, res, pb, st = pairs(m, s.src, kind, s.T, mode, maxd)
                flagged, differing, worst = compare_scene_pairs(label, s, kind, leaf, offsets, s.T, mode == "fp64", maxd, got, res[3])
                assert (got >= 0).sum() > 0.2 * len(got), label
                print("%-58s pairs %4d  flagged %d  differing %d  worst error / bound %.2f" % (label, (got >= 0).sum(), flagged, differing, worst))

                class Mapped:
                    def factors(self):
                        c, mm = pb.factors()
                        return rows(c), mm

                    def error(self, f, Tq):
                        return pb.error(f, Tq)

                rm.check_pass(label, Mapped(), st, s.T, res, tp, tn, tc, s.sp, s.sc, mode == "fp64", factor, None, None, np.inf if maxd is None else float(maxd) ** 2)
    m.set_search_offsets(1)


def clone(s, kind, leaf, offsets):
    """the scene's map again through from_voxels, with search offsets of its own (a batch may hold one map under one pattern only)"""
    m, coords, _, (tp, tn, tc), _ = scene_map(s, kind, leaf)
    if kind == "gaussian":
        _, means, c6, _ = m.download()
        c = sga.GaussianVoxelMap.from_voxels(leaf, coords, means, c6)
        c.set_search_offsets(offsets)
        return c
    d = m.download()
    if kind == "flat_cov":
        return KINDS[kind][0].from_voxels(leaf, d[0], d[1], d[2], d[3], search_offsets=offsets)
    return KINDS[kind][0].from_voxels(leaf, d[0], d[1], d[2], search_offsets=offsets, normals=d[3] if kind == "flat_normal" else None)


@pytest.mark.parametrize("family", ["gaussian", "flat"])
def test_posed_scene_batched(scene, family):
    """one BatchProblem of three members (different kinds or leaves, 1 / 7 / 27 offsets, a pose each): every member's pairs equal the restatement"""
    s = scene
    if family == "gaussian":
        members, factor = [("gaussian", 0.5, 1), ("gaussian", 1.0, 7), ("gaussian", 0.5, 27)], "GICP"
    else:
        members, factor = [("flat", 0.5, 27), ("flat_normal", 1.0, 1), ("flat_cov", 0.5, 7)], "ICP"
    Ts = [s.T, rm.step(s.T, 0.05), rm.step(s.T, -0.08)]
    maps = [clone(s, kind, leaf, offsets) for kind, leaf, offsets in members]
    problems = [sga.Problem(m, s.src) for m in maps]
    bp = sga.BatchProblem(problems)
    st = sga.make_setting(factor, max_correspondence_distance=0.3)
    H, b, e, n = bp.linearize(st.factor, Ts)
    for k, (kind, leaf, offsets) in enumerate(members):
        label = "batched %s leaf %.1f offsets %d" % (kind, leaf, offsets)
        got = problems[k].factors()[0]
        flagged, differing, worst = compare_scene_pairs(label, s, kind, leaf, offsets, Ts[k], False, 0.3, got, int(n[k]))
        assert np.array_equal(H[k], H[k].T) and (got >= 0).sum() > 0.2 * len(got), label
        print("%-58s pairs %4d  flagged %d  differing %d  worst error / bound %.2f" % (label, (got >= 0).sum(), flagged, differing, worst))
    del bp


# ---- 7. k-NN ---------------------------------------------------------------------------------------------------------------------------------
def check_knn(label, m, coords, leaf, kw, queries, offsets, cut):
    org = origin_of(m)
    qf = (np.asarray(queries, np.float64) - org).astype(np.float32).astype(np.float64)  # the search runs on the fp32 query of the device frame
    m.set_search_offsets(offsets)
    full = part = False
    for k in (1, 2, 10, 40):
        for max_sq in (None, cut):
            gi, gd = m.batch_knn_search(np.asarray(queries, np.float64), k, -1.0 if max_sq is None else max_sq)
            wi, wd = ms.knn(coords, leaf, org, offsets, qf, k, max_sq, **kw)
            assert gi.shape == wi.shape == (len(qf), k)
            assert np.array_equal(gi, wi), (label, offsets, k, max_sq, np.flatnonzero((gi != wi).any(1))[:8])
            fin = np.isfinite(wd)
            assert np.array_equal(np.isfinite(gd), fin) and (np.abs(gd[fin] - wd[fin]) <= np.spacing(wd[fin].astype(np.float32))).all(), (label, offsets, k, max_sq)
            full, part = full or bool((wi[:, -1] >= 0).any()), part or bool((wi[:, -1] < 0).any())
    assert full and part, label  # full lists and lists with unused slots both occur


@pytest.mark.parametrize("offsets", OFFSETS)
def test_knn_designed(offsets):
    """the tie scenes and two filled tables: k = 1, 2, 10, 40 (more than there are candidates), with and without a cut, a query with no voxel
    in reach; 27 offsets visit the centre twice"""
    far = np.array([[500.5, 0.5, 0.5]])
    g, f = cases.case_ties()
    for case, kind in ((g, "gaussian"), (f, "flat")):
        m = map_from_case(case, kind, offsets)
        check_knn("ties", m, case.coords, case.leaf, case.contents(family_of(kind)), np.concatenate([case.queries, far]), offsets, 0.0625)
    for V in (129, 2049):
        case = cases.case_table_fill(V)
        for kind in ("gaussian", "flat"):
            m = map_from_case(case, kind, offsets)
            check_knn("fill %d" % V, m, case.coords, case.leaf, case.contents(family_of(kind)), np.concatenate([case.queries[::max(1, V // 100)], far]), offsets, 0.75)


@pytest.mark.parametrize("kind", ["gaussian", "flat"])
def test_knn_scene(scene, kind):
    """the scene's maps at leaf 0.5: 300 posed source points and a query far outside, 27 offsets (the duplicated centre) and 7"""
    s = scene
    m, coords, kw, _, _ = scene_map(s, kind, 0.5)
    q = np.concatenate([fr.transform(s.T, s.points[::14].astype(np.float64)), [[400.0, 3.0, 1.0]]])
    try:
        for offsets in (27, 7):
            check_knn("scene", m, coords, 0.5, kw, q, offsets, 0.04)
    finally:
        m.set_search_offsets(1)

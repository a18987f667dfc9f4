"""tests/map_search_ref.py (the voxel-map searches restated in numpy, float64) pinned on the CPU:

  * against the oracle: the correspondences of orc.linearize over orc.VoxelMap and orc.FlatMap on the C1 clouds, for 1 / 7 / 27 search
    offsets at the identity and at a pose, equal nearest() on the oracle's own double map contents for every point;
  * against the compiled reference where it is there: FlatMap.knn and VoxelMap.knn for k = 1, 6, 40 equal knn();
  * the designed cases of tests/test_map_search_gpu.py (built here, shared with it) give the answers written out by hand;
  * the random scene of that file stays under its cap of ambiguous queries by the restatement and its bounds alone.
"""
import math

import numpy as np
import pytest

import map_search_ref as ms

EPS32, EPS64 = 2.0 ** -24, 2.0 ** -53
CAP_FP32 = 0.005  # share of a case's queries that may be flagged ambiguous in fp32 arithmetic; none in fp64


# ---- maps and designed cases (shared with tests/test_map_search_gpu.py) ----------------------------------------------------------------
class Case:
    """voxels: [(coordinate (3,), [point, ...])] in voxel-id order; queries (n, 3) float64; expect {offsets: {family: (n,) int64}}"""

    def __init__(self, leaf, voxels, queries, expect):
        self.leaf = float(leaf)
        self.coords = np.array([c for c, _ in voxels], np.int64).reshape(-1, 3)
        self.lists = [np.asarray(p, np.float64).reshape(-1, 3) for _, p in voxels]
        self.queries = np.asarray(queries, np.float64).reshape(-1, 3)
        self.expect = expect

    def means(self):
        assert all(len(p) == 1 for p in self.lists)
        return np.concatenate(self.lists) if self.lists else np.zeros((0, 3))

    def counts(self):
        return np.array([len(p) for p in self.lists], np.uint32)

    def points(self):
        """(P, 3): the points of voxel 0 first, then voxel 1, ... (from_voxels' layout)"""
        return np.concatenate(self.lists) if self.lists else np.zeros((0, 3))

    def contents(self, family, origin=(0.0, 0.0, 0.0)):
        """the keyword arguments of nearest() / knn() for records held as fl32(x - origin)"""
        o = np.asarray(origin, np.float64)
        if family == "gaussian":
            return dict(means=(self.means() - o).astype(np.float32).astype(np.float64))
        return dict(**slots16(self.counts(), (self.points() - o).astype(np.float32).astype(np.float64)))


def slots16(counts, points):
    counts = np.asarray(counts, np.int64)
    p16 = np.zeros((len(counts), ms.CAP, 3))
    p16[np.arange(ms.CAP)[None, :] < counts[:, None]] = np.asarray(points, np.float64).reshape(-1, 3)
    return dict(points=p16, counts=counts)


def flat_id(voxel, slot=0):
    return (int(voxel) << 32) | int(slot)


def in_pattern(o, offsets):
    """written out, not read from the restatement's table: 1 = the centre, 7 = the centre and its six face neighbours, 27 = the cube"""
    return {1: o == (0, 0, 0), 7: abs(o[0]) + abs(o[1]) + abs(o[2]) <= 1, 27: max(abs(o[0]), abs(o[1]), abs(o[2])) <= 1}[offsets]


def case_single_offsets(leaf=1.0):
    """27 sites in each of the eight octants (216 sites, any two at least six voxels apart on some axis): site o has ONE occupied voxel, at
    c + o, and one query in the middle of voxel c.  The centres on the x axis include 0 (whose -x neighbour is voxel -1), those on the y
    and z axes -1 (whose + neighbour is voxel 0): the sites straddle the sign change on every axis.  The query has a pair exactly when o
    is in the pattern."""
    cube = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    pos, neg = [(0, 6, 12), (5, 11, 17), (5, 11, 17)], [(-7, -13, -19), (-1, -7, -13), (-1, -7, -13)]
    voxels, queries, sites = [], [], []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                for n, o in enumerate(cube):
                    digit = (n % 3, (n // 3) % 3, n // 9)
                    c = tuple((pos if s > 0 else neg)[a][digit[a]] for a, s in enumerate((sx, sy, sz)))
                    v = tuple(c[a] + o[a] for a in range(3))
                    voxels.append((v, [[(v[a] + 0.5) * leaf for a in range(3)]]))
                    queries.append([(c[a] + 0.5) * leaf for a in range(3)])
                    sites.append(o)
    expect = {}
    for offsets in (1, 7, 27):
        hit = np.array([in_pattern(o, offsets) for o in sites])
        ids = np.arange(len(sites), dtype=np.int64)
        expect[offsets] = {"gaussian": np.where(hit, ids, -1), "flat": np.where(hit, ids << 32, -1)}
    return Case(leaf, voxels, queries, expect)


def case_ties():
    """Dyadic coordinates, leaf 1, scenes eight voxels apart along x.  Voxel ids in the order written.
      a  voxel 0 at (1,0,0) and voxel 1 at (-1,0,0), both 0.75 from the query in the empty (0,0,0): 7 offsets meet +x first, 27 meet
         (-1,0,0) first, one offset meets neither;
      b  voxel 2 = the query's own (8,0,0) and voxel 3 = (8,0,-1), both 0.25 away: the centre is visited first under every pattern;
      (flat only)
      c  voxel 4 (16,0,0) holds two points 0.25 either side of the query: the lower slot;
      d  voxel 5 (24,0,0) holds 16 points, the query nearest the last;
      e  voxel 6 (32,0,0) holds no point, voxel 7 (33,0,0) one: no pair with one offset, voxel 7 with 7 and 27."""
    voxels = [((1, 0, 0), [[1.25, 0.5, 0.5]]), ((-1, 0, 0), [[-0.25, 0.5, 0.5]]), ((8, 0, 0), [[8.5, 0.5, 0.375]]), ((8, 0, -1), [[8.5, 0.5, -0.125]])]
    queries = [[0.5, 0.5, 0.5], [8.5, 0.5, 0.125]]
    g = Case(1.0, voxels, queries, {1: {"gaussian": np.array([-1, 2])}, 7: {"gaussian": np.array([0, 2])}, 27: {"gaussian": np.array([1, 2])}})
    voxels = voxels + [((16, 0, 0), [[16.25, 0.5, 0.5], [16.75, 0.5, 0.5]]), ((24, 0, 0), [[24 + i / 16 + 1 / 32, 0.5, 0.5] for i in range(16)]), ((32, 0, 0), []),
                       ((33, 0, 0), [[33.25, 0.5, 0.5]])]
    queries = queries + [[16.5, 0.5, 0.5], [24 + 15 / 16 + 1 / 32, 0.5, 0.75], [32.5, 0.5, 0.5]]
    f = Case(1.0, voxels, queries, {
        1: {"flat": np.array([-1, flat_id(2), flat_id(4, 0), flat_id(5, 15), -1])},
        7: {"flat": np.array([flat_id(0), flat_id(2), flat_id(4, 0), flat_id(5, 15), flat_id(7)])},
        27: {"flat": np.array([flat_id(1), flat_id(2), flat_id(4, 0), flat_id(5, 15), flat_id(7)])},
    })
    return g, f


FACE_LEAVES = [0.1, 0.3, 0.5, 1.0, 2.0]
FACE_K = [-12, -6, 0, 6, 12]


def scalar_voxel(x, leaf):
    """floor(x * (1 / leaf)) in Python's own double arithmetic (no numpy, no truncation trick)"""
    return math.floor(float(x) * (1.0 / float(leaf)))


def case_faces(leaf, offsets):
    """Queries on the faces k * leaf (as fp32 values), one fp32 ulp below and one above, and at +0.0 / -0.0; y and z in the middle of voxel 0.
    The occupied voxels tell the query's voxel c apart.  One offset: the row x = -14 .. 14 is occupied, the pair is c.  7 / 27 offsets: for a
    face k only k - 2 and k + 1 are occupied, so c = k pairs with k + 1 (through +x) and c = k - 1 with k - 2 (through -x)."""
    mid = 0.5 * leaf
    xs = []
    for k in FACE_K:
        f = np.float32(k * leaf)
        xs += [(k, f), (k, np.nextafter(f, np.float32(-np.inf))), (k, np.nextafter(f, np.float32(np.inf)))]
    xs += [(0, np.float32(0.0)), (0, np.float32(-0.0))]
    row = list(range(-14, 15)) if offsets == 1 else sorted({k - 2 for k in FACE_K} | {k + 1 for k in FACE_K})
    voxels = [((x, 0, 0), [[(x + 0.5) * leaf, mid, mid]]) for x in row]
    queries = [[float(x), mid, mid] for _, x in xs]
    want = []
    for k, x in xs:
        c = scalar_voxel(x, leaf)
        assert c in (k - 1, k), (leaf, k, x, c)
        if leaf in (0.5, 1.0, 2.0):  # dyadic leaves: by hand, the face and above belong to k, below to k - 1
            assert c == (k if float(x) >= k * leaf else k - 1)
        want.append(row.index(c if offsets == 1 else (k + 1 if c == k else k - 2)))
    ids = np.array(want, np.int64)
    return Case(leaf, voxels, queries, {offsets: {"gaussian": ids, "flat": ids << 32}})


CAST_SHIFT = 0.25 - 2.0 ** -40


def case_cast(leaf, offsets):
    """(dyadic leaves) source points 0.25 below a face under the translation 0.25 - 2^-40 along x: the double query lies 2^-40 below the face
    (voxel k - 1), its fp32 rounding on it (voxel k).  -> (case over the QUERIES in double, source points, translation)"""
    faces = case_faces(leaf, offsets)
    row = [int(c[0]) for c in faces.coords]
    ks = [k for k in FACE_K if k != 0]  # (2^-40 below zero is an fp32 value of its own)
    src = np.array([[k * leaf - 0.25, 0.5 * leaf, 0.5 * leaf] for k in ks])
    t = np.array([CAST_SHIFT, 0.0, 0.0])
    q = src + t
    assert (q[:, 0] < np.array(ks) * leaf).all() and (q[:, 0].astype(np.float32) == (np.array(ks) * leaf).astype(np.float32)).all()
    ids = np.array([row.index(k - 1 if offsets == 1 else k - 2) for k in ks], np.int64)
    voxels = [(tuple(c), p) for c, p in zip(faces.coords, faces.lists)]
    return Case(leaf, voxels, q, {offsets: {"gaussian": ids, "flat": ids << 32}}), src, t


EDGE = (1 << 20) - 1


def case_range_edge(sign):
    """leaf 1, one occupied voxel at cx = sign * (2^20 - 1), the last the 21-bit key holds.  Queries in it, in its inner neighbour and in
    cx = sign * 2^20, which is out of range: with one offset that query has no pair; with 7 or 27 the centre offers nothing and the
    offset back towards the origin offers the occupied voxel."""
    cx = sign * EDGE
    voxels = [((cx, 0, 0), [[cx + 0.5, 0.5, 0.5]])]
    queries = [[cx + 0.5, 0.5, 0.5], [cx - sign + 0.5, 0.5, 0.5], [cx + sign + 0.5, 0.5, 0.5]]
    assert [scalar_voxel(q[0], 1.0) for q in queries] == [cx, cx - sign, sign * (1 << 20)]
    one, wide = np.array([0, -1, -1], np.int64), np.array([0, 0, 0], np.int64)
    return Case(1.0, voxels, queries, {1: {"gaussian": one, "flat": np.where(one >= 0, one << 32, -1)}, 7: {"gaussian": wide, "flat": wide << 32}, 27: {"gaussian": wide, "flat": wide << 32}})


FILL_V = [1, 2, 3, 127, 128, 129, 2047, 2048, 2049]


def case_table_fill(V, seed=11):
    """V random distinct voxels (leaf 1) with one point each on a 1/16 grid, one query per occupied voxel and as many in voxels next to
    occupied ones (most of them empty), all on the 1/16 grid shifted by 1/32: every squared distance is a small multiple of 2^-10, exact
    in fp32 and in fp64, and exact ties are common.  No hand-written answers: the restatement is the expectation."""
    rng = np.random.default_rng(seed + V)
    side = max(4, int(round((4 * V) ** (1 / 3))))  # about a quarter of the box is occupied: clusters in space, and so along no probe run in particular
    cells = rng.choice((2 * side) ** 3, V, replace=False)
    coords = np.stack([cells % (2 * side), (cells // (2 * side)) % (2 * side), cells // (2 * side) ** 2], 1) - side
    pts = coords + rng.integers(0, 16, (V, 3)) / 16.0
    near = coords + rng.integers(-1, 2, (V, 3))
    qv = np.concatenate([coords, near])
    queries = qv + rng.integers(0, 16, (2 * V, 3)) / 16.0 + 1 / 32
    return Case(1.0, [(tuple(c), [p]) for c, p in zip(coords, pts)], queries, {})


def restate(case, family, offsets, queries=None, origin=(0.0, 0.0, 0.0)):
    q = case.queries if queries is None else queries
    return ms.nearest(case.coords, case.leaf, origin, offsets, np.asarray(q, np.float64) - np.asarray(origin, np.float64), **case.contents(family, origin))


# ---- the random scene of case 6 ------------------------------------------------------------------------------------------------------
SCENE_SEED = 20
SCENE_LEAVES = [0.5, 1.0]
SCENE_MAXD = [None, 0.3]


def scene_pose():
    """a rotation of 3 degrees about (0.2, -0.3, 1) and a translation of a few metres"""
    k = np.array([0.2, -0.3, 1.0]) / np.linalg.norm([0.2, -0.3, 1.0])
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    a = np.deg2rad(3.0)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    T[:3, 3] = [2.5, -1.5, 0.4]
    return T


def scene_clouds(seed=SCENE_SEED):
    """(target (8192, 3) float32, source (4096, 3) float32, T): a rolling ground and two walls, 30 m across; the source is every other target
    point, 5 cm of noise added, seen from the pose T (so T source lies on the target)"""
    rng = np.random.default_rng(seed)
    n = 8192
    xy = rng.uniform(-15, 15, (n, 2))
    ground = np.stack([xy[:, 0], xy[:, 1], 0.3 * np.sin(0.4 * xy[:, 0]) + 0.2 * np.cos(0.3 * xy[:, 1])], 1)
    u, h = rng.uniform(-15, 15, n), rng.uniform(0, 4, n)
    wall_a = np.stack([u, np.full(n, 9.0) + 0.05 * np.sin(u), h], 1)
    wall_b = np.stack([np.full(n, -11.0) + 0.05 * np.cos(u), u, h], 1)
    pick = rng.integers(0, 4, n)
    target = np.where((pick <= 1)[:, None], ground, np.where((pick == 2)[:, None], wall_a, wall_b)) + rng.normal(0, 0.01, (n, 3))
    target = target.astype(np.float32)
    T = scene_pose()
    world = target[::2].astype(np.float64) + rng.normal(0, 0.05, (n // 2, 3))
    Ti = np.linalg.inv(T)
    source = (world @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return target, source, T


def query_bounds(src_dev, R, t, fp64):
    """The device forms q = R p + t by three fused multiply-adds per axis from the pose rounded to its arithmetic: the entries of R and t
    are off by u each (fp32; exact in fp64), every fma rounds once, so per axis |q_dev - q| <= (1 + 3) u (sum_j |R_ij| |p_j| + |t_i|) to
    first order; 5 u covers the second order.  delta (n,) = that bound over the three axes.  A distance measured from the moved query
    in the device's arithmetic (a subtraction, three products, two sums: 4 u relative on d2, 2 u on d) is off by at most
    sqrt(3) delta + 2 u d; two candidates may change places when their distances differ by less than twice that: bound(d)."""
    u = EPS64 if fp64 else EPS32
    a = np.abs(np.asarray(src_dev, np.float64)) @ np.abs(R).T + np.abs(t)
    delta = 5 * u * a.max(1)

    def bound(d):
        return 2 * (np.sqrt(3.0) * delta + 2 * u * np.asarray(d, np.float64))

    return delta, bound


def flagged_queries(q, leaf, org, best, second, delta, bound, max_sq):
    """the queries whose pair or inlier verdict the bounds leave open: near a face, near a tie, or near the rejector's threshold"""
    far = np.sqrt(np.where(np.isfinite(second), second, np.where(np.isfinite(best), best, 0.0)))
    b = bound(far)
    near_face, near_tie = ms.ambiguous(q, leaf, org, delta, best, second, b)
    near_cut = np.zeros(len(q), bool)
    if max_sq is not None and np.isfinite(max_sq):
        near_cut = np.isfinite(best) & (np.abs(np.sqrt(best) - np.sqrt(max_sq)) <= b)
    return near_face | near_tie | near_cut, b


# ---- the restatement against the oracle -------------------------------------------------------------------------------------------------
def parity_pose():
    from scipy.spatial.transform import Rotation

    T = np.eye(4)  # the second pose of tests/test_gpu_parity.py::test_gaussian_voxelmap_searched_over_7_and_27_voxels
    T[:3, :3] = Rotation.from_rotvec(np.array([0.1, 0.2, 1.0]) / np.linalg.norm([0.1, 0.2, 1.0]) * np.deg2rad(0.7)).as_matrix()
    T[:3, 3] = [0.49, 0.12, -0.02]
    return T


@pytest.fixture(scope="module")
def oracle_maps(orc, c1_f32):
    d = c1_f32
    ot = orc.Cloud(d["tp"], d["tn"], d["tc"])
    os_ = orc.Cloud(d["sp"], d["sn"], d["sc"], tree=False)
    vm = orc.VoxelMap(ot, 1.0)
    fm = orc.FlatMap(1.0)
    fm.insert(ot)
    return ot, os_, vm, fm


@pytest.mark.parametrize("pose", ["identity", "posed"])
@pytest.mark.parametrize("offsets", [1, 7, 27])
@pytest.mark.parametrize("family", ["gaussian", "flat"])
def test_nearest_equals_the_oracle(orc, c1_f32, oracle_maps, family, offsets, pose):
    """every correspondence of orc.linearize over a voxel map equals nearest() on the oracle's own double contents; no tolerance"""
    _, os_, vm, fm = oracle_maps
    T = np.eye(4) if pose == "identity" else parity_pose()
    q = c1_f32["sp"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    m = vm if family == "gaussian" else fm
    m.set_search_offsets(offsets)
    try:
        f = orc.Factors(len(os_))
        st = orc.default_setting(factor_kind=orc.GICP, num_threads=1)
        _, _, _, n = orc.linearize(m, os_, st, T, f)
        if family == "gaussian":
            coords, means, _, _ = m.get()
            idx, best, _ = ms.nearest(coords, 1.0, np.zeros(3), offsets, q, means=means)
            got = f.get(is_voxelmap=True)[0]
        else:
            coords, counts, pts, _ = m.get()
            idx, best, _ = ms.nearest(coords, 1.0, np.zeros(3), offsets, q, **slots16(counts, pts))
            got = f.get(2)[0]
    finally:
        m.set_search_offsets(1)
    want = np.where(best <= st.max_dist_sq, idx, -1)
    assert (want >= 0).sum() > 0.5 * len(q) and (want < 0).any()  # both verdicts occur
    assert n == (want >= 0).sum() and np.array_equal(got, want), (n, (want >= 0).sum(), np.flatnonzero(got != want)[:8])


@pytest.mark.parametrize("offsets", [1, 7, 27])
def test_knn_equals_the_compiled_reference(c1_f32, offsets):
    """FlatMap.knn (1 / 7 / 27 offsets) and VoxelMap.knn (its own voxel) of the compiled reference for k = 1, 6, 40 equal knn() in float64 on
    the same contents: indices and distances, the unused slots included"""
    from oracle import ref

    if not ref.available():
        pytest.skip("oracle/_ref is not built here")
    d = c1_f32
    rt = ref.Cloud(d["tp"], d["tn"], d["tc"], tree=False)
    rf, rg = ref.FlatMap(1.0), ref.VoxelMap(1.0)
    rf.set_search_offsets(offsets)
    rf.insert(rt)
    rg.insert(rt)
    rng = np.random.default_rng(5)
    q = np.concatenate([d["sp"][rng.choice(len(d["sp"]), 500, replace=False)].astype(np.float64) + rng.normal(0, 0.05, (500, 3)), rng.uniform(-60, 60, (100, 3))])
    coords, counts, pts, _ = rf.get()
    gcoords, means, _, _ = rg.get()
    for k in (1, 6, 40):
        cases = [(rf, dict(coords=coords, offsets=offsets, **slots16(counts, pts)))]
        if offsets == 1:
            cases.append((rg, dict(coords=gcoords, offsets=1, means=means)))
        for r, kw in cases:
            ri, rd = r.knn(q, k)
            ri = ri.astype(np.int64)
            none = rd >= np.finfo(np.float64).max  # the reference leaves max() and its own "invalid" in the unused slots
            wi, wd = ms.knn(kw.pop("coords"), 1.0, np.zeros(3), kw.pop("offsets"), q, k, dtype=np.float64, **kw)
            assert np.array_equal(none, wi < 0) and (~none[:, 0]).sum() > 0.5 * len(q)
            assert np.array_equal(np.where(none, -1, ri), wi) and np.array_equal(np.where(none, np.inf, rd), wd), (k, np.flatnonzero((np.where(none, -1, ri) != wi).any(1))[:8])


# ---- the designed cases through the restatement alone ------------------------------------------------------------------------------------
def check_expected(case, offsets, label):
    for family, want in case.expect[offsets].items():
        idx, _, _ = restate(case, family, offsets)
        assert np.array_equal(idx, want), (label, family, offsets, np.flatnonzero(idx != want)[:8], idx[idx != want][:8], want[idx != want][:8])


@pytest.mark.parametrize("offsets", [1, 7, 27])
def test_designed_single_offsets(offsets):
    case = case_single_offsets()
    assert len(case.queries) == 216 and (case.expect[offsets]["gaussian"] >= 0).sum() == 8 * offsets
    check_expected(case, offsets, "single offsets")


@pytest.mark.parametrize("offsets", [1, 7, 27])
def test_designed_ties(offsets):
    for case in case_ties():
        check_expected(case, offsets, "ties")


@pytest.mark.parametrize("offsets", [1, 7, 27])
@pytest.mark.parametrize("leaf", FACE_LEAVES)
def test_designed_faces(leaf, offsets):
    check_expected(case_faces(leaf, offsets), offsets, "faces")
    if leaf in (0.5, 1.0, 2.0):
        case, _, _ = case_cast(leaf, offsets)
        check_expected(case, offsets, "cast")
        # the fp32 rounding of the same queries lies ON the faces: the upper voxel
        up, _, _ = restate(case, "gaussian", offsets, queries=case.queries.astype(np.float32).astype(np.float64))
        assert (up != case.expect[offsets]["gaussian"]).all()


@pytest.mark.parametrize("offsets", [1, 7, 27])
@pytest.mark.parametrize("sign", [1, -1])
def test_designed_range_edge(sign, offsets):
    case = case_range_edge(sign)
    check_expected(case, offsets, "range edge")
    origin = np.array([sign * 1048576.0, 0.0, 0.0])  # in a shifted frame, as the device holds it
    for family, want in case.expect[offsets].items():
        assert np.array_equal(restate(case, family, offsets, origin=origin)[0], want)


def test_fast_floor_and_knn_rules():
    x = np.array([-2.0, -1.5, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 1.5, -1e-300, np.nextafter(1.0, 0.0)])
    assert ms.fast_floor(x).tolist() == [-2, -2, -1, -1, 0, 0, 0, 1, 1, -1, 0]
    # k-NN by hand on the flat tie scene: the query between the two points of voxel 4, 27 offsets -> the centre is visited twice
    _, f = case_ties()
    kw = f.contents("flat")
    q = f.queries[2:3]
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 27, q, 5, **kw)
    assert i[0].tolist() == [flat_id(4, 0), flat_id(4, 1), flat_id(4, 0), flat_id(4, 1), -1] and d[0].tolist() == [0.0625] * 4 + [np.inf]
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 27, q, 2, **kw)
    assert i[0].tolist() == [flat_id(4, 0), flat_id(4, 1)]  # as far as the worst: dropped
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 7, q, 3, **kw)
    assert i[0].tolist() == [flat_id(4, 0), flat_id(4, 1), -1]
    # sorted insertion, the cut, more k than candidates: the 16-point voxel from one end
    q = np.array([[24.0, 0.5, 0.5]])
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 1, q, 40, **kw)
    assert i[0, :16].tolist() == [flat_id(5, s) for s in range(16)] and (i[0, 16:] == -1).all() and np.isinf(d[0, 16:]).all()
    assert d[0, :16].tolist() == [(s / 16 + 1 / 32) ** 2 for s in range(16)]
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 1, q, 10, max_sq=(3 / 16 + 1 / 32) ** 2, **kw)
    assert i[0].tolist() == [flat_id(5, s) for s in range(4)] + [-1] * 6  # a distance equal to the cut is kept, the next is not
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 1, np.array([[24.999, 0.5, 0.5]]), 2, **kw)
    assert i[0].tolist() == [flat_id(5, 15), flat_id(5, 14)]
    i, d = ms.knn(f.coords, 1.0, np.zeros(3), 27, np.array([[100.5, 0.5, 0.5]]), 3, **kw)
    assert (i == -1).all() and np.isinf(d).all()


# ---- the cap of the random scene ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("leaf", SCENE_LEAVES)
def test_scene_stays_under_the_cap(orc, leaf):
    """By the restatement and its bounds alone (maps of the oracle over the same cloud stand in for the device's): the share of queries the
    fp32 bounds leave open is at most CAP_FP32 for every family, pattern and rejector, and the fp64 bounds leave none open."""
    target, source, T = scene_clouds()
    cov = np.tile(np.eye(3) * 1e-2, (len(target), 1, 1))
    ot = orc.Cloud(target.astype(np.float64), None, cov)
    vm = orc.VoxelMap(ot, leaf)
    fm = orc.FlatMap(leaf)
    fm.insert(ot)
    src = source.astype(np.float64)
    q = src @ T[:3, :3].T + T[:3, 3]
    coords, means, _, _ = vm.get()
    fcoords, counts, pts, _ = fm.get()
    maps = {"gaussian": (coords, dict(means=means)), "flat": (fcoords, slots16(counts, pts))}
    paired = 0
    for family, (c, kw) in maps.items():
        for offsets in (1, 7, 27):
            idx, best, second = ms.nearest(c, leaf, np.zeros(3), offsets, q, **kw)
            paired += (idx >= 0).sum()
            for maxd in SCENE_MAXD:
                max_sq = None if maxd is None else float(maxd) ** 2
                for fp64 in (False, True):
                    delta, bound = query_bounds(src, T[:3, :3], T[:3, 3], fp64)
                    flagged, _ = flagged_queries(q, leaf, np.zeros(3), best, second, delta, bound, max_sq)
                    share = flagged.mean()
                    if flagged.any():
                        print("leaf %.1f %-8s offsets %2d maxd %s %s: %d of %d flagged" % (leaf, family, offsets, maxd, "fp64" if fp64 else "fp32", flagged.sum(), len(q)))
                    assert share == 0 if fp64 else share <= CAP_FP32, (family, offsets, maxd, fp64, flagged.sum())
    assert paired > 3 * len(q)  # the scene does meet the maps

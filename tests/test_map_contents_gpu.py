"""What a voxel map holds after every insert (csrc/voxelmap.hip, csrc/voxelmap_build.hip; the shared steps of csrc/voxel_steps.hpp) against
tests/map_contents_ref.py, the float64 restatement that tests/test_map_contents_ref.py pins to the oracle, to the compiled reference and to
hand-written answers on the CPU.  The sequences are built there and shared.

The restatement receives exactly what the device holds: the records fl32(p - o) (the upload's origin is asserted to be the stated one and
the records are read back), the fp32 normals and covariances, the pose.  Points that map_contents_ref calls ambiguous are removed from the
input before either side sees it: none in a designed sequence, at most 1 % in a random one (the CPU file shows: none for these seeds).

Compared after EVERY insert:
  * exactly: size(), the coordinates row by row (the voxel ids), the counts, which points a flat voxel holds in which slot;
  * values: a stored value m leaves the device as fl32(m - o_map) and download() returns fl32(that + o_map), so
        |got - m| <= 2^-24 (|m - o_map| + |m|) (1 + 2^-20)  +  (N + 16) 2^-52 sum |terms| / N
    (o_map through sga_index_origin; the last term is the fp64 slack of the running state, its scale the magnitudes of the terms that went
    into the voxel; the factor 1 + 2^-20 is for the second order of the two roundings); covariances and normals 2^-24 |c| plus that slack;
  * the hash: batch_knn_search((coords + 0.5) leaf, 1) over one offset finds voxel v (for a flat map one of its slots), the centre of a
    voxel that an LRU sweep removed finds nothing.

Gaussian incremental maps: faces and octants, the range edge (NaN, +-inf, +-3e38, +-2^31), launch edges, growth one voxel at a time, running
sums, creation order, LRU, a far frame, a random posed scene.  Flat maps, all four kinds: the keep rule, order, attributes, LRU refresh,
growth.  One-shot maps, lone and batched (B = 1, 3): the faces, range-edge, launch-edge, creation-order and far-frame clouds.

Observed on the MI355X (printed with -s): 79 tests in 1.9 s, the slowest 0.34 s; no point of any sequence is ambiguous; the largest error
over its bound is 0.99 (fp32 rounding of a covariance: the bound is that rounding), 0.89 for a mean (far frame), 0 where the values are dyadic.
Before the fix of csrc/voxel_hash.hpp / voxel_steps.hpp the one-shot range-edge cases failed at the counts (voxel 0 held 31 points for 28:
the three NaN points), test_queries_beyond_the_conversion_find_nothing failed for the NaN queries (they found voxel 0), and
test_range_edge failed at the hash check after the cloud at +2^31 (the map's frame had followed it).  A point or query at exactly -2^31
voxel units was dropped by that build as well: the undefined abs(INT_MIN) happened to compile into a test that rejects it.

Each of these defects, seeded into a scratch build, fails the designed cases named (and others):
  LRU `<` as `<=`                       test_lru[1-1], [1-2], [2-3], test_lru_changed_between_inserts, test_lru_removes_only_the_last_voxel, test_flat_lru_refresh
  flat `< min_sq` as `<=`               test_flat_keep_rule[10-0.0], [10-0.0625], [16-0.0], [16-0.0625]
  un-finalize skipped                   test_running_sums, test_growth_one_voxel_at_a_time, test_launch_edges, test_range_edge, test_lru[...]
  posed_cov as R^T C R                  test_faces_and_octants[*-quarter_z], [*-permuted], test_running_sums, test_launch_edges, test_flat_order[cov]
  grow copying half of `used`           test_growth_one_voxel_at_a_time, test_flat_growth[*]
  seg_first from a run's last entry     test_creation_order, test_faces_and_octants[*], test_flat_lru_refresh[*]
  range test with `<= 2^20`             test_range_edge, test_one_shot_lone / _batched_alone[range edge], test_one_shot_batched_by_three[0]
  the flat run loop walked backwards    test_flat_keep_rule[*], test_flat_order[*], test_flat_lru_refresh[*]
"""
import numpy as np
import pytest

import map_contents_ref as mc
import small_gicp_amd as sga
import test_map_contents_ref as cases
from small_gicp_amd import api

pytestmark = pytest.mark.gpu

E24, E52 = 2.0 ** -24, 2.0 ** -52
SECOND_ORDER = 1.0 + 2.0 ** -20
FLAT_KINDS = {"points": (api.IncrementalVoxelMap, False, False), "normal": (api.IncrementalVoxelMapNormal, True, False), "cov": (api.IncrementalVoxelMapCov, False, True),
              "normal_cov": (api.IncrementalVoxelMapNormalCov, True, True)}


# ---- what the device holds ---------------------------------------------------------------------------------------------------------------
def origin_of(m):
    o = np.zeros(3)
    api.check(sga.load().sga_index_origin(m.h, api._dp(o)))
    return o


def upload(step, normals=True, covs=True):
    """the step's cloud on the device: the origin is the stated one and the records are the ones the restatement is given"""
    cloud = sga.PointCloud(step.points, normals=step.normals if normals else None, covs=step.covs if covs else None)
    assert np.array_equal(cloud.origin(), step.origin), (cloud.origin(), step.origin)
    if len(step.points):
        with np.errstate(invalid="ignore"):
            assert np.array_equal(cloud.xyz64(), step.records() + step.origin, equal_nan=True)
    return cloud


def check_hash(label, m, coords, counts, leaf, gone):
    """every voxel is found under its coordinates, with its id; a removed voxel's centre finds nothing"""
    V = len(coords)
    if V:
        idx, d2 = m.batch_knn_search((coords.astype(np.float64) + 0.5) * leaf, 1)
        assert np.array_equal(idx[:, 0] >> 32, np.arange(V)), (label, np.flatnonzero((idx[:, 0] >> 32) != np.arange(V))[:8])
        assert ((idx[:, 0] & 0xFFFFFFFF) < counts).all() and np.isfinite(d2).all(), label
    if len(gone):
        idx, d2 = m.batch_knn_search((np.array(sorted(gone), dtype=np.float64) + 0.5) * leaf, 1)
        assert (idx == -1).all() and np.isinf(d2).all(), (label, idx[:8, 0])


def within(label, what, got, want, bound):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (label, what, got.shape, want.shape)
    assert np.isfinite(got).all(), (label, what, "not finite", np.argwhere(~np.isfinite(got))[:4])
    err = np.abs(got - want)
    bad = err > bound
    assert not bad.any(), (label, what, int(bad.sum()), np.argwhere(bad)[:4], err[bad][:4], np.broadcast_to(bound, err.shape)[bad][:4])
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err > 0, err / bound, 0.0)
    return float(r.max()) if r.size else 0.0


def compare_gaussian(label, m, want, gone=()):
    """-> the worst error over its bound"""
    V = want.size()
    assert m.size() == V, (label, m.size(), V)
    coords, means, c6, counts = m.download()
    assert np.array_equal(coords, want.coords()), (label, np.flatnonzero((coords != want.coords()).any(1))[:8])
    assert np.array_equal(counts, want.counts()), (label, np.flatnonzero(counts != want.counts())[:8])
    worst = 0.0
    if V:
        wm, wc, sm, sc = want.means()
        o = origin_of(m)
        worst = within(label, "means", means, wm, E24 * (np.abs(wm - o) + np.abs(wm)) * SECOND_ORDER + sm)
        worst = max(worst, within(label, "covariances", api.mats_from_sym6(c6.astype(np.float64)), wc, E24 * np.abs(wc) * SECOND_ORDER + sc))
    check_hash(label, m, want.coords(), np.ones(V, np.int64), want.leaf, gone)
    return worst


def compare_flat(label, m, want, has_normals, has_covs, gone=()):
    V = want.size()
    assert m.size() == V, (label, m.size(), V)
    worst = 0.0
    if V:
        coords, counts, pts, nr, c6 = m._download(has_normals, has_covs)
        assert np.array_equal(coords, want.coords()), (label, np.flatnonzero((coords != want.coords()).any(1))[:8])
        assert np.array_equal(counts, want.counts()), (label, np.flatnonzero(counts != want.counts())[:8], counts[counts != want.counts()][:8])
        w = want.slots()
        o = origin_of(m)
        worst = within(label, "points", pts, w["points"], E24 * (np.abs(w["points"] - o) + np.abs(w["points"])) * SECOND_ORDER + w["slack_points"])
        if has_normals:
            worst = max(worst, within(label, "normals", nr, w["normals"], E24 * np.abs(w["normals"]) * SECOND_ORDER + w["slack_normals"]))
        if has_covs:
            worst = max(worst, within(label, "covariances", api.mats_from_sym6(c6.astype(np.float64)), w["covs"], E24 * np.abs(w["covs"]) * SECOND_ORDER + w["slack_covs"]))
    check_hash(label, m, want.coords(), want.counts(), want.leaf, gone)
    return worst


def prepared(seq, kind):
    """the sequence without its ambiguous points: none may go from a designed one, at most the cap from a random one"""
    clean, removed, total = cases.cleaned(seq, kind)
    assert removed <= (cases.AMBIGUOUS_CAP * total if seq.random else 0), (seq.name, removed, total)
    return clean


def run_gaussian(seq):
    seq = prepared(seq, mc.GAUSSIAN)
    m = sga.GaussianVoxelMap(seq.leaf)
    if seq.lru is not None:
        m.set_lru(*seq.lru)
    worst, before = 0.0, set()
    for k, s, want, _ in cases.restate(seq, mc.GAUSSIAN):
        if s.lru is not None:
            m.set_lru(*s.lru)
        m.insert(upload(s), s.T)
        now = set(map(tuple, want.coords().tolist()))
        worst = max(worst, compare_gaussian((seq.name, "insert", k), m, want, before - now))
        cases.check_expectation(seq, k, want, seq.expect[k])
        before = now
    print("%-28s %2d inserts, %5d voxels at the end, worst error / bound %.3f" % (seq.name, len(seq.steps), m.size(), worst))
    return m


def run_flat(seq, kind, bare=False):
    """bare: the clouds carry only the attributes the kind keeps"""
    cls, has_n, has_c = FLAT_KINDS[kind]
    seq = prepared(seq, mc.FLAT)
    m = cls(seq.leaf)
    m.set_setting(seq.min_sq, seq.max_points)
    if seq.lru is not None:
        m.set_lru(*seq.lru)
    worst, before = 0.0, set()
    for k, s, want, _ in cases.restate(seq, mc.FLAT, has_n, has_c):
        if s.lru is not None:
            m.set_lru(*s.lru)
        m.insert(upload(s, has_n or not bare, has_c or not bare), s.T)
        now = set(map(tuple, want.coords().tolist()))
        worst = max(worst, compare_flat((seq.name, kind, "insert", k), m, want, has_n, has_c, before - now))
        cases.check_expectation(seq, k, want, seq.expect[k])
        before = now
    print("%-28s %-10s %2d inserts, %5d voxels at the end, worst error / bound %.3f" % (seq.name, kind, len(seq.steps), m.size(), worst))
    return m


# ---- Gaussian incremental maps ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose_name", list(cases.EXACT_POSES))
@pytest.mark.parametrize("leaf", cases.FACE_LEAVES)
def test_faces_and_octants(leaf, pose_name):
    """dyadic points at voxel centres and exactly on faces, edges and corners in all eight octants, -0.0 among them; every pose is exact"""
    run_gaussian(cases.case_faces(leaf, pose_name))


@pytest.mark.parametrize("pose_name", list(cases.EXACT_POSES))
def test_interior_points_at_leaf_0_3(pose_name):
    run_gaussian(cases.case_interior(pose_name))


def test_range_edge():
    """+-(2^20 - 1) are kept; 2^20, -(2^20 - 1) - 0.5, +-2^31, +-3e38, +-inf and NaN on each axis in turn are dropped, each in a cloud of its
    own (whose frame is centred on it: the record is 0 and the value arrives through the pose's translation); the eight voxels stay as
    they are and finite, and take ordinary points afterwards.  A cloud of which no point can enter the map does not move the map's frame
    either: with the frame at 2^31 the fp32 records of the voxels at the origin would be worth nothing (the hash check finds every voxel
    through its fp32 centre after every insert)."""
    m = run_gaussian(cases.case_range_edge())
    assert not origin_of(m).any()


def test_launch_edges():
    """clouds of 1, 255, 256, 257 and 2049 points touching 1, 255, 256, 257 and 257 voxels"""
    run_gaussian(cases.case_launch_edges())


def test_growth_one_voxel_at_a_time():
    """200 -> 511 -> 512 -> 513 (the table is rebuilt) -> 1023 -> 1024 -> 1025 (the arrays are regrown and copied) -> 2100 (both)"""
    m = run_gaussian(cases.case_growth())
    assert m.size() == cases.GROWTH_TOTALS[-1]


def test_running_sums():
    """one voxel hit in 12 consecutive inserts by 1, 2, 3 and 17 points under general rotations, anisotropic covariances"""
    run_gaussian(cases.case_running_sums())


def test_creation_order():
    run_gaussian(cases.case_creation_order())


@pytest.mark.parametrize("horizon,cycle", cases.LRU_PAIRS)
def test_lru(horizon, cycle):
    """nine inserts over a sliding window of voxels and an empty cloud: sweeps that remove nothing, everything, only voxel 0; both sides of
    lru + horizon < counter; inserts into renumbered survivors and into an emptied map"""
    run_gaussian(cases.case_lru(horizon, cycle))


def test_lru_changed_between_inserts():
    run_gaussian(cases.case_lru_changing())


def test_lru_removes_only_the_last_voxel():
    run_gaussian(cases.case_lru_last())


def test_far_frame():
    """float64 clouds around (1e5, 2e5, 300) (records relative to a non-zero origin), poses 3 km away with general rotations"""
    m = run_gaussian(cases.case_far_frame())
    assert np.abs(origin_of(m)).max() > 1e5  # the map's frame follows the posed scan


@pytest.mark.parametrize("leaf", cases.SCENE_LEAVES)
def test_random_posed_scene(leaf):
    run_gaussian(cases.case_scene(leaf))


# ---- flat maps ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_sq", cases.KEEP_MIN_SQ)
@pytest.mark.parametrize("max_points", cases.KEEP_MAX)
def test_flat_keep_rule(max_points, min_sq):
    """a point exactly 0.25 away is kept at min_sq 0.0625, one 2^-20 nearer is rejected; duplicates are rejected, but kept at min_sq 0; a
    voxel stops at max_points.  The clouds carry only what the kind keeps."""
    for kind in FLAT_KINDS:
        run_flat(cases.case_keep(max_points, min_sq), kind, bare=True)


@pytest.mark.parametrize("kind", list(FLAT_KINDS))
def test_flat_order(kind):
    """of mutually exclusive points the earliest in the cloud wins; a cell filled over three inserts under three poses, with rejections
    against points kept under another pose"""
    run_flat(cases.case_exclusive(), kind)
    run_flat(cases.case_fill(), kind)


def test_flat_attributes():
    """normals rotate without the translation, covariances are R C R^T, in slot order; all four kinds keep the same points in the same slots"""
    held = {}
    for kind in FLAT_KINDS:
        m = run_flat(cases.case_attributes(), kind)
        coords, counts, pts, _, _ = m._download(False, False)
        held[kind] = (coords, counts, pts)
    for kind in FLAT_KINDS:
        assert all(np.array_equal(a, b) for a, b in zip(held[kind], held["points"])), kind


@pytest.mark.parametrize("kind", list(FLAT_KINDS))
def test_flat_lru_refresh(kind):
    """a full voxel hit only by rejected points is refreshed and survives the sweep that removes its untouched neighbour"""
    run_flat(cases.case_lru_refresh(), kind)


@pytest.mark.parametrize("kind", list(FLAT_KINDS))
def test_flat_growth(kind):
    m = run_flat(cases.case_growth(), kind)
    assert m.size() == cases.GROWTH_TOTALS[-1]


# ---- one-shot maps ----------------------------------------------------------------------------------------------------------------------------------
ONE_SHOT = cases.one_shot_steps()
LEAF_ONE = [name for name, (leaf, _) in ONE_SHOT.items() if leaf == 1.0]


def check_one_shot(name, m, leaf, step):
    """the map against the restatement's single insert at the identity: ids, coordinates and counts exactly, means and covariances within
    the bound (the map's frame is the cloud's), no voxel holds a NaN"""
    assert not mc.near_face(step.records(), step.origin, None, leaf).any(), name
    want, drop = mc.one_shot(step.records(), step.origin, step.covs.astype(np.float64), leaf)
    assert np.array_equal(origin_of(m), step.origin), name
    worst = compare_gaussian(("one-shot", name), m, want)
    if name == "range edge":
        _, vox, counts = cases.one_shot_edge_cloud()
        assert want.coords().tolist() == [list(v) for v in vox] and want.counts().tolist() == counts and int(drop.sum()) == 3 * len(cases.EXTREMES)
    return worst


@pytest.mark.parametrize("name", list(ONE_SHOT))
def test_one_shot_lone(name):
    leaf, step = ONE_SHOT[name]
    worst = check_one_shot(name, sga.GaussianVoxelMap.from_cloud(upload(step), leaf), leaf, step)
    print("one-shot %-16s worst error / bound %.3f" % (name, worst))


@pytest.mark.parametrize("name", list(ONE_SHOT))
def test_one_shot_batched_alone(name):
    """build_gaussian_voxelmaps with B = 1"""
    leaf, step = ONE_SHOT[name]
    (m,) = sga.build_gaussian_voxelmaps([upload(step)], leaf)
    check_one_shot(name, m, leaf, step)


@pytest.mark.parametrize("first", range(0, len(LEAF_ONE), 3))
def test_one_shot_batched_by_three(first):
    """build_gaussian_voxelmaps with B = 3: the clouds of leaf 1 in threes (the range-edge cloud spans more than 65536 voxels: it goes through
    the lone routine inside the call, its neighbours through the shared launches)"""
    names = [LEAF_ONE[(first + j) % len(LEAF_ONE)] for j in range(3)]
    maps = sga.build_gaussian_voxelmaps([upload(ONE_SHOT[n][1]) for n in names], 1.0)
    for n, m in zip(names, maps):
        check_one_shot(n, m, 1.0, ONE_SHOT[n][1])


# ---- the query side of the same range test ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offsets", [1, 7, 27])
def test_queries_beyond_the_conversion_find_nothing(offsets):
    """csrc/voxel_hash.hpp decides the range of a query's voxel on the double as well: queries at -2^31 (whose voxel coordinate is INT_MIN),
    +-3e38, +-inf and NaN on each axis find nothing in a map that holds the voxels around the origin; ordinary queries find their voxel"""
    c = np.array([[i, j, k] for i in (-1, 0) for j in (-1, 0) for k in (-1, 0)], dtype=np.float64)
    pts = cases.f32(c + 0.5)
    gm = sga.GaussianVoxelMap(1.0)
    gm.insert(sga.PointCloud(pts, covs=cases.designed_covs(len(pts))))
    fm = api.IncrementalVoxelMap(1.0)
    fm.insert(sga.PointCloud(pts))
    q = []
    for a in range(3):
        for value in (-2147483648.0, 2147483648.0, -3e38, 3e38, -np.inf, np.inf, np.nan):
            p = [0.5, 0.5, 0.5]
            p[a] = value
            q.append(p)
    for m in (gm, fm):
        m.set_search_offsets(offsets)
        idx, d2 = m.batch_knn_search(np.array(q), 1)
        assert (idx == -1).all(), (offsets, np.flatnonzero(idx[:, 0] != -1), idx[idx != -1][:8])
        idx, _ = m.batch_knn_search(c + 0.5, 1)
        assert np.array_equal(idx[:, 0] >> 32, np.arange(len(c)))

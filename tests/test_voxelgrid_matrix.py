"""The voxel grid (sga_voxelgrid_sampling, csrc/preprocess.hip) against its definition in float64 (tests/voxelgrid_ref.py), in every regime
of its host code and kernels: both key widths and the three key layouts, the three branches of the sort (and rocPRIM's own change of
algorithm above 2^20 keys), the 64-tile look-back window of ds_segments_kernel, runs that start on, end on and straddle its 2048-key tiles,
the unrolled and the remainder loop of ds_mean_kernel, both ways of launching it, the partition at lattice points, every kind of dropped
point, geo-referenced frames, and the status words a context keeps between calls — including the reset at 2^30 - 1 calls.

Every case goes through check(): it asserts through PointCloud._voxelgrid_plan (the code the call itself runs) that the input reached
the regime the case names, runs the grid twice and requires identical bits, the input's origin on the output, the restatement's voxel
count and every centroid coordinate within

    |out - mean| <= ulp32(max(|out|, |mean|)) / 2 + 2 (N + 2) 2^-53 max|p_i|

(voxelgrid_ref.centroid_bound; nothing measured, no row exempt).  The largest error / bound seen on an MI355X is recorded below.

WORST_RATIO_OBSERVED = (not measured yet)
"""
from typing import NamedTuple

import numpy as np
import pytest

import small_gicp_amd as sga
from voxelgrid_ref import check_grid, downsample_ref

gpu = pytest.mark.gpu
F32 = np.float32
TILE = 2048  # kSegTile
WORST = {}   # label -> error / bound, printed per case


# ---- the check -----------------------------------------------------------------------------------------------------------------------
def records_of(cloud):
    """The fp32 records of a cloud (device frame).  xyz64 is record + origin in double: taking the origin off again must give numbers
    that fp32 holds exactly — membership is then decided on what the device holds, not on the caller's numbers before rounding."""
    x = cloud.xyz64() - cloud.origin()
    r = x.astype(F32)
    assert np.array_equal(r.astype(np.float64), x, equal_nan=True), "xyz64 - origin is not the fp32 record"
    return r


def check(label, cloud, leaf, want_plan=None, ref=None):
    """The five checks of the module docstring; returns (the output's records, the restatement)."""
    plan = cloud._voxelgrid_plan(leaf)
    for key, want in (want_plan or {}).items():
        assert plan[key] == want, (label, key, plan[key], "expected", want, plan)
    a, b = sga.voxelgrid_sampling(cloud, leaf), sga.voxelgrid_sampling(cloud, leaf)
    ra, rb = records_of(a), records_of(b)
    assert ra.shape == rb.shape and np.array_equal(ra.view(np.uint32), rb.view(np.uint32)), (label, "two runs differ", ra.shape, rb.shape)
    assert np.array_equal(a.origin(), cloud.origin()) and np.array_equal(b.origin(), cloud.origin()), (label, a.origin(), cloud.origin())
    if ref is None:
        ref = downsample_ref(records_of(cloud), cloud.origin(), leaf)
    worst = check_grid(ra, ref, label)
    WORST[label] = max(worst, WORST.get(label, 0.0))
    print("%-44s n=%8d voxels=%8d dropped=%7d largest run=%7d  keys %d B %2d bits box=%d sort=%d tiles=%5d spec=%d  error / bound %.3f" % (
        label, cloud.size(), len(ref.counts), len(ref.dropped), ref.counts.max() if len(ref.counts) else 0, plan["key_bytes"], plan["total"], plan["box"], plan["sort"], plan["tiles"], plan["speculative"], worst))
    return ra, ref


def upload(points, path, ctx=None):
    """The same points through one of the upload paths: 'pageable' (the box comes from the staging pass), 'pinned' (the box arrives as a
    note from the pack kernel), 'slice' (a cloud made on the device: no box, the reference's key layout)."""
    kw = {} if ctx is None else {"ctx": ctx}
    if path == "pageable":
        return sga.PointCloud(points, **kw)
    if path == "pinned":
        assert points.dtype == F32
        return sga.PointCloud(sga.pinned_copy(points), **kw)
    if path == "slice":
        return sga.PointCloud(points, **kw).slice(0, len(points))
    raise ValueError(path)


class Between:
    """a field of the plan that may take any value of a range"""

    def __init__(self, lo, hi):
        self.lo, self.hi = lo, hi

    def __eq__(self, v):
        return self.lo <= v <= self.hi

    def __repr__(self):
        return "Between(%d, %d)" % (self.lo, self.hi)


NO_BOX = {"key_bytes": 8, "bits": (21, 21, 21), "total": 63, "box": False}


def sort_path(n):
    return 0 if n <= 2048 else 1 if n <= 200_000 else 2


def plan_of_size(n):
    """the fields of the plan that follow from the number of points alone"""
    return {"sort": sort_path(n), "tiles": (n + TILE - 1) // TILE, "speculative": n <= 262_144}


# ---- clouds --------------------------------------------------------------------------------------------------------------------------
def scan(n, seed, extent=60.0):
    """a Gaussian scene shaped like a LiDAR scan: 20 m standard deviation in x and y, z in [-2, 6)"""
    rng = np.random.default_rng(seed)
    p = rng.normal(0.0, extent / 3, (n, 3)).astype(F32)
    p[:, 2] = rng.uniform(-2.0, 6.0, n).astype(F32)
    return p


def sized_scan(n):
    """the scene shrunk with the number of points, so that small clouds too have voxels of several points (about three at 0.25 m)"""
    f = min(1.0, max(0.01, (n / 1_500_000) ** 0.5))
    return (scan(n, 100 + n % 97) * F32(f)).astype(F32)


def in_voxels(coords, counts, leaf, rng):
    """counts[j] points strictly inside voxel coords[j] (5 % to 95 % of its edge)"""
    c = np.repeat(np.asarray(coords, dtype=np.float64), counts, axis=0)
    return ((c + rng.uniform(0.05, 0.95, c.shape)) * leaf).astype(F32)


RUNS = list(range(1, 41)) + [255, 256, 257, 1000, 5000]


def run_shapes_cloud(seed=11, leaf=0.25):
    """voxels holding exactly r points for every r of RUNS (ds_mean_kernel: no, one, several trips of the unrolled loop, every remainder),
    in shuffled point order"""
    rng = np.random.default_rng(seed)
    j = np.arange(len(RUNS))
    coords = np.c_[2 * j - 40, (7 * j) % 11 - 5, j % 4 - 2]
    p = in_voxels(coords, RUNS, leaf, rng)
    return p[rng.permutation(len(p))]


def aligned_run_cloud(before, run, after, seed=12, leaf=0.25):
    """`before` one-point voxels, one voxel of `run` points, `after` one-point voxels, in that order of the keys (z decides), shuffled"""
    rng = np.random.default_rng(seed)
    coords = np.r_[np.c_[np.arange(before) - before // 2, np.zeros(before), np.full(before, -1)], [[0, 0, 0]], np.c_[np.arange(after) - after // 2, np.zeros(after), np.full(after, 1)]]
    p = in_voxels(coords, [1] * before + [run] + [1] * after, leaf, rng)
    return p[rng.permutation(len(p))]


def two_voxel_cloud(n=300_000, scattered=0, seed=13, leaf=1.0):
    """n points in two voxels (more than 64 consecutive tiles without a run head, twice) and `scattered` points in voxels of their own,
    half of them sorted in front of the long runs and half behind"""
    rng = np.random.default_rng(seed)
    p = in_voxels([[0, 0, 0], [1, 0, 0]], [n // 2, n - n // 2], leaf, rng)
    if scattered:
        s = rng.uniform(-200.0, 200.0, (scattered, 3))
        s[: scattered // 2, 2] = rng.uniform(-50.0, -1.5, scattered // 2)
        s[scattered // 2 :, 2] = rng.uniform(2.5, 50.0, scattered - scattered // 2)
        p = np.r_[p, s.astype(F32)]
    return p[rng.permutation(len(p))]


def lattice_cloud():
    """one point per voxel of a 41^3 lattice of 1 mm voxels, at the voxels' centres"""
    g = np.arange(-20, 21, dtype=np.float64)
    k = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    return ((k + 0.5) * 1e-3).astype(F32)


BOUNDARY_LEAVES = [0.25, 0.1, 1.0 / 3.0, 10.0, 1e6]


def boundary_cloud(seed=14):
    """points on the lattice j * leaf of every leaf of BOUNDARY_LEAVES but the last (0.25: exact in fp32; 0.1, 1/3: not), j negative and
    positive, on one axis, two or all three; the fp32 neighbours on either side of each; +-0 and fp32 denormals.  Centred: origin 0."""
    rng = np.random.default_rng(seed)
    rows = []
    for leaf in BOUNDARY_LEAVES[:-1]:
        j = np.r_[np.arange(-300, 301), rng.integers(-4000, 4001, 400), -4000, 4000]  # (the box is symmetric: the origin stays 0)
        on = (j * leaf).astype(F32)
        for v in (on, np.nextafter(on, F32(np.inf)), np.nextafter(on, F32(-np.inf))):
            other = (rng.integers(-40, 41, (len(v), 2)) * leaf).astype(F32)
            rows += [np.c_[v, other], np.c_[other[:, 0], v, other[:, 1]], np.c_[other, v], np.c_[v, v, v]]
    tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, -1.1754944e-38], F32)
    rows.append(np.stack(np.meshgrid(tiny, tiny[:4], tiny[:2], indexing="ij"), -1).reshape(-1, 3))
    p = np.concatenate(rows).astype(F32)
    return p[rng.permutation(len(p))]


def reciprocal_cloud():
    """The multiples of 3.5 m, which fp32 holds exactly, up to +-105 km on x: points of the lattice of leaf 0.7 at which p * (1 / 0.7) and
    p / 0.7 round to different sides of the integer for thousands of them (the nearest at 10.5 m) — the grid multiplies."""
    k = np.arange(-30_000, 30_001)
    x = (3.5 * k).astype(F32)
    return np.c_[x, (k % 7 * 0.1).astype(F32), (k % 3 * 0.1).astype(F32)]


def with_bad(points, bad_rows, seed=15):
    """points with the given rows appended, shuffled"""
    p = np.r_[points, np.asarray(bad_rows, dtype=F32).reshape(-1, 3)].astype(F32)
    return p[np.random.default_rng(seed).permutation(len(p))]


def layout_cloud(zext, seed=16, n=60_000):
    """a uniform box of +-150 x +-150 x +-zext metres with its corners occupied, and three points without a voxel (their key is
    1 << total: the top bit of a 32-bit key when total is 31)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3)) * [150.0, 150.0, zext]
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * [150.0, 150.0, zext]
    return with_bad(np.r_[p, corners].astype(F32), [[np.nan, 0, 0], [0, np.inf, 0], [1, 2, -np.inf]], seed)


def outlier_cloud(seed=17, n=50_000):
    """a dense scan and one finite outlier 2.6e5 m away: inside the grid at 0.25 m, 21 key bits on x"""
    return with_bad(scan(n, seed), [[2.6e5, 1.0, 0.5]], seed)


def geo_cloud(seed=18, n=40_000):
    """float64 input far from the origin"""
    return scan(n, seed).astype(np.float64) + np.array([1_000_064.0, -2_000_000.0, 128.0])


def limit_cloud(seed=19, n=30_000):
    """float64 input straddling the positive limit 2^20 * leaf of the grid at leaf 1.0, on x"""
    rng = np.random.default_rng(seed)
    return np.c_[2.0**20 + rng.uniform(-50.0, 50.0, n), rng.uniform(-30.0, 30.0, n), rng.uniform(-2.0, 6.0, n)]


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    label: str
    make: object     # () -> (n, 3) points, float32 or float64
    leaf: float
    want: dict       # fields of the plan the uploaded cloud must show (the size's fields are added; a 'slice' always shows NO_BOX)
    paths: tuple     # upload paths; all of them must give equal bits


BOX4 = {"key_bytes": 4, "box": True}
BOX8 = {"key_bytes": 8, "box": True}
CASES = []


def case(label, make, leaf, want, paths=("pageable",)):
    CASES.append(Case(label, make, leaf, want, tuple(paths)))


# sizes: the sort's branches, one and several tiles, the 64-tile window (131072 = 64 x 2048), both launches of the centroid kernel, onesweep
SIZES = [1, 2, 7, 8, 9, 255, 256, 257, 2047, 2048, 2049, 4097, 131_071, 131_072, 131_073, 199_999, 200_000, 200_001, 262_143, 262_144, 262_145, 1_048_576, 1_048_577, 1_500_000]
for _n in SIZES:
    case("size %d" % _n, lambda n=_n: sized_scan(n), 0.25, BOX4, ("pageable", "slice") if _n in (1, 9, 2048, 2049, 200_001, 262_145, 1_048_577) else ("pageable",))
# key layouts, each through the three upload paths
case("layout total 31", lambda: layout_cloud(40.0), 0.25, {**BOX4, "bits": (11, 11, 9), "total": 31}, ("pageable", "pinned", "slice"))
case("layout total 32", lambda: layout_cloud(80.0), 0.25, {**BOX8, "bits": (11, 11, 10), "total": 32}, ("pageable", "pinned", "slice"))
case("layout outlier 2.6e5 m", outlier_cloud, 0.25, {**BOX8, "total": Between(33, 62)}, ("pageable", "pinned", "slice"))
case("layout scan", lambda: scan(120_000, 20), 0.25, BOX4, ("pageable", "pinned", "slice"))
case("box of one point", lambda: np.tile(np.array([[1.5, -2.0, 0.25]], F32), (5000, 1)), 0.25, {**BOX4, "bits": (2, 2, 2), "total": 6}, ("pageable", "pinned", "slice"))
case("box of one x", lambda: np.c_[np.full(5000, 3.125), scan(5000, 21)[:, 1:]].astype(F32), 0.25, BOX4, ("pageable", "slice"))
# run shapes
case("runs 1..40, 255..257, 1000, 5000", run_shapes_cloud, 0.25, BOX4, ("pageable", "slice"))
case("run starts on a tile boundary", lambda: aligned_run_cloud(2 * TILE, 5000, 1000), 0.25, BOX4)       # [4096, 9096): tile 3 has no head at all
case("run ends on a tile boundary", lambda: aligned_run_cloud(4 * TILE - 5000, 5000, 1000), 0.25, BOX4)  # [3192, 8192)
case("run straddles a tile boundary", lambda: aligned_run_cloud(1000, 5000, 1000), 0.25, BOX4)           # [1000, 6000)
case("run is one whole tile", lambda: aligned_run_cloud(TILE, TILE, 1000), 0.25, BOX4)                   # [2048, 4096)
case("300000 points in two voxels", lambda: two_voxel_cloud(), 1.0, {**BOX4, "tiles": 147}, ("pageable", "slice"))
case("300000 in two voxels + 50000 scattered", lambda: two_voxel_cloud(scattered=50_000), 1.0, {**BOX4, "tiles": 171})
case("one voxel per point", lattice_cloud, 1e-3, BOX4, ("pageable", "slice"))
case("one voxel in total", lambda: np.abs(scan(100_000, 22)) + F32(0.5), 1e3, {**BOX4, "bits": (2, 2, 2)}, ("pageable", "slice"))
# the boundaries of the partition
for _leaf in BOUNDARY_LEAVES:
    case("lattice points at leaf %.6g" % _leaf, boundary_cloud, _leaf, {"box": True}, ("pageable", "slice"))
case("lattice points at leaf 0.7: reciprocal multiply", reciprocal_cloud, 0.7, {"box": True}, ("pageable", "slice"))
# dropped points.  One outlier moves the centre of the box, and with it the device frame, half way to it (the scan's records are then coarse:
# the restatement works on the records); a mirrored pair keeps the origin at 0 and the records what they were.
for _v in (1e9, 3e38):
    for _a in range(3):
        for _s in (1.0, -1.0):
            _row = [0.0, 0.0, 0.0]
            _row[_a] = _s * _v
            case("dropped %+.0e on axis %d" % (_s * _v, _a), lambda row=tuple(_row): with_bad(scan(5000, 23), [row]), 0.25, {"box": _v < 1e15}, ("pageable", "slice"))
        _rows = np.zeros((2, 3))
        _rows[0, _a], _rows[1, _a] = _v, -_v
        case("dropped +-%.0e on axis %d" % (_v, _a), lambda rows=_rows.copy(): with_bad(scan(5000, 24), rows), 0.25, {"box": _v < 1e15}, ("pageable", "slice"))
NONFINITE = [[v if a == k else 1.0 for k in range(3)] for v in (np.nan, np.inf, -np.inf) for a in range(3)]
case("dropped NaN, +inf, -inf in each coordinate", lambda: with_bad(scan(5000, 25), NONFINITE), 0.25, BOX4, ("pageable", "pinned", "slice"))
case("everything dropped: NaN", lambda: np.full((5000, 3), np.nan, F32), 0.25, NO_BOX, ("pageable", "pinned"))
case("everything dropped: out of range", lambda: np.full((5000, 3), 1e9, F32), 0.25, {**BOX4, "bits": (1, 1, 1), "total": 3}, ("pageable", "slice"))
case("first dropped point at n - 1", lambda: with_bad(scan(6000, 26), [[np.nan, 0, 0]]), 0.25, BOX4, ("pageable", "slice"))
case("first dropped point at 2048", lambda: with_bad(scan(TILE, 27), [[np.nan, 0, 0]] * 100), 0.25, BOX4, ("pageable", "slice"))
case("first dropped point at 4096", lambda: with_bad(scan(2 * TILE, 28), [[0, 3e5, 0], [0, -3e5, 0]] * 50), 0.25, BOX8, ("pageable", "slice"))
case("300000 points, all dropped", lambda: np.full((300_000, 3), -1e9, F32), 0.25, {**BOX4, "speculative": False}, ("pageable", "slice"))
case("300000 points, all but one dropped", lambda: with_bad(np.full((299_999, 3), np.nan, F32), [[1.0, 2.0, 3.0]]), 0.25, {**BOX4, "speculative": False}, ("pageable", "slice"))
case("exactly one valid point", lambda: with_bad(np.full((999, 3), np.nan, F32), [[-1.0, 2.0, -3.0]]), 0.25, BOX4, ("pageable", "pinned", "slice"))
# geo-referenced clouds (float64 input: the frame's origin is subtracted in double before the upload)
case("geo-referenced at leaf 4", geo_cloud, 4.0, BOX4, ("pageable", "slice"))
case("geo-referenced at leaf 0.25: all dropped", geo_cloud, 0.25, {"box": True}, ("pageable", "slice"))
case("straddling the positive limit at leaf 1", limit_cloud, 1.0, BOX4, ("pageable", "slice"))

LABELS = [c.label for c in CASES]
assert len(set(LABELS)) == len(LABELS)


def assert_shape(label, n, ref):
    """what a case's name promises about its cloud, asserted on the restatement of the records the device holds"""
    if "all dropped" in label or "everything dropped" in label:
        assert len(ref.counts) == 0 and len(ref.dropped) == n
    if "all but one dropped" in label or "exactly one valid" in label:
        assert len(ref.counts) == 1 and len(ref.dropped) == n - 1
    if label.startswith("first dropped point at"):
        want_first = n - 1 if label.endswith("n - 1") else int(label.split()[-1])
        assert n - len(ref.dropped) == want_first  # the dropped points sort behind every voxel
    if label.startswith("dropped "):
        assert 1 <= len(ref.dropped) and (len(ref.dropped) <= 2 or "NaN" in label), len(ref.dropped)
    if label == "one voxel per point":
        assert len(ref.counts) == n
    if label == "one voxel in total":
        assert len(ref.counts) == 1
    if label.startswith("300000 points in two voxels"):
        assert len(ref.counts) == 2 and ref.counts.min() > 64 * TILE
    if label.startswith("300000 in two voxels +"):
        long_runs = np.flatnonzero(ref.counts > 64 * TILE)
        assert len(long_runs) == 2 and long_runs[0] > 20_000 and long_runs[1] < len(ref.counts) - 20_000, (long_runs, len(ref.counts))
    if label.startswith("runs 1..40"):
        assert sorted(ref.counts.tolist()) == RUNS
    if label.startswith("run "):
        long_run = int(np.argmax(ref.counts))
        first, length = int(ref.counts[:long_run].sum()), int(ref.counts[long_run])
        assert {"run starts on a tile boundary": first % TILE == 0 and (first + length) % TILE != 0, "run ends on a tile boundary": first % TILE != 0 and (first + length) % TILE == 0,
                "run straddles a tile boundary": first % TILE != 0 and (first + length) % TILE != 0 and first // TILE != (first + length) // TILE,
                "run is one whole tile": first % TILE == 0 and length == TILE}[label], (first, length)
    if label.startswith("straddling"):
        assert 0.3 * n < len(ref.dropped) < 0.7 * n
    if label == "geo-referenced at leaf 4":
        assert len(ref.dropped) == 0 and 0 < len(ref.counts) < n


@gpu
@pytest.mark.parametrize("label", LABELS)
def test_case(label):
    c = CASES[LABELS.index(label)]
    pts = c.make()
    first_out = first_records = ref = None
    for path in c.paths:
        cloud = upload(pts, path)
        records = records_of(cloud)
        if first_records is not None:
            assert np.array_equal(records, first_records, equal_nan=True), (label, path, "the upload paths hold different records")
        if label.startswith("lattice points"):
            assert not cloud.origin().any()  # (the denormals are records as they are)
        want = {**c.want, **plan_of_size(len(pts)), **(NO_BOX if path == "slice" else {})}
        out, ref = check("%s / %s" % (label, path), cloud, c.leaf, want, ref)
        if first_out is None:
            first_out, first_records = out, records
        else:  # the same records by another path: the same bits
            assert out.shape == first_out.shape and np.array_equal(out.view(np.uint32), first_out.view(np.uint32)), (label, path, "differs from", c.paths[0])
    assert_shape(label, len(pts), ref)


@gpu
def test_the_output_of_a_grid_downsampled_again():
    """a cloud the voxel grid made (no box: the reference's keys), downsampled at a coarser leaf"""
    first = sga.voxelgrid_sampling(sga.PointCloud(scan(200_000, 30)), 0.1)
    assert 2048 < first.size() <= 200_000
    check("grid of a grid", first, 0.5, {**NO_BOX, **plan_of_size(first.size())})
    geo = sga.voxelgrid_sampling(sga.PointCloud(geo_cloud()), 2.0)  # (2e6 m / 2 m: still inside the grid)
    assert geo.origin().any() and geo.size() > 2048
    check("grid of a geo-referenced grid", geo, 8.0, {**NO_BOX, **plan_of_size(geo.size())})


STATE_TILES = [1500, 1, 700, 1500]


def _state_clouds(ctx):
    clouds = {}
    for tiles in sorted(set(STATE_TILES + [300])):
        n = tiles * TILE - 5
        cloud = sga.PointCloud(scan(n, 40 + tiles), ctx=ctx)
        clouds[tiles] = (cloud, downsample_ref(records_of(cloud), cloud.origin(), 0.25))
    return clouds


@gpu
@pytest.mark.parametrize("stream_ordered", [False, True])
def test_status_words_are_reused_across_calls_of_one_context(stream_ordered):
    """One fresh context: a call of 1500 tiles (the status array is made for it), then 1 tile, then 700, then the first again — every call
    finds the words of the calls before it, tagged with older epochs, and must read them as 'nothing yet'."""
    ctx = sga.Context(0)
    ctx.set_stream_ordered(stream_ordered)
    clouds = _state_clouds(ctx)
    for k, tiles in enumerate(STATE_TILES):
        cloud, ref = clouds[tiles]
        check("context state %d: %d tiles%s" % (k, tiles, ", stream-ordered" if stream_ordered else ""), cloud, 0.25, {"tiles": tiles}, ref)
    ctx.set_stream_ordered(False)


@gpu
def test_epoch_wraps_at_2_30():
    """The reset of the status words after 2^30 - 1 calls of one context (about a day of an odometry service), reached through
    sga_debug_set_voxelgrid_epoch: four checks of different tile counts (two calls each) with the reset between the first and the second.

    Why no look-back after the reset can wait on a stale word (voxelgrid_run, ds_segments_kernel): a workgroup waits only while a
    predecessor's word carries another epoch than its launch's.  The call that finds epoch >= 2^30 - 1 zeroes the WHOLE status array with a
    memset enqueued on the context's stream before its kernels, and restarts at epoch 1; a zeroed word carries epoch 0, which no launch
    uses, so it reads as 'nothing yet' exactly like the words of a fresh array — and every predecessor a workgroup waits for has taken its
    tile before it (tiles are handed out in arrival order), so it publishes the launch's epoch without waiting for anybody.  The calls
    before the reset use 2^30 - 2 and 2^30 - 1, which fit the 30 bits of the tag and exceed every epoch a word of this context carries.
    The setter moves the epoch forwards only, so it cannot make an older word look current; that also lets the test read the epoch back."""
    ctx = sga.Context(0)
    clouds = _state_clouds(ctx)
    cloud, ref = clouds[1500]
    check("epoch wrap: before", cloud, 0.25, {"tiles": 1500}, ref)  # makes the status array: epochs 1 and 2
    ctx._set_voxelgrid_epoch(2**30 - 3)
    for k, tiles in enumerate([700, 1, 300, 1500]):  # epochs 2^30 - 2, 2^30 - 1 | 1, 2 | 3, 4 | 5, 6
        cloud, ref = clouds[tiles]
        check("epoch wrap %d: %d tiles" % (k, tiles), cloud, 0.25, {"tiles": tiles}, ref)
    with pytest.raises(sga.SgaError):
        ctx._set_voxelgrid_epoch(5)  # the epoch is 6: the counter did start again
    ctx._set_voxelgrid_epoch(6)
    with pytest.raises(sga.SgaError):
        ctx._set_voxelgrid_epoch(2**30)


def test_matrix_covers_every_regime():
    """(CPU) the plans the cases assert cover both key widths, the three key layouts, the three branches of the sort (and both of rocPRIM's
    algorithms in the last), both launches of the centroid kernel, and the look-back over more than one window — with both key types."""
    seen = set()
    for c in CASES:
        n = len(c.make()) if c.label.startswith(("size", "300000")) else None
        for path in c.paths:
            want = {**c.want, **(NO_BOX if path == "slice" else {})}
            if "key_bytes" not in want:
                continue
            layout = "reference" if not want["box"] else "short 32" if want["key_bytes"] == 4 else "short 64"
            seen.add(("layout", layout))
            if n is not None:
                size = plan_of_size(n)
                seen.add(("sort", size["sort"], want["key_bytes"]))
                seen.add(("speculative", size["speculative"], want["key_bytes"]))
                seen.add(("onesweep", n > 1 << 20, want["key_bytes"]))
                seen.add(("tiles > 64", size["tiles"] > 64, want["key_bytes"]))
    want_seen = {("layout", v) for v in ("reference", "short 32", "short 64")}
    for kb in (4, 8):
        want_seen |= {("sort", s, kb) for s in (0, 1, 2)} | {("speculative", v, kb) for v in (False, True)} | {("onesweep", True, kb), ("tiles > 64", True, kb)}
    assert want_seen <= seen, sorted(want_seen - seen, key=str)
    totals = [c.want.get("total") for c in CASES]
    assert 31 in totals and 32 in totals and any(isinstance(t, Between) and 32 < t.lo and t.hi < 63 for t in totals), totals
    src = open(__file__).read()
    for needed in ("sga_debug_set_voxelgrid_epoch", "stream_ordered", "grid of a grid"):
        assert needed in src

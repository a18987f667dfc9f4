"""tests/map_contents_ref.py (what a voxel map holds after insert(), restated in numpy, float64) pinned on the CPU:

  * against the oracle: the eight-step C1 sequence of test_incremental_voxelmap_matches_oracle on the fp32-rounded clouds for three
    (leaf, horizon, clear_cycle), against orc.VoxelMap and orc.FlatMap: coordinates, counts and sizes equal after every step, means,
    points and covariances within 1e-12 relative;
  * against the compiled reference (ref.VoxelMap, ref.FlatMap) where it is there: the same;
  * the designed sequences of tests/test_map_contents_gpu.py (built here, shared with it) give the answers written out by hand;
  * no point of a designed sequence is ambiguous, and the random ones stay under their cap, by the restatement alone.

A sequence is a list of steps: a cloud (the device holds fl32(p - o) for the origin o STATED here — frame_origin(), the rule of the
project's device frames, or a value written out —, which the GPU tests check against the upload's choice), fp32 normals and covariances,
a pose, and the LRU pair set before the insert where it changes.
"""
import numpy as np
import pytest

import map_contents_ref as mc

AMBIGUOUS_CAP = 0.01  # share of a random sequence's points that may be removed as ambiguous; none in a designed one
LIMIT = 1 << 20


# ---- poses -----------------------------------------------------------------------------------------------------------------------------
def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def rot(axis, ang):
    a = np.asarray(axis, dtype=np.float64)
    k = a / np.linalg.norm(a)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


IDENTITY = np.eye(4)
QUARTER_Z = pose([[0, -1, 0], [1, 0, 0], [0, 0, 1]], [0.25, -0.5, 2.0])    # (x, y, z) -> (-y, x, z) + a dyadic translation
PERMUTED = pose([[0, 0, -1], [-1, 0, 0], [0, 1, 0]], [-1.5, 0.75, 4.0])    # (x, y, z) -> (-z, -x, y) + a dyadic translation
EXACT_POSES = {"identity": IDENTITY, "quarter_z": QUARTER_Z, "permuted": PERMUTED}


def unposed(T, y):
    """p with T p = y, exactly, for the exact poses and dyadic y"""
    T = np.asarray(T, dtype=np.float64)
    return (np.asarray(y, dtype=np.float64).reshape(-1, 3) - T[:3, 3]) @ T[:3, :3]


# ---- attributes ------------------------------------------------------------------------------------------------------------------------
def designed_covs(n):
    """anisotropic, symmetric positive definite (diagonally dominant), dyadic: R C R^T differs from R^T C R far above any bound"""
    c = np.zeros((n, 3, 3), np.float32)
    i = np.arange(n)
    c[:, 0, 0], c[:, 1, 1], c[:, 2, 2] = (1 + i % 3) / 64.0, 1 / 16.0, 1 / 4.0
    c[:, 0, 1] = c[:, 1, 0] = 1 / 128.0
    c[:, 0, 2] = c[:, 2, 0] = -1 / 256.0
    c[:, 1, 2] = c[:, 2, 1] = 1 / 512.0
    return c


def designed_normals(n):
    table = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0.70710677], [0.6, 0.0, -0.8]], np.float32)
    return table[np.arange(n) % len(table)]


def random_covs(rng, n):
    a = rng.normal(size=(n, 3, 3)) * 0.1
    return (a @ a.transpose(0, 2, 1) + 1e-3 * np.eye(3)).astype(np.float32)


# ---- sequences (shared with tests/test_map_contents_gpu.py) ---------------------------------------------------------------------------------
def frame_origin(points):
    """the origin of a cloud's device frame as the project states it: per axis 128 * round-half-even(centre / 128) of the box of the finite
    coordinates, 0 where there is none.  0 for every cloud whose box is centred within 64 m of the origin."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    o = np.zeros(3)
    for a in range(3):
        x = p[np.isfinite(p[:, a]), a]
        if len(x):
            o[a] = 128.0 * np.rint(0.5 * (x.min() + x.max()) / 128.0)
    return o + 0.0  # (no -0.0)


class Step:
    def __init__(self, points, T=None, origin=None, lru=None, covs=None, normals=None):
        self.points = np.asarray(points).reshape(-1, 3)
        assert self.points.dtype in (np.float32, np.float64)
        self.origin = frame_origin(self.points) if origin is None else np.asarray(origin, dtype=np.float64)
        self.T, self.lru = T, lru
        n = len(self.points)
        self.covs = designed_covs(n) if covs is None else np.asarray(covs, np.float32).reshape(n, 3, 3)
        self.normals = designed_normals(n) if normals is None else np.asarray(normals, np.float32).reshape(n, 3)

    def records(self):
        """what the device holds: fl32(p - o), as doubles"""
        with np.errstate(invalid="ignore", over="ignore"):
            return (self.points.astype(np.float64) - self.origin).astype(np.float32).astype(np.float64)

    def without(self, mask):
        keep = ~np.asarray(mask, bool)
        return Step(self.points[keep], self.T, self.origin, self.lru, self.covs[keep], self.normals[keep])


class Seq:
    """expect: per step (or None) a dict with any of coords [(x, y, z), ...] in voxel-id order, counts [...], size, and for flat maps
    slots [[(insert, index of the point), ...] per voxel]; written by hand"""

    def __init__(self, name, leaf, steps, lru=None, min_sq=0.01, max_points=10, expect=None, random=False):
        self.name, self.leaf, self.steps, self.lru, self.min_sq, self.max_points = name, float(leaf), steps, lru, float(min_sq), int(max_points)
        self.expect = expect or [None] * len(steps)
        self.random = random
        assert len(self.expect) == len(steps)


def restate(seq, kind, normals=True, covs=True):
    """the restatement after every step of the sequence -> yields (step number, step, map, (dropped, kept, ambiguous))"""
    m = mc.Map(seq.leaf, kind, seq.min_sq, seq.max_points)
    if seq.lru is not None:
        m.set_lru(*seq.lru)
    for k, s in enumerate(seq.steps):
        if s.lru is not None:
            m.set_lru(*s.lru)
        cv = s.covs.astype(np.float64) if (covs or kind == mc.GAUSSIAN) else None
        nr = s.normals.astype(np.float64) if (normals and kind == mc.FLAT) else None
        yield k, s, m, m.insert(s.records(), s.origin, s.T, nr, cv)


def cleaned(seq, kind):
    """the sequence without its ambiguous points (map_contents_ref.py; decided on the inputs, before either side sees them) -> (sequence,
    number removed, number of points).  Removing a point changes what the later ones meet, so the pass is repeated until none is left."""
    total = sum(len(s.points) for s in seq.steps)
    removed = 0
    for _ in range(4):
        masks = [info[2] for _, _, _, info in restate(seq, kind)]
        n = int(sum(m.sum() for m in masks))
        if n == 0:
            return seq, removed, total
        removed += n
        seq = Seq(seq.name, seq.leaf, [s.without(m) for s, m in zip(seq.steps, masks)], seq.lru, seq.min_sq, seq.max_points, seq.expect, seq.random)
    raise AssertionError("ambiguous points keep appearing in %s" % seq.name)


def f32(points):
    return np.asarray(points, dtype=np.float32).reshape(-1, 3)


# 1. faces and octants ------------------------------------------------------------------------------------------------------------------------
# grid coordinate -> voxel, written out: a value on a face belongs to the voxel above it, -0.0 to voxel 0
FACE_AXIS = {1: {"centre": (1.5, 1), "face": (1.0, 1)}, -1: {"centre": (-1.5, -2), "face": (-1.0, -1)}}
FACE_LEAVES = [0.5, 1.0, 2.0]


def face_grid_points():
    """(grid coordinates (n, 3), voxel (n, 3)): in each octant the centre of a voxel, a point on a face, on an edge and on a corner; then
    points with +0.0 and -0.0 coordinates"""
    g, c = [], []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                for on in ((), (0,), (1, 2), (0, 1, 2), (2,), (0, 2)):
                    pick = [FACE_AXIS[s]["face" if a in on else "centre"] for a, s in enumerate((sx, sy, sz))]
                    g.append([p[0] for p in pick])
                    c.append([p[1] for p in pick])
    for z in ([0.0, 0.5, 0.5], [-0.0, 0.5, 0.5], [0.5, -0.0, -0.0], [-0.0, -0.0, 0.0], [-0.5, 0.0, -0.0]):
        g.append(z)
        c.append([-1 if v == -0.5 else 0 for v in z])
    return np.array(g), np.array(c, dtype=np.int64)


def first_appearance(coords):
    """(coordinates in the order of their first appearance, how often each appears): the voxel ids and counts of a Gaussian map"""
    order, count = [], {}
    for c in map(tuple, np.asarray(coords).tolist()):
        if c not in count:
            order.append(c)
        count[c] = count.get(c, 0) + 1
    return order, [count[c] for c in order]


def case_faces(leaf, pose_name):
    """dyadic points on faces, edges and corners of the voxel grid, in all eight octants, posed exactly.  The cloud holds T^-1 y for the grid
    points y, so the posed points are the grid points under every pose and the hand-written voxels hold for all three."""
    g, c = face_grid_points()
    T = EXACT_POSES[pose_name]
    p = g * leaf if pose_name == "identity" else unposed(T, g * leaf)  # (the identity keeps the -0.0 coordinates as they are)
    assert np.array_equal(p.astype(np.float32).astype(np.float64), p)
    order, counts = first_appearance(c)
    return Seq("faces leaf %g %s" % (leaf, pose_name), leaf, [Step(f32(p), T)], expect=[dict(coords=order, counts=counts)])


def case_interior(pose_name, leaf=0.3):
    """leaf 0.3 has no representable face but 0: interior points only, a quarter of a voxel off the centres"""
    k = np.array([[i, j, l] for i in (-3, 0, 2) for j in (-1, 0, 4) for l in (-2, 1)], dtype=np.float64)
    y = ((k + 0.25) * leaf).astype(np.float32).astype(np.float64)
    T = EXACT_POSES[pose_name]
    p = unposed(T, y).astype(np.float32)
    order, counts = first_appearance(k.astype(np.int64))
    return Seq("interior leaf %g %s" % (leaf, pose_name), leaf, [Step(p, T)], expect=[dict(coords=order, counts=counts)])


# 2. the range edge ---------------------------------------------------------------------------------------------------------------------------
EXTREMES = [1048576.0, -1048575.5, 2147483648.0, -2147483648.0, 3e38, -3e38, np.inf, -np.inf, np.nan]  # every one of them is dropped
ORDINARY = [[0.5, 0.5, 0.5], [1.5, 0.5, 0.5]]                                                        # voxels 0 and 1


def edge_first_cloud():
    """(points, voxels by hand): two ordinary voxels, then on every axis the last coordinates the key holds: 1048575.5 -> 2^20 - 1 and
    -1048575.0 -> -(2^20 - 1)"""
    pts, vox = [list(p) for p in ORDINARY], [(0, 0, 0), (1, 0, 0)]
    for a in range(3):
        for value, c in ((1048575.5, LIMIT - 1), (-1048575.0, -(LIMIT - 1))):
            p, v = [0.5, 0.5, 0.5], [0, 0, 0]
            p[a], v[a] = value, c
            pts.append(p)
            vox.append(tuple(v))
    return pts, vox


def edge_extreme_clouds():
    """for the one-shot cloud: per axis and extreme value an ordinary point, the extreme, an ordinary point"""
    out = []
    for a in range(3):
        for value in EXTREMES:
            p = [0.5, 0.5, 0.5]
            p[a] = value
            out.append(np.array([ORDINARY[0], p, ORDINARY[1]], dtype=np.float32))
    return out


def case_range_edge():
    """leaf 1, identity.  Every extreme point comes in a cloud of its own — the frame of a cloud follows its box, and an ordinary point beside
    3e38 would not survive the upload — and is dropped: the map keeps its eight voxels and their contents.  After the extremes of an axis
    the two ordinary points are inserted again."""
    pts, vox = edge_first_cloud()
    steps, expect, hits = [Step(f32(pts))], [dict(coords=vox, counts=[1] * len(vox))], 1
    for a in range(3):
        for value in EXTREMES:
            p = [0.5, 0.5, 0.5]
            p[a] = value
            steps.append(Step(f32([p])))
            expect.append(dict(coords=vox, counts=[hits, hits] + [1] * (len(vox) - 2)))
        hits += 1
        steps.append(Step(f32(ORDINARY)))
        expect.append(dict(coords=vox, counts=[hits, hits] + [1] * (len(vox) - 2)))
    return Seq("range edge", 1.0, steps, lru=(1000, 1000), expect=expect)


def one_shot_edge_cloud():
    """(points, coords, counts by hand): everything of the range-edge case in ONE cloud, for the one-shot maps"""
    pts, vox = edge_first_cloud()
    extra = np.concatenate(edge_extreme_clouds())
    n = len(extra) // 3
    return np.concatenate([f32(pts), extra]), vox, [1 + n, 1 + n] + [1] * (len(vox) - 2)


# 3. launch edges -----------------------------------------------------------------------------------------------------------------------------
def grid_voxel(i):
    """voxel number i of the designed grids: distinct for i < 4096, on both sides of 0 on x and y"""
    return (i % 64 - 32, i // 64 - 16, 0)


def voxel_points(ids, leaf, offset):
    return np.array([[(c + o) * leaf for c, o in zip(grid_voxel(i), offset)] for i in ids], dtype=np.float64)


LAUNCH_CLOUDS = [1, 255, 256, 257, 2049]


def launch_cloud(n):
    """n dyadic points over min(n, 257) voxels: 1, 255, 256, 257 voxels of one point, or 257 voxels of seven or eight points"""
    i = np.arange(n)
    return voxel_points(i % 257, 1.0, (0.5, 0.25, 0.75)) + np.stack([(i // 257) / 64.0, np.zeros(n), np.zeros(n)], 1)


def case_launch_edges():
    """one map, five inserts of 1, 255, 256, 257 and 2049 points touching 1, 255, 256, 257 and 257 voxels, under the three exact poses in turn"""
    steps, poses = [], [IDENTITY, QUARTER_Z, PERMUTED]
    for k, n in enumerate(LAUNCH_CLOUDS):
        T = poses[k % 3]
        steps.append(Step(f32(unposed(T, launch_cloud(n))), T))
    return Seq("launch edges", 1.0, steps)


# 4. growth -----------------------------------------------------------------------------------------------------------------------------------
GROWTH_TOTALS = [200, 511, 512, 513, 1023, 1024, 1025, 2100]  # voxels after each insert


def case_growth():
    """The hash table starts with 1024 slots (200 voxels) and is rebuilt when 2 n > 1024: at 513.  The per-voxel arrays start with room for
    1024 voxels and are regrown and copied at 1025, and again at 2100 (with the table).  Inserts that add ONE voxel also touch voxels 0,
    511 and 1023 where they exist, so state that was copied is read back.  Gaussian and flat maps (max 10 points, 0.1 apart: every point
    is kept until the voxel is full)."""
    steps, expect, have, visit = [], [], 0, 0
    for total in GROWTH_TOTALS:
        ids = list(range(have, total))
        pts = voxel_points(ids, 1.0, (0.5, 0.5, 0.5))
        if total - have == 1:
            visit += 1
            old = [v for v in (0, 511, 1023) if v < have]
            pts = np.concatenate([voxel_points(old, 1.0, (0.5 - visit / 8.0, 0.5, 0.5 + visit / 16.0)), pts])
        steps.append(Step(f32(pts)))
        expect.append(dict(size=total))
        have = total
    return Seq("growth", 1.0, steps, expect=expect)


# 5. running sums -------------------------------------------------------------------------------------------------------------------------------
def case_running_sums():
    """one voxel, (3, -2, 1) at leaf 1, hit in 12 consecutive inserts by 1, 2, 3 and 17 points under 12 general rotations; the points are
    T^-1 of targets within 0.3 of the voxel's centre, so none is near a face"""
    rng = np.random.default_rng(5)
    steps, total = [], 0
    for k in range(12):
        n = (1, 2, 3, 17)[k % 4]
        T = pose(rot(rng.normal(size=3), 0.3 + 0.2 * k), rng.uniform(-5, 5, 3))
        y = np.array([3.5, -1.5, 1.5]) + rng.uniform(-0.3, 0.3, (n, 3))
        steps.append(Step(f32((y - T[:3, 3]) @ T[:3, :3]), T))
        total += n
    return Seq("running sums", 1.0, steps, expect=[None] * 11 + [dict(coords=[(3, -2, 1)], counts=[total])])


# 6. creation order -------------------------------------------------------------------------------------------------------------------------------
def case_creation_order():
    """first appearances in DESCENDING order of the hash key (z, then y, then x), revisits in between: ids follow the cloud, not the sort"""
    seen = [(2, 2, 2), (1, 2, 2), (2, 2, 2), (2, 1, 2), (-1, -1, 1), (1, 2, 2), (0, 0, 0), (2, 2, 2), (5, 0, -1), (-1, -1, 1), (-3, -3, -3), (2, 1, 2), (-4, -3, -3)]
    pts = [[c + 0.5 + 0.125 * (i % 3) for c in v] for i, v in enumerate(seen)]
    coords = [(2, 2, 2), (1, 2, 2), (2, 1, 2), (-1, -1, 1), (0, 0, 0), (5, 0, -1), (-3, -3, -3), (-4, -3, -3)]
    second = [(7, 7, 7), (0, 0, 0), (6, 7, 7), (-4, -3, -3), (7, 7, 7)]
    pts2 = [[c + 0.25 for c in v] for v in second]
    return Seq("creation order", 1.0, [Step(f32(pts)), Step(f32(pts2))],
               expect=[dict(coords=coords, counts=[3, 2, 2, 2, 1, 1, 1, 1]), dict(coords=coords + [(7, 7, 7), (6, 7, 7)], counts=[3, 2, 2, 2, 2, 1, 1, 2, 2, 1])])


# 7. LRU ------------------------------------------------------------------------------------------------------------------------------------------
LRU_PAIRS = [(0, 1), (1, 1), (1, 2), (2, 3), (0, 4), (2 ** 32 - 1, 1)]


def window_cloud(k):
    """the voxels (k, 0, 0), (k + 1, 0, 0), (k + 2, 0, 0), one point each"""
    return f32([[k + j + 0.5, 0.25 + k / 32.0, 0.5] for j in range(3)])


def lru_steps():
    """nine inserts over a window that slides by one voxel, an EMPTY cloud after the fifth: voxel (j, 0, 0) is last touched by insert j"""
    steps = [Step(window_cloud(k)) for k in range(9)]
    steps.insert(5, Step(np.zeros((0, 3), np.float32)))
    return steps


def case_lru(horizon, cycle):
    return Seq("lru (%d, %d)" % (horizon, cycle), 1.0, lru_steps(), lru=(horizon, cycle), expect=[dict(size=n) for n in LRU_SIZES[(horizon, cycle)]])


# sizes after each of the ten steps, by hand.  Insert k (counter k before it; the empty cloud is step 5) touches three voxels, two of them new
# after the first; a sweep at counter c keeps lru >= c - horizon.
LRU_SIZES = {
    (0, 1): [0] * 10,                              # every sweep removes everything, the voxels just touched included
    (1, 1): [3, 3, 3, 3, 3, 0, 3, 3, 3, 3],        # only the voxels of the last insert survive; the empty cloud's sweep removes them too
    (1, 2): [3, 3, 4, 3, 4, 0, 3, 3, 4, 3],        # sweeps at counters 2, 4, 6 (the empty cloud's), 8, 10
    (2, 3): [3, 4, 4, 5, 6, 3, 4, 5, 4, 5],        # sweeps at counters 3, 6 (the empty cloud's), 9
    (0, 4): [3, 4, 5, 0, 3, 3, 4, 0, 3, 4],        # sweeps at counters 4 and 8 remove everything
    (2 ** 32 - 1, 1): [3, 4, 5, 6, 7, 7, 8, 9, 10, 11],  # a sweep after every insert that removes nothing: lru + horizon does not wrap
}


def case_lru_changing():
    """set_lru between inserts: (2, 3) for four inserts, (1, 2) before the fifth, (0, 4) before the eighth"""
    steps = lru_steps()
    steps[4].lru, steps[7].lru = (1, 2), (0, 4)
    return Seq("lru changing", 1.0, steps, lru=(2, 3), expect=[dict(size=n) for n in [3, 4, 4, 5, 6, 0, 3, 0, 3, 4]])


def case_lru_last():
    """(1, 1): A, B, C are created; the next insert touches A and B, so its sweep removes ONLY THE LAST voxel; then the survivors are hit
    again and D is created behind them"""
    A, B, C, D = [0.5, 0.5, 0.5], [4.5, 0.5, 0.5], [8.5, 0.5, 0.5], [-3.5, 0.5, 0.5]
    steps = [Step(f32([A, B, C])), Step(f32([B, A, A])), Step(f32([D, B, A]))]
    return Seq("lru last", 1.0, steps, lru=(1, 1), expect=[dict(coords=[(0, 0, 0), (4, 0, 0), (8, 0, 0)], counts=[1, 1, 1]), dict(coords=[(0, 0, 0), (4, 0, 0)], counts=[3, 2]),
                                                              dict(coords=[(0, 0, 0), (4, 0, 0), (-4, 0, 0)], counts=[4, 3, 1])])


# 8. far frame -------------------------------------------------------------------------------------------------------------------------------------
FAR_CENTRE = np.array([100000.0, 200100.0, 300.0])
FAR_ORIGIN = np.array([99968.0, 200064.0, 256.0])  # 128 * round(centre / 128): 781.25 -> 781, 1563.28 -> 1563, 2.34 -> 2


def far_cloud(seed, n=300):
    rng = np.random.default_rng(seed)
    p = rng.uniform([-20, -20, -2], [20, 20, 2], (n, 3))
    p[0], p[1] = [-20, -20, -2], [20, 20, 2]  # the box is centred on FAR_CENTRE whatever the seed
    return p + FAR_CENTRE


def case_far_frame():
    """float64 clouds around (1e5, 2e5, 300): the records are relative to a non-zero origin; poses with general rotations about 3 km away"""
    Ts = [pose(rot([0.2, -0.1, 1.0], 0.7), [2000.0, -2200.0, 40.0]), pose(rot([0.1, 0.3, 1.0], 0.71), [2001.5, -2199.0, 40.2])]
    steps = [Step(far_cloud(11 + k), T, FAR_ORIGIN, covs=random_covs(np.random.default_rng(21 + k), 300)) for k, T in enumerate(Ts)]
    return Seq("far frame", 1.0, steps, random=True)


# 9. a random posed scene -----------------------------------------------------------------------------------------------------------------------------
SCENE_LEAVES = [0.5, 1.0, 2.0]
_scans = {}


def scene_scans():
    if not _scans:
        for k in range(3):
            rng = np.random.default_rng(100 + k)
            _scans[k] = (rng.uniform([-20, -20, -2], [20, 20, 2], (2000, 3)).astype(np.float32), random_covs(rng, 2000), rng.normal(size=(2000, 3)).astype(np.float32))
    return _scans


def case_scene(leaf):
    """three scans of 2000 points in [-20, 20]^2 x [-2, 2] with random SPD covariances, eight inserts along a curved path, LRU (2, 3)"""
    scans = scene_scans()
    steps = []
    for k in range(8):
        p, c, nr = scans[k % 3]
        steps.append(Step(p, pose(rot([0.1, 0.2, 1.0], 0.05 * k), [6.0 * k, -2.0 * k, 0.1 * k]), covs=c, normals=nr))
    return Seq("scene leaf %g" % leaf, leaf, steps, lru=(2, 3), random=True)


# 10. flat maps: the keep rule ---------------------------------------------------------------------------------------------------------------------
KEEP_MAX = [1, 10, 16]
KEEP_MIN_SQ = [0.0, 0.0625, 0.01]
# voxel (0, 0, 0): b is EXACTLY 0.25 from a; c is 2^-20 nearer than 0.25 to b; the fourth is a again
KEEP_A, KEEP_B, KEEP_C = [0.25, 0.5, 0.5], [0.5, 0.5, 0.5], [0.75 - 2.0 ** -20, 0.5, 0.5]
KEEP_FIRST = {0.0: [0, 1, 2, 3], 0.0625: [0, 1], 0.01: [0, 1, 2]}  # which of a, b, c, a voxel (0, 0, 0) keeps, by hand: d2 < min_sq rejects


def keep_lattice():
    """20 points of voxel (2, 0, 0) on a lattice of 0.25: every pair is at least 0.25 apart, so only max_points stops them"""
    return [[2 + 0.25 * (i % 4), 0.25 * ((i // 4) % 4), 0.5 + 0.25 * (i // 16)] for i in range(20)]


def case_keep(max_points, min_sq):
    pts = [KEEP_A, KEEP_B, KEEP_C, KEEP_A] + keep_lattice()
    first = KEEP_FIRST[min_sq][:max_points]
    slots = [[(0, i) for i in first], [(0, 4 + i) for i in range(min(20, max_points))]]
    return Seq("keep %d %g" % (max_points, min_sq), 1.0, [Step(f32(pts))], min_sq=min_sq, max_points=max_points,
               expect=[dict(coords=[(0, 0, 0), (2, 0, 0)], counts=[len(s) for s in slots], slots=slots)])


# 11. flat maps: order ---------------------------------------------------------------------------------------------------------------------------------
def case_exclusive():
    """100 voxels, three mutually exclusive points each (0.03125 apart along x, min_sq 0.01), at positions j, 100 + j and 200 + j of the cloud, the
    voxels in descending key order: the earliest in the CLOUD wins, which the sort must not disturb"""
    vox = [grid_voxel(4000 - 7 * j) for j in range(100)]
    pts = [[v[0] + 0.5 + 0.03125 * r, v[1] + 0.5, v[2] + 0.5] for r in range(3) for v in vox]
    return Seq("exclusive", 1.0, [Step(f32(pts))], expect=[dict(coords=vox, counts=[1] * 100, slots=[[(0, j)] for j in range(100)])])


def fill_lattice(i):
    """point i of a lattice of 0.125 in voxel (1, -1, 0): any two are at least 0.125 apart (d2 0.0156 > 0.01)"""
    return [1 + 0.125 * (i % 8), -1 + 0.125 * ((i // 8) % 8), 0.25 + 0.125 * (i // 64)]


def case_fill():
    """a cell filled over three inserts under the three exact poses: 7 + 5 + 9 candidates into 16 slots.  The second insert repeats two
    points of the first (rejected against points kept under another pose), so 7 + 3 are kept and the third adds 6 of its 9."""
    first, second, third = list(range(7)), [7, 2, 8, 5, 9], list(range(10, 19))
    steps = [Step(f32(unposed(T, [fill_lattice(i) for i in ids])), T) for ids, T in ((first, IDENTITY), (second, QUARTER_Z), (third, PERMUTED))]
    s1 = [(0, i) for i in range(7)]
    s2 = s1 + [(1, 0), (1, 2), (1, 4)]
    s3 = s2 + [(2, i) for i in range(6)]
    return Seq("fill", 1.0, steps, max_points=16, expect=[dict(coords=[(1, -1, 0)], counts=[len(s)], slots=[s]) for s in (s1, s2, s3)])


# 12. flat maps: attributes ---------------------------------------------------------------------------------------------------------------------------
def case_attributes():
    """400 random points in a box of 6 m under two general poses, normals and anisotropic covariances: R n without the translation, R C R^T"""
    rng = np.random.default_rng(31)
    steps = []
    for k in range(2):
        p = rng.uniform(-3, 3, (400, 3)).astype(np.float32)
        nr = rng.normal(size=(400, 3))
        nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(np.float32)
        steps.append(Step(p, pose(rot([1.0, -0.4, 0.3], 0.9 + k), [1.5 + k, -2.5, 0.75]), covs=random_covs(rng, 400), normals=nr))
    return Seq("attributes", 1.0, steps, random=True)


# 13. flat maps: LRU refresh ---------------------------------------------------------------------------------------------------------------------------
def case_lru_refresh():
    """max 2 points, 0.25 apart, LRU (1, 1).  A holds two points, B and C one.  The second insert offers A a third point (rejected: full)
    and C a duplicate (rejected: too near): both are touched and survive the sweep, B is not and goes."""
    A1, A2, A3, B, C = [0.25, 0.5, 0.5], [0.75, 0.5, 0.5], [0.5, 0.125, 0.5], [4.5, 0.5, 0.5], [8.5, 0.5, 0.5]
    steps = [Step(f32([A1, B, A2, C])), Step(f32([A3, C])), Step(f32([B]))]
    return Seq("lru refresh", 1.0, steps, lru=(1, 1), min_sq=0.0625, max_points=2, expect=[
        dict(coords=[(0, 0, 0), (4, 0, 0), (8, 0, 0)], counts=[2, 1, 1], slots=[[(0, 0), (0, 2)], [(0, 1)], [(0, 3)]]),
        dict(coords=[(0, 0, 0), (8, 0, 0)], counts=[2, 1], slots=[[(0, 0), (0, 2)], [(0, 3)]]),
        dict(coords=[(4, 0, 0)], counts=[1], slots=[[(2, 0)]])])


# 14. one-shot maps --------------------------------------------------------------------------------------------------------------------------------
def one_shot_steps():
    """{name: (leaf, step)}: the clouds of the designed sequences, each for a one-shot map of its own"""
    out = {}
    for leaf in FACE_LEAVES:
        out["faces %g" % leaf] = (leaf, case_faces(leaf, "identity").steps[0])
    out["range edge"] = (1.0, Step(one_shot_edge_cloud()[0]))
    for n in LAUNCH_CLOUDS:
        out["launch %d" % n] = (1.0, Step(f32(launch_cloud(n))))
    out["creation order"] = (1.0, case_creation_order().steps[0])
    far = case_far_frame().steps[0]
    out["far frame"] = (1.0, Step(far.points, None, far.origin, covs=far.covs))
    return out


GAUSSIAN_DESIGNED = ([lambda l=l, p=p: case_faces(l, p) for l in FACE_LEAVES for p in EXACT_POSES] + [lambda p=p: case_interior(p) for p in EXACT_POSES] +
                     [case_range_edge, case_launch_edges, case_growth, case_running_sums, case_creation_order, case_lru_changing, case_lru_last] + [lambda hc=hc: case_lru(*hc) for hc in LRU_PAIRS])
FLAT_DESIGNED = [lambda m=m, q=q: case_keep(m, q) for m in KEEP_MAX for q in KEEP_MIN_SQ] + [case_exclusive, case_fill, case_lru_refresh, case_growth]
GAUSSIAN_RANDOM = [case_far_frame] + [lambda l=l: case_scene(l) for l in SCENE_LEAVES]
FLAT_RANDOM = [case_attributes]


# ---- the hand-written answers ---------------------------------------------------------------------------------------------------------------
def check_expectation(seq, k, m, want):
    if want is None:
        return
    label = (seq.name, k)
    if "size" in want:
        assert m.size() == want["size"], label + (m.size(), want["size"])
    if "coords" in want:
        assert m.coords().tolist() == [list(c) for c in want["coords"]], label
    if "counts" in want:
        assert m.counts().tolist() == list(want["counts"]), label + (m.counts().tolist(),)
    if "slots" in want and m.kind == mc.FLAT:
        src = m.slots()["source"].tolist()
        assert src == [list(s) for v in want["slots"] for s in v], label + (src,)


@pytest.mark.parametrize("make", GAUSSIAN_DESIGNED)
def test_designed_gaussian_sequences_give_the_hand_written_answers(make):
    seq = make()
    for k, s, m, (drop, kept, amb) in restate(seq, mc.GAUSSIAN):
        assert not amb.any(), (seq.name, k, np.flatnonzero(amb))
        assert np.array_equal(kept, ~drop)
        check_expectation(seq, k, m, seq.expect[k])
        ms, cs = m.means()[:2]
        assert np.isfinite(ms).all() and np.isfinite(cs).all(), (seq.name, k)


@pytest.mark.parametrize("make", FLAT_DESIGNED)
def test_designed_flat_sequences_give_the_hand_written_answers(make):
    seq = make()
    for k, s, m, (drop, kept, amb) in restate(seq, mc.FLAT):
        assert not amb.any(), (seq.name, k, np.flatnonzero(amb))
        check_expectation(seq, k, m, seq.expect[k])


def test_range_edge_drops_by_hand():
    """the first cloud keeps every point, every cloud of one point drops it; the one-shot cloud (an ordinary point either side of every
    extreme) gives the same voxels"""
    seq = case_range_edge()
    for k, s, m, (drop, kept, amb) in restate(seq, mc.GAUSSIAN):
        assert drop.tolist() == ([False] * 8 if k == 0 else [True] if len(s.points) == 1 else [False, False]), k
    pts, vox, counts = one_shot_edge_cloud()
    m, drop = mc.one_shot(pts.astype(np.float64), np.zeros(3), designed_covs(len(pts)), 1.0)
    assert m.coords().tolist() == [list(v) for v in vox] and m.counts().tolist() == counts and int(drop.sum()) == 3 * len(EXTREMES)
    assert np.isfinite(m.means()[0]).all()


def test_lru_sweeps_cover_their_edges():
    """over the LRU sequences a sweep removes nothing, everything, only voxel 0 and only the last voxel; lru + horizon == counter (kept) and
    == counter - 1 (removed) both occur at one sweep; after "everything" an insert starts from an empty map"""
    seen = set()
    for seq in [case_lru(h, c) for h, c in LRU_PAIRS] + [case_lru_changing(), case_lru_last()]:
        m = mc.Map(seq.leaf)
        m.set_lru(*seq.lru)
        for s in seq.steps:
            if s.lru is not None:
                m.set_lru(*s.lru)
            was_empty = m.size() == 0 and m.inserts > 0
            m.insert(s.records(), s.origin, s.T, None, s.covs)
            if was_empty and len(s.points) > 0:
                seen.add("insert into an emptied map")
            for counter, horizon, lrus, removed in m.sweeps[-1:] if m.sweeps and m.sweeps[-1][0] == m.counter else []:
                V = len(lrus)
                if V == 0:
                    continue
                if not removed.any():
                    seen.add("nothing")
                if removed.all():
                    seen.add("everything")
                if V > 1 and removed[0] and not removed[1:].any():
                    seen.add("only voxel 0")
                if V > 1 and removed[-1] and not removed[:-1].any():
                    seen.add("only the last")
                if ((lrus + horizon == counter) & ~removed).any() and ((lrus + horizon == counter - 1) & removed).any():
                    seen.add("both sides of the boundary")
                if len(s.points) == 0 and removed.any():
                    seen.add("an empty cloud sweeps")
    assert seen == {"nothing", "everything", "only voxel 0", "only the last", "both sides of the boundary", "an empty cloud sweeps", "insert into an emptied map"}, seen


def test_covariances_tell_the_rotation_from_its_transpose():
    """R C R^T against R^T C R on the designed covariances under the poses of the running sums: the difference is far above the fp32 bound"""
    seq = case_running_sums()
    for s in seq.steps:
        R = np.asarray(s.T)[:3, :3]
        c = s.covs.astype(np.float64)
        assert np.abs(R @ c @ R.T - R.T @ c @ R).max() > 1e-3


# ---- ambiguity on the committed inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("make", GAUSSIAN_RANDOM + FLAT_RANDOM)
def test_random_sequences_stay_under_the_cap_of_ambiguous_points(make):
    seq = make()
    for kind in ((mc.FLAT,) if make in FLAT_RANDOM else (mc.GAUSSIAN, mc.FLAT)):
        _, removed, total = cleaned(seq, kind)
        assert removed <= AMBIGUOUS_CAP * total, (seq.name, kind, removed, total)
        assert removed == 0, (seq.name, kind, removed)  # the committed seeds: none at all


def test_one_shot_clouds_have_no_ambiguous_point():
    """at the identity every cloud of the one-shot tests is exact or clear of the faces; the range-edge cloud gives the hand-written voxels"""
    for name, (leaf, step) in one_shot_steps().items():
        assert not mc.near_face(step.records(), step.origin, None, leaf).any(), name
        m, drop = mc.one_shot(step.records(), step.origin, step.covs.astype(np.float64), leaf)
        assert np.isfinite(m.means()[0]).all() and np.isfinite(m.means()[1]).all() and m.size() > 0, name
        assert drop.any() == (name == "range edge"), name


def test_far_frame_origin_is_the_stated_one():
    lo, hi = far_cloud(11).min(0), far_cloud(11).max(0)
    assert np.array_equal(128.0 * np.rint(0.5 * (lo + hi) / 128.0), FAR_ORIGIN)
    rec = case_far_frame().steps[0].records()
    assert np.abs(rec).max() < 128.0


def test_exactness_rule():
    """dyadic points under the exact poses are exact, also on a face; a general rotation is not; a point within delta of a face is ambiguous
    only when it is not exact"""
    g, _ = face_grid_points()
    for T in EXACT_POSES.values():
        assert mc.exact_points(unposed(T, g), np.zeros(3), T).all()
        assert not mc.near_face(unposed(T, g), np.zeros(3), T, 1.0).any()
    T = pose(rot([0.1, 0.2, 1.0], 0.3), [0.1, 0.2, 0.3])
    p = (np.array([[1.0, 1.5, 1.5], [1.5, 1.5, 1.5]]) - T[:3, 3]) @ T[:3, :3]  # lands within rounding of the face x = 1, and mid-voxel
    assert not mc.exact_points(p, np.zeros(3), T).any()
    assert mc.near_face(p, np.zeros(3), T, 1.0).tolist() == [True, False]


# ---- the oracle and the compiled reference -----------------------------------------------------------------------------------------------------
C1_SETTINGS = [(1.0, 2, 3), (0.5, 0, 1), (2.0, 1, 2)]
C1_SIZES = {(1.0, 2, 3): [1098, 1921, 1869, 2675, 3437, 1937, 2743, 3539], (0.5, 0, 1): [0] * 8, (2.0, 1, 2): [408, 408, 706, 425, 710, 427, 715, 424]}


def se3(axis, ang, t):
    """the pose of tests/test_gpu_parity.py, by the same route"""
    from scipy.spatial.transform import Rotation

    return pose(Rotation.from_rotvec(np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis) * ang).as_matrix(), t)


def c1_steps(d):
    return [(("tp", "tn", "tc") if k % 2 == 0 else ("sp", "sn", "sc"), se3([0.1, 0.2, 1.0], 0.02 * k, [6.0 * k, -2.0 * k, 0.1 * k])) for k in range(8)]


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return 0.0 if a.size == 0 else float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def pin_c1(d, make_cloud, make_gaussian, make_flat, leaf, horizon, cycle):
    clouds = {"tp": make_cloud(d["tp"].astype(np.float64), d["tn"].astype(np.float64), d["tc"].astype(np.float64)[:, :3, :3]),
              "sp": make_cloud(d["sp"].astype(np.float64), d["sn"].astype(np.float64), d["sc"].astype(np.float64)[:, :3, :3])}
    og, of = make_gaussian(leaf), make_flat(leaf)
    mg, mf = mc.Map(leaf, mc.GAUSSIAN), mc.Map(leaf, mc.FLAT, 0.01, 10)
    for m in (og, of, mg, mf):
        m.set_lru(horizon, cycle)
    of.set_setting(0.01, 10)
    worst, sizes = 0.0, []
    for (p, n, c), T in c1_steps(d):
        og.insert(clouds[p], T)
        of.insert(clouds[p], T)
        mg.insert(d[p].astype(np.float64), np.zeros(3), T, None, d[c].astype(np.float64)[:, :3, :3])
        mf.insert(d[p].astype(np.float64), np.zeros(3), T, None, d[c].astype(np.float64)[:, :3, :3])
        coords, means, covs, counts = og.get()
        assert len(og) == mg.size() and np.array_equal(coords, mg.coords()) and np.array_equal(counts.astype(np.int64), mg.counts())
        m, cv = mg.means()[:2]
        worst = max(worst, rel(m, means), rel(cv, covs))
        coords, counts, pts, covs = of.get()
        assert len(of) == mf.size() and np.array_equal(coords, mf.coords()) and np.array_equal(counts.astype(np.int64), mf.counts())
        if len(pts):
            got = mf.slots()
            worst = max(worst, rel(got["points"], pts), rel(got["covs"], covs))
        sizes.append(mg.size())
    assert sizes == C1_SIZES[(leaf, horizon, cycle)], sizes
    assert worst <= 1e-12, worst
    return worst


@pytest.mark.parametrize("leaf,horizon,cycle", C1_SETTINGS)
def test_restatement_equals_the_oracle_on_c1(orc, c1_f32, leaf, horizon, cycle):
    worst = pin_c1(c1_f32, orc.Cloud, lambda l: orc.VoxelMap(None, l), orc.FlatMap, leaf, horizon, cycle)
    print("leaf %g lru (%d, %d): worst relative difference %.2e" % (leaf, horizon, cycle, worst))


@pytest.mark.parametrize("leaf,horizon,cycle", C1_SETTINGS)
def test_restatement_equals_the_compiled_reference_on_c1(c1_f32, leaf, horizon, cycle):
    from oracle import ref

    if not ref.available():
        pytest.skip("the compiled reference is not here")
    worst = pin_c1(c1_f32, lambda p, n, c: ref.Cloud(p, n, c, tree=False), ref.VoxelMap, ref.FlatMap, leaf, horizon, cycle)
    print("leaf %g lru (%d, %d): worst relative difference %.2e" % (leaf, horizon, cycle, worst))

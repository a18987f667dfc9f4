"""tests/occupancy_ref.py — the numpy float64 restatement of sga_occupancy_*  — on cases decided by hand (a
beam inside one cell, a beam along an axis, the diagonal through lattice corners where every tmax ties and the lowest axis must win, an
endpoint that wins over the beams passing through it, clamping, ranges, a box out of reach, epochs) and on the exact cases of
tests/test_occupancy_gpu.py, whose figures are pinned HERE: the GPU test compares the device with these and with the restatement.

The exact cases: the scene outliers_ref.planes_with_scatter(seed), the scan fp32(T^-1 scene), three scans into one grid at POSES, ranges
0.5 / 12.0, OctoMap's log-odds, threshold 0.  The cap is ZERO band beams in every one of the 18 integrations (occupancy_ref: a component
of go or ge within 1e-9 of an integer, rho within 1e-9 of a range limit, a step that passes within 1e-9 of a cell edge); it is asserted
on the restatement.  (An origin of (-12, -12, -12) would put the first sensor on the lattice at leaf 0.5: all 3000 beams in the band.)
Cells after the scans 1 / 2 / 3 as (unknown, free, occupied): CASES below.

The meaning case: synthetic.kitti_like_scan(f, n_rings=16, n_az=251) through with_moving_sphere for f = 0 .. 5 at the generator's poses,
leaf 0.5, 80 x 64 x 12 cells, ranges 1.0 / 30.0: MEANING below.  No device and no library call."""
import functools

import numpy as np
import pytest

import occupancy_ref as ref
import outliers_ref

F32 = np.float32
RANGES = (0.5, 12.0)


def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """(test_cloud_merge_gpu.pose's formula: Rz Ry Rx and t)"""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


POSES = [pose(0.3, -0.2, 0.1, t=(1.5, -2.0, 0.5)), pose(-1.1, 0.15, -0.05, t=(-2.5, 3.0, 1.25)), pose(2.4, 0.1, 0.2, t=(0.5, 0.75, 2.0))]
ORIGIN_A = (-12.13, -11.87, -12.31)
# name: origin, leaf, dims, seed, n_plane, n_scatter, truncated per scan, (unknown, free, occupied) after each scan, (cells hit, cells freed) per scan
CASES = {
    "A": (ORIGIN_A, 0.5, (48, 48, 48), 1, 1450, 100, (32, 131, 27), ((106497, 3211, 884), (103801, 5892, 899), (102728, 6961, 903)), ((884, 3211), (851, 4291), (889, 3734))),
    "B": (ORIGIN_A, 0.25, (96, 96, 96), 1, 1450, 100, (32, 131, 27), ((869364, 13378, 1994), (855671, 27056, 2009), (851852, 30871, 2013)), ((1994, 13378), (1920, 21600), (1999, 17516))),
    "C": ((-4.13, -6.21, -1.07), 0.5, (16, 20, 8), 1, 1450, 100, (32, 131, 27), ((1648, 631, 281), (1073, 1206, 281), (919, 1360, 281)), ((281, 631), (281, 921), (281, 908))),  # beams leave the box
    "D": ((3.17, -6.21, -1.07), 0.4, (10, 30, 20), 1, 1450, 100, (32, 131, 27), ((3980, 1521, 499), (3672, 1829, 499), (3595, 1906, 499)), ((499, 1521), (497, 1633), (499, 1589))),  # every sensor outside the box
    "E": (ORIGIN_A, 0.5, (48, 48, 48), 3, 1450, 100, (28, 131, 30), ((106498, 3205, 889), (103672, 6014, 906), (102536, 7149, 907)), ((889, 3205), (856, 4368), (886, 3765))),
    "F": (ORIGIN_A, 0.5, (48, 48, 48), 5, 340, 50, (13, 33, 10), ((107732, 2362, 498), (105642, 4443, 507), (104968, 5115, 509)), ((498, 2362), (485, 3357), (501, 2819))),
}
NAMES = ("unknown", "free", "occupied")


@functools.lru_cache(maxsize=None)
def scene(seed, n_plane=1450, n_scatter=100):
    p = outliers_ref.planes_with_scatter(seed, n_plane, n_scatter)
    p.setflags(write=False)
    return p


def seen_from(points, T):
    """fp32(T^-1 points): the scene in the frame of a sensor at T"""
    Ti = np.linalg.inv(T)
    return np.ascontiguousarray((points.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32))


@functools.lru_cache(maxsize=None)
def scan_of(seed, k, n_plane=1450, n_scatter=100):
    p = seen_from(scene(seed, n_plane, n_scatter), POSES[k])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def exact_reference(name, mode=0):
    """the restatement's grid after each of the three scans of a case: a list of (scan statistics, stamp, L, cell counts)"""
    origin, leaf, dims, seed, n_plane, n_scatter = CASES[name][:6]
    grid = ref.Grid(origin, leaf, dims)
    out = []
    for k, T in enumerate(POSES):
        st = grid.integrate(scan_of(seed, k, n_plane, n_scatter), T, *RANGES, mode=mode)
        out.append((st, grid.stamp.copy(), grid.L.copy(), grid.stats(0.0)))
    return out, grid


# ---- the meaning case ---------------------------------------------------------------------------------------------------------------------
MEANING = dict(frames=6, n_rings=16, n_az=251, offset=(-10.13, -15.87, -2.31), leaf=0.5, dims=(80, 64, 12), min_range=1.0, max_range=30.0, radius=1.0,
               points=(3527, 3669, 3711, 3742, 3764, 3782), ghosts={0: 24, 1: 74}, cells={0: (45229, 13949, 2262), 1: (58399, 0, 3041)}, wall_cells=286)


@functools.lru_cache(maxsize=None)
def meaning_frames():
    """[(scan with the sphere (sensor frame), the returns the sphere changed, T_world_sensor)] and the grid's origin"""
    from small_gicp_amd import synthetic

    frames = []
    for f in range(MEANING["frames"]):
        pts, Tws = synthetic.kitti_like_scan(f, n_rings=MEANING["n_rings"], n_az=MEANING["n_az"])
        pts, changed = synthetic.with_moving_sphere(pts, Tws, synthetic.mover_centre(f), MEANING["radius"])
        frames.append((pts, changed, Tws))
    return frames, synthetic._sensor_pose(0)[:3, 3] + np.array(MEANING["offset"])


def ghost_cells(indices, centres, origin):
    """the occupied cells (their linear indices, given their centres' records) within one radius of an EARLIER centre of the mover and
    outside 1.1 radii of the last"""
    from small_gicp_amd import synthetic

    w = np.asarray(centres, dtype=np.float64) + origin
    r, last = MEANING["radius"], MEANING["frames"] - 1
    trail = np.zeros(len(w), bool)
    for f in range(last):
        trail |= np.linalg.norm(w - synthetic.mover_centre(f), axis=1) <= r
    return set(np.asarray(indices)[trail & (np.linalg.norm(w - synthetic.mover_centre(last), axis=1) > 1.1 * r)].tolist())


def static_wall_cells(grid):
    """the cells that hold a static return above the ground (unchanged by the sphere, world z > 0.5, within max_range) in at least HALF
    the scans: three hits and at most three misses leave L >= 3 * 0.85 - 3 * 0.4 > 0 in any order, so none of them may be free"""
    frames, origin = meaning_frames()
    seen = np.zeros(grid.cells, np.int64)
    for pts, changed, Tws in frames:
        w = pts.astype(np.float64) @ Tws[:3, :3].T + Tws[:3, 3]
        sel = ~changed & (w[:, 2] > 0.5) & (np.linalg.norm(pts.astype(np.float64), axis=1) <= MEANING["max_range"])
        c = np.floor((w[sel] - origin) / MEANING["leaf"]).astype(np.int64)
        seen[np.unique(grid._linear(c[grid._inside(c)]))] += 1
    return np.nonzero(2 * seen >= len(frames))[0]


@functools.lru_cache(maxsize=None)
def meaning_reference(mode):
    frames, origin = meaning_frames()
    grid = ref.Grid(origin, MEANING["leaf"], MEANING["dims"])
    stats = [grid.integrate(pts, Tws, MEANING["min_range"], MEANING["max_range"], mode) for pts, _, Tws in frames]
    return grid, stats


# ---- cases decided by hand ----------------------------------------------------------------------------------------------------------------
def cloud(*rows):
    return np.array(rows, dtype=F32).reshape(-1, 3)


def at(x, y, z):
    T = np.eye(4)
    T[:3, 3] = (x, y, z)
    return T


def test_a_beam_that_starts_and_ends_in_one_cell_of_a_one_cell_grid():
    g = ref.Grid((0, 0, 0), 1.0, (1, 1, 1))
    st = g.integrate(cloud([0.5, 0.0, 0.0]), at(0.25, 0.5, 0.5), 0.0, 10.0)
    assert (st["hits"], st["cells_hit"], st["cells_freed"], st["steps"], st["band"]) == (1, 1, 0, 0, 0)
    assert g.stamp.tolist() == [3] and g.L.tolist() == [F32(0.85)] and g.epoch == 1
    assert g.stats() == dict(total=1, unknown=0, free=0, occupied=1, epoch=1)
    # truncated inside the one cell: a free candidate, no hit
    g = ref.Grid((0, 0, 0), 1.0, (1, 1, 1))
    st = g.integrate(cloud([5.0, 0.0, 0.0]), at(0.25, 0.5, 0.5), 0.0, 0.5)
    assert (st["truncated"], st["cells_hit"], st["cells_freed"]) == (1, 0, 1) and g.stamp.tolist() == [2] and g.L.tolist() == [F32(-0.4)]


def test_a_beam_along_an_axis():
    g = ref.Grid((0, 0, 0), 0.5, (8, 1, 1))
    st = g.integrate(cloud([3.0, 0.0, 0.0]), at(0.25, 0.25, 0.25), 0.0, 10.0)
    assert (st["steps"], st["longest"], st["band"], st["ties"]) == (6, 6, 0, 0)
    assert g.stamp.tolist() == [2, 2, 2, 2, 2, 2, 3, 0] and g.L.tolist() == [F32(-0.4)] * 6 + [F32(0.85), 0.0]
    # backwards, and along z
    g = ref.Grid((0, 0, 0), 0.5, (1, 1, 8))
    st = g.integrate(cloud([0.0, 0.0, -3.0]), at(0.25, 0.25, 3.75), 0.0, 10.0)
    assert g.stamp.tolist() == [0, 3, 2, 2, 2, 2, 2, 2] and st["band"] == 0


def test_the_lowest_axis_wins_every_tie_on_the_diagonal_through_lattice_corners():
    g = ref.Grid((0, 0, 0), 0.5, (4, 4, 4))
    st = g.integrate(cloud([1.0, 1.0, 1.0]), at(0.25, 0.25, 0.25), 0.0, 10.0)
    assert (st["steps"], st["ties"], st["band"]) == (6, 1, 1)  # exact inputs: the tie is real, and it is a band beam by the rule
    lin = lambda x, y, z: (z * 4 + y) * 4 + x
    free = [lin(0, 0, 0), lin(1, 0, 0), lin(1, 1, 0), lin(1, 1, 1), lin(2, 1, 1), lin(2, 2, 1)]  # x, then y, then z, twice
    assert np.nonzero(g.stamp == 2)[0].tolist() == sorted(free) and np.nonzero(g.stamp == 3)[0].tolist() == [lin(2, 2, 2)]
    assert st["cells_freed"] == 6 and st["cells_hit"] == 1
    # the other way round the steps are negative and the order is the same: x, y, z
    g = ref.Grid((0, 0, 0), 0.5, (4, 4, 4))
    g.integrate(cloud([-1.0, -1.0, -1.0]), at(1.25, 1.25, 1.25), 0.0, 10.0)
    free = [lin(2, 2, 2), lin(1, 2, 2), lin(1, 1, 2), lin(1, 1, 1), lin(0, 1, 1), lin(0, 0, 1)]
    assert np.nonzero(g.stamp == 2)[0].tolist() == sorted(free) and np.nonzero(g.stamp == 3)[0].tolist() == [lin(0, 0, 0)]


def test_an_endpoint_wins_over_the_beams_that_pass_through_it_and_a_cell_is_updated_once():
    g = ref.Grid((0, 0, 0), 0.5, (8, 1, 1))
    st = g.integrate(cloud([1.5, 0.0, 0.0], [3.0, 0.0, 0.0], [3.1, 0.0, 0.0], [1.6, 0.0, 0.0]), at(0.25, 0.25, 0.25), 0.0, 10.0)
    assert g.stamp.tolist() == [2, 2, 2, 3, 2, 2, 3, 0]  # cell 3 is an endpoint although two beams pass through it
    assert g.L.tolist() == [F32(-0.4)] * 3 + [F32(0.85)] + [F32(-0.4)] * 2 + [F32(0.85), 0.0]  # once per scan, whatever the number of beams
    assert (st["hits"], st["cells_hit"], st["cells_freed"]) == (4, 2, 5)
    # the next scan sees through cell 3: freed, stamp 2 e
    st = g.integrate(cloud([3.0, 0.0, 0.0]), at(0.25, 0.25, 0.25), 0.0, 10.0)
    assert g.stamp.tolist() == [4, 4, 4, 4, 4, 4, 5, 0] and g.L[3] == F32(F32(0.85) + F32(-0.4)) and g.L[6] == F32(F32(0.85) + F32(0.85)) and g.epoch == 2


def test_the_same_scan_eight_times_reaches_the_clamps_exactly():
    g = ref.Grid((0, 0, 0), 0.5, (8, 1, 1))
    for _ in range(8):
        g.integrate(cloud([3.0, 0.0, 0.0]), at(0.25, 0.25, 0.25), 0.0, 10.0)
    assert g.L.tolist() == [F32(-2.0)] * 6 + [F32(3.5), 0.0] and g.stamp.tolist() == [16] * 6 + [17, 0]
    assert g.stats(0.0) == dict(total=8, unknown=1, free=6, occupied=1, epoch=8) and g.stats(-5.0)["occupied"] == 7 and g.stats(5.0)["free"] == 7


def test_ranges_modes_and_a_box_out_of_reach():
    sensor = at(0.25, 0.25, 0.25)
    g = ref.Grid((0, 0, 0), 0.5, (8, 1, 1))
    st = g.integrate(cloud([2.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]), sensor, 3.0, 10.0)  # nearer than min_range, not finite
    assert (st["beams"], st["ignored"], st["hits"]) == (3, 3, 0) and not g.stamp.any() and g.epoch == 1
    st = g.integrate(cloud([5.0, 0.0, 0.0]), sensor, 0.0, 2.0)  # truncated at 2 m inside the box: cells 0 .. 4 free, no hit
    assert (st["truncated"], st["cells_hit"], st["cells_freed"]) == (1, 0, 5) and g.stamp.tolist() == [4] * 5 + [0] * 3
    g = ref.Grid((0, 0, 0), 0.5, (3, 1, 1))
    st = g.integrate(cloud([5.0, 0.0, 0.0], [3.0, 0.0, 0.0]), sensor, 0.0, 2.0)  # ... and outside it; a hit outside the box touches nothing
    assert (st["truncated"], st["hits"], st["cells_hit"], st["cells_freed"]) == (2, 0, 0, 3)
    st = g.integrate(cloud([1.0, 0.0, 0.0], [3.0, 0.0, 0.0]), sensor, 0.0, 10.0, mode=1)  # endpoints only
    assert (st["hits"], st["cells_hit"], st["cells_freed"]) == (2, 1, 0) and g.stamp.tolist() == [2, 2, 5] and g.epoch == 2
    before = (g.stamp.copy(), g.L.copy())
    st = g.integrate(cloud([1.0, 0.0, 0.0]), at(100.0, 0.25, 0.25), 0.0, 10.0)  # the box is farther than max_range from the sensor
    assert g.epoch == 3 and st["beams"] == 1 and st["hits"] == 0 and np.array_equal(g.stamp, before[0]) and np.array_equal(g.L, before[1])
    assert not g.reachable(at(100.0, 0.25, 0.25), 10.0) and g.reachable(at(11.0, 0.25, 0.25), 10.0)
    st = g.integrate(np.zeros((0, 3), F32), sensor, 0.0, 10.0)  # an empty scan advances the epoch
    assert g.epoch == 4 and st["beams"] == 0
    g.clear()
    assert g.epoch == 0 and not g.stamp.any() and not g.L.any()


def test_classify_and_export():
    g = ref.Grid((0, 0, 0), 0.5, (8, 1, 1))
    g.integrate(cloud([3.0, 0.0, 0.0]), at(0.25, 0.25, 0.25), 0.0, 10.0)
    c = g.classify(cloud([0.1, 0.1, 0.1], [3.3, 0.1, 0.1], [3.6, 0.1, 0.1], [-0.1, 0.1, 0.1], [0.1, 0.6, 0.1], [np.nan, 0.1, 0.1], [4.0, 0.1, 0.1]))
    assert c["state"].tolist() == [1, 2, 0, 0, 0, 0, 0] and c["counts"] == dict(total=7, unknown=5, free=1, occupied=1, epoch=1)
    assert c["band"].tolist() == [6]  # 4.0 / 0.5 is a face
    assert g.classify(cloud([3.3, 0.1, 0.1]), threshold=1.0)["state"].tolist() == [1] and g.classify(cloud([0.1, 0.1, 0.1]), threshold=-0.5)["state"].tolist() == [2]
    # a pose and an origin: the same point of the world
    T = pose(0.0, 0.0, 0.0, t=(1.0, 0.0, 0.0))
    assert g.classify(cloud([1.3, 0.1, 0.1]), T, o_c=(1.0, 0.0, 0.0))["state"].tolist() == [2]
    idx, L, centres = g.export(0.0, 4)
    assert idx.tolist() == [6] and L.tolist() == [F32(0.85)] and centres.tolist() == [[3.25, 0.25, 0.25]]
    idx, L, centres = g.export(0.0, 3)
    assert idx.tolist() == [0, 1, 2, 3, 4, 5, 7] and centres[:, 0].tolist() == [0.25, 0.75, 1.25, 1.75, 2.25, 2.75, 3.75]


# ---- the pinned figures -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_the_exact_cases_have_no_band_beam_and_the_pinned_figures(name):
    _, _, dims, seed, n_plane, n_scatter, truncated, cells, touched = CASES[name]
    out, grid = exact_reference(name)
    for k, (st, stamp, L, counts) in enumerate(out):
        assert st["band"] == 0 and st["ties"] == 0, (name, k)  # the cap: ZERO band beams
        assert st["beams"] == 2 * n_plane + n_scatter and st["truncated"] == truncated[k] and st["ignored"] + st["hits"] + st["truncated"] == st["beams"]
        assert tuple(counts[w] for w in NAMES) == cells[k], (name, k)
        assert (st["cells_hit"], st["cells_freed"]) == touched[k], (name, k)
        assert counts["total"] == int(np.prod(dims)) and counts["epoch"] == k + 1
        assert int((stamp == 2 * (k + 1) + 1).sum()) == st["cells_hit"] and int((stamp == 2 * (k + 1)).sum()) == st["cells_freed"]
    # endpoints only: the same hits, nothing freed
    out1, _ = exact_reference(name, 1)
    for k in range(3):
        assert out1[k][0]["cells_hit"] == touched[k][0] and out1[k][0]["cells_freed"] == 0 and out1[k][3]["free"] == 0
    # the points of the scene and of the last scan against the grid: nothing within 1e-9 of a face
    assert len(grid.classify(scene(seed, n_plane, n_scatter))["band"]) == 0 and len(grid.classify(scan_of(seed, 2, n_plane, n_scatter), POSES[2])["band"]) == 0


def test_the_meaning_case_has_the_pinned_figures():
    frames, origin = meaning_frames()
    assert tuple(len(p) for p, _, _ in frames) == MEANING["points"]
    ghosts = {}
    for mode in (0, 1):
        grid, stats = meaning_reference(mode)
        assert all(st["band"] == 0 for st in stats)
        counts = grid.stats(0.0)
        assert tuple(counts[w] for w in NAMES) == MEANING["cells"][mode]
        idx, _, centres = grid.export(0.0, 4)
        ghosts[mode] = ghost_cells(idx, centres, origin)
        assert len(ghosts[mode]) == MEANING["ghosts"][mode]
    assert ghosts[0] <= ghosts[1]  # free space only ever takes occupied cells away
    grid, _ = meaning_reference(0)
    wall = static_wall_cells(grid)
    assert len(wall) == MEANING["wall_cells"] and not (grid.cell_states(0.0)[wall] == ref.FREE).any()

"""The occupancy grid on the device (csrc/occupancy.hip: sga_occupancy_*) against the fp64 restatement of
tests/occupancy_ref.py, which never goes through the library, and against the figures pinned in tests/test_occupancy_ref.py.

The comparison rule is derived, not tuned.  After go and ge every operation of the walk is a single IEEE operation in the stated order,
so the device and the restatement can differ only through the pose product and rho (contraction under -ffp-contract=fast) and through
floor at a face.  A beam is IN THE BAND when a component of go or ge lies within 1e-9 of an integer, when rho lies within 1e-9 of a range
limit, or when at some step another eligible axis has (tmax_b - tmax_a) * |d_b| < 1e-9.  The cap is ZERO band beams in every exact case,
asserted on the restatement before anything is compared (if it ever fails: another seed or origin, never a looser rule).  Then everything
is EQUAL: the stamps and the log-odds of every cell bit for bit after each scan, the scan statistics, classify's states, counts and kept,
the output cloud's records and attributes equal to input [kept] bit for bit, export's order, indices, log-odds and centres, and two runs
from clear give identical bytes.

The exact cases (tests/test_occupancy_ref.py: CASES) — scene outliers_ref.planes_with_scatter(seed), scan fp32(T^-1 scene), three scans
into one grid, ranges 0.5 / 12.0, threshold 0 — with the cells after the scans 1 / 2 / 3 as unknown / free / occupied:
    A  origin (-12.13, -11.87, -12.31), leaf 0.5, 48^3, seed 1 (3000 beams)   106497/3211/884   103801/5892/899   102728/6961/903
    B  as A, leaf 0.25, 96^3                                                    869364/13378/1994 855671/27056/2009 851852/30871/2013
    C  origin (-4.13, -6.21, -1.07), leaf 0.5, 16 x 20 x 8: beams leave the box 1648/631/281      1073/1206/281     919/1360/281
    D  origin (3.17, -6.21, -1.07), leaf 0.4, 10 x 30 x 20: sensors outside     3980/1521/499     3672/1829/499     3595/1906/499
    E  as A, seed 3                                                             106498/3205/889   103672/6014/906   102536/7149/907
    F  as A, seed 5, 340 + 340 + 50 = 730 beams                                 107732/2362/498   105642/4443/507   104968/5115/509
With quarter-turn poses and integer / half-integer coordinates at leaf 0.5 the arithmetic is exact on both sides: ties really occur (the
sensor sits on a lattice corner, beams run through edges and corners), every beam is a band beam by the rule, and equality must hold all
the same — lowest axis first.

Meaning (tests/test_occupancy_ref.py: MEANING): kitti_like_scan(0 .. 5, n_rings=16, n_az=251) through with_moving_sphere at the
generator's poses, leaf 0.5, 80 x 64 x 12, ranges 1.0 / 30.0: 74 occupied cells on the mover's trail with the endpoints alone, 24 with
free space, the 24 a subset of the 74, and none of the 286 static wall cells (a static return above the ground in at least half the
scans) is free."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import occupancy_ref as ref
import small_gicp_amd as sga
import test_occupancy_ref as cases
from conftest import ROOT
from test_cloud_merge_gpu import FAR, QUARTER, attributes, pose, records, upload_relative
from test_cloud_outliers_gpu import attributes_for

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = np.zeros(3)
NAMES = cases.NAMES
SCAN_NAMES = ("beams", "ignored", "hits", "truncated", "cells_hit", "cells_freed")
MASKS = [None, "occupied", ("unknown", "occupied"), "free", 7]


def at(x, y, z):
    return pose(t=(x, y, z))


def cloud(*rows):
    return np.array(rows, dtype=F32).reshape(-1, 3)


# ---- the calls and the comparisons ----------------------------------------------------------------------------------------------------------
def same_cells(dev, want, what=""):
    """the device grid's raw arrays against the restatement's, bit for bit"""
    stamp, L = dev.download()
    assert stamp.dtype == np.uint32 and L.dtype == F32 and stamp.shape == (dev.dims[2], dev.dims[1], dev.dims[0])
    ds, dl = stamp.reshape(-1), L.reshape(-1)
    bad = np.nonzero((ds != want.stamp) | (dl.view(np.uint32) != want.L.view(np.uint32)))[0]
    assert len(bad) == 0, (what, "%d cells differ, the first at %d: device (%d, %r), restatement (%d, %r)" % (len(bad), bad[0], ds[bad[0]], dl[bad[0]], want.stamp[bad[0]], want.L[bad[0]]) if len(bad) else "")
    assert dev.epoch == want.epoch, what
    return ds, dl


def integrate_both(dev, want, scan_rel, T, min_range, max_range, mode=0, o_c=ZERO, what="", max_band=0, ctx=None, scan=None):
    """one scan into the device grid and into the restatement; the statistics and every cell must be equal -> the restatement's statistics"""
    st_ref = want.integrate(scan_rel, T, min_range, max_range, mode, o_c=o_c)
    if max_band is not None:
        assert st_ref["band"] <= max_band, (what, "the restatement has %d beams in the band" % st_ref["band"])
    scan = scan if scan is not None else upload_relative(scan_rel, None, None, o_c)
    st = dev.integrate(scan, T, min_range, max_range, mode, return_stats=True, ctx=ctx)
    print("%s: device %s, restatement %s, band %d, ties %d, cells walked %d (longest beam %d)" % (what, [st[w] for w in SCAN_NAMES], [st_ref[w] for w in SCAN_NAMES], st_ref["band"], st_ref["ties"], st_ref["steps"], st_ref["longest"]))
    assert [st[w] for w in SCAN_NAMES] == [st_ref[w] for w in SCAN_NAMES], what
    same_cells(dev, want, what)
    return st_ref


def check_classify(dev, want, rel, T, threshold=0.0, o_c=ZERO, nrm=None, cov6=None, masks=MASKS, what=""):
    """classify over every mask: states, counts, kept, records and attributes equal input [kept] bit for bit"""
    w = want.classify(rel, T, threshold, o_c=o_c)
    assert len(w["band"]) == 0, (what, "the restatement has %d points within 1e-9 of a face" % len(w["band"]))
    cl = upload_relative(rel, nrm, cov6, o_c)
    finite = np.isfinite(np.asarray(rel, dtype=np.float64)).all(axis=1)
    for keep in masks:
        res = dev.classify(cl, T, threshold, keep=keep, return_state=True, return_kept=keep is not None)
        counts, state = res[0], res[2 if keep is not None else 1]
        assert state.dtype == np.uint8 and np.array_equal(state, w["state"]), (what, keep)
        assert counts == w["counts"], (what, keep)
        if keep is None:
            assert len(res) == 2
            continue
        out, kept = res[1], res[3]
        mask = sga.api._state_mask(keep, "keep")
        want_kept = np.nonzero((mask >> w["state"].astype(np.int64)) & 1)[0]
        assert kept.dtype == np.int64 and np.array_equal(kept, want_kept), (what, keep)
        assert out.size() == len(kept) and np.array_equal(out.origin(), np.asarray(o_c, dtype=np.float64))
        if len(kept) == 0:
            assert out._has() == (False, False)  # an empty cloud without attributes
            continue
        assert out._has() == (nrm is not None, cov6 is not None)
        if finite[kept].all():  # (records() reads through a kd-tree when the origin is not zero: finite records only)
            rec, _ = records(out)
            assert rec.tobytes() == np.ascontiguousarray(rel[kept]).tobytes(), (what, keep)  # bit for bit
        nr, c6 = attributes(out)
        if nrm is not None:
            assert nr.tobytes() == np.ascontiguousarray(nrm[kept]).tobytes(), (what, keep)
        if cov6 is not None:
            assert c6.tobytes() == np.ascontiguousarray(cov6[kept]).tobytes(), (what, keep)
    return w


def check_export(dev, want, threshold=0.0, whiches=("occupied", "free", ("free", "occupied"), 7), what=""):
    for which in whiches:
        idx, L, centres = want.export(threshold, sga.api._state_mask(which, "which"))
        res = dev.export(threshold, which)
        assert res["count"] == len(idx) and res["indices"].dtype == np.int64 and np.array_equal(res["indices"], idx), (what, which)
        assert res["log_odds"].dtype == F32 and res["log_odds"].tobytes() == L.tobytes(), (what, which)
        out = res["cloud"]
        assert out.size() == len(idx) and np.array_equal(out.origin(), want.g) and out._has() == (False, False)
        if len(idx):
            rec = records(out)[0] if not want.g.any() else cell_records(out)
            assert rec.tobytes() == centres.tobytes(), (what, which)
    # a capacity below the count: the count is the whole, the first entries are written
    idx, L, centres = want.export(threshold, 4)
    if len(idx) > 3:
        res = dev.export(threshold, "occupied", capacity=3)
        assert res["count"] == len(idx) and np.array_equal(res["indices"], idx[:3]) and res["log_odds"].tobytes() == L[:3].tobytes() and res["cloud"].size() == 3
        assert cell_records(res["cloud"]).tobytes() == centres[:3].tobytes()
        res = dev.export(threshold, "occupied", capacity=0, return_cloud=False)
        assert res["count"] == len(idx) and len(res["indices"]) == 0 and "cloud" not in res
    assert dev.occupied_cloud(threshold).size() == len(idx)
    st = dev.stats(threshold)
    assert st == want.stats(threshold), what


def cell_records(out):
    """the device-frame records of a cloud of cell centres, exactly: the download in double is record + origin, and the records are
    half-multiples of the leaf: subtracting the origin again is exact to well below fp32's spacing, so rounding gives the record back"""
    return (out.xyz64() - out.origin()).astype(F32)


def new_grids(origin, leaf, dims, **kw):
    return sga.OccupancyGrid(origin, leaf, dims, **kw), ref.Grid(origin, leaf, dims, **kw)


# ---- 1. the exact cases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_exact_cases_equal_the_restatement_and_the_pinned_figures(name):
    origin, leaf, dims, seed, n_plane, n_scatter, truncated, cells, touched = cases.CASES[name]
    pinned, _ = cases.exact_reference(name)
    dev, want = new_grids(origin, leaf, dims)
    first = []
    for k, T in enumerate(cases.POSES):
        st = integrate_both(dev, want, cases.scan_of(seed, k, n_plane, n_scatter), T, *cases.RANGES, what="%s scan %d" % (name, k + 1))
        assert st["truncated"] == truncated[k] and (st["cells_hit"], st["cells_freed"]) == touched[k]
        counts = dev.stats(0.0)
        assert tuple(counts[w] for w in NAMES) == cells[k] and counts["total"] == int(np.prod(dims)) and counts["epoch"] == k + 1  # the pinned figures
        assert np.array_equal(want.stamp, pinned[k][1]) and want.L.tobytes() == pinned[k][2].tobytes()
        first.append(dev.download())
    # the queries: the scene in the world (with normals and covariances in case A), the last scan at its pose
    rel = cases.scene(seed, n_plane, n_scatter)
    nrm, cov6 = attributes_for(len(rel)) if name == "A" else (None, None)
    w = check_classify(dev, want, rel, None, nrm=nrm, cov6=cov6, what=name + " scene")
    if name == "A":
        assert min(w["counts"][s] for s in NAMES) > 0  # every state occurs
    check_classify(dev, want, cases.scan_of(seed, 2, n_plane, n_scatter), cases.POSES[2], masks=[None, ("unknown", "occupied")], what=name + " scan 3")
    check_export(dev, want, what=name)
    # two runs from clear give identical bytes
    dev.clear()
    assert dev.epoch == 0 and dev.stats()["unknown"] == dev.cells
    for k, T in enumerate(cases.POSES):
        dev.integrate(upload_relative(cases.scan_of(seed, k, n_plane, n_scatter), None, None, ZERO), T, *cases.RANGES)
        again = dev.download()
        assert again[0].tobytes() == first[k][0].tobytes() and again[1].tobytes() == first[k][1].tobytes(), (name, k)


@pytest.mark.parametrize("name", ["A", "C"])
def test_endpoints_only_equal_the_restatement(name):
    origin, leaf, dims, seed, n_plane, n_scatter = cases.CASES[name][:6]
    dev, want = new_grids(origin, leaf, dims)
    for k, T in enumerate(cases.POSES):
        st = integrate_both(dev, want, cases.scan_of(seed, k, n_plane, n_scatter), T, *cases.RANGES, mode=1, what="%s mode 1 scan %d" % (name, k + 1))
        assert st["cells_freed"] == 0
    assert dev.stats()["free"] == 0
    # ... and mixed with full scans in one grid
    integrate_both(dev, want, cases.scan_of(seed, 0, n_plane, n_scatter), cases.POSES[0], *cases.RANGES, mode=0, what=name + " mode 0 after mode 1")
    check_export(dev, want, what=name + " mixed modes")


# ---- 2. sizes at which the kernels can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_scans(n):
    origin, leaf, dims = cases.CASES["F"][:3]
    dev, want = new_grids(origin, leaf, dims)
    for k, T in enumerate(cases.POSES):
        integrate_both(dev, want, cases.scan_of(5, k, 340, 50)[:n], T, *cases.RANGES, what="a scan of %d, pose %d" % (n, k))
    check_export(dev, want, what="scans of %d" % n)


def test_a_scan_of_9001_beams():
    origin, leaf, dims = cases.CASES["A"][:3]
    scan_rel = np.ascontiguousarray(np.concatenate([cases.scan_of(s, 0) for s in (1, 3, 7)] + [cases.scan_of(9, 0)[:1]]))
    assert len(scan_rel) == 9001
    dev, want = new_grids(origin, leaf, dims)
    integrate_both(dev, want, scan_rel, cases.POSES[0], *cases.RANGES, what="9001 beams")
    integrate_both(dev, want, scan_rel, cases.POSES[0], *cases.RANGES, mode=1, what="9001 beams, endpoints only")
    check_classify(dev, want, scan_rel, cases.POSES[0], masks=[None, 5, 2], what="9001 points")
    check_export(dev, want, what="9001 beams")


def test_an_empty_scan_and_a_box_out_of_reach_advance_the_epoch_and_enqueue_nothing():
    dev, want = new_grids((0, 0, 0), 0.5, (8, 1, 1))
    sensor = at(0.25, 0.25, 0.25)
    integrate_both(dev, want, cloud([3.0, 0.0, 0.0]), sensor, 0.0, 10.0, what="one beam")
    before = (sga.occupancy_launches(), sga.occupancy_waits())
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    assert dev.integrate(empty, sensor, 0.0, 10.0, return_stats=True) == dict(beams=0, ignored=0, hits=0, truncated=0, cells_hit=0, cells_freed=0)
    assert dev.integrate(empty, sensor, 0.0, 10.0) is None and dev.epoch == 3
    far = upload_relative(cloud([1.0, 0.0, 0.0]), None, None, ZERO)
    assert dev.integrate(far, at(100.0, 0.25, 0.25), 0.0, 10.0, return_stats=True) == dict(beams=1, ignored=0, hits=0, truncated=0, cells_hit=0, cells_freed=0)
    assert (sga.occupancy_launches(), sga.occupancy_waits()) == before and dev.epoch == 4
    for _ in range(2):
        want.integrate(np.zeros((0, 3), F32), sensor, 0.0, 10.0)
    want.integrate(cloud([1.0, 0.0, 0.0]), at(100.0, 0.25, 0.25), 0.0, 10.0)
    same_cells(dev, want, "after the scans that touch nothing")
    integrate_both(dev, want, cloud([1.0, 0.0, 0.0]), at(11.1, 0.25, 0.25), 0.0, 10.0, what="within reach of the box, the beam outside")
    # an empty cloud classifies to nothing, and nothing is enqueued
    before = (sga.occupancy_launches(), sga.occupancy_waits())
    counts, out, state, kept = dev.classify(empty, None, keep="occupied", return_state=True, return_kept=True)
    assert counts == dict(total=0, unknown=0, free=0, occupied=0, epoch=5) and out.size() == 0 and len(state) == 0 and len(kept) == 0
    assert (sga.occupancy_launches(), sga.occupancy_waits()) == before


def test_one_cell_one_beam_and_the_axes():
    dev, want = new_grids((0, 0, 0), 1.0, (1, 1, 1))
    integrate_both(dev, want, cloud([0.5, 0.0, 0.0]), at(0.25, 0.5, 0.5), 0.0, 10.0, what="a beam inside the one cell")
    assert want.stamp.tolist() == [3]
    integrate_both(dev, want, cloud([5.0, 0.0, 0.0]), at(0.25, 0.5, 0.5), 0.0, 0.5, what="truncated inside the one cell")
    integrate_both(dev, want, cloud([5.0, 1.1, -2.3], [-3.0, 0.4, 0.2]), at(0.25, 0.5, 0.5), 0.0, 10.0, what="beams that leave the one cell")
    check_export(dev, want, whiches=("occupied", 7), what="1 x 1 x 1")
    check_classify(dev, want, cloud([0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [np.nan, 0.0, 0.0]), None, masks=[None, 1, 4, 7], what="1 x 1 x 1")
    for axis in range(3):
        for sign in (1.0, -1.0):
            dims = [1, 1, 1]
            dims[axis] = 8
            dev, want = new_grids((0, 0, 0), 0.5, dims)
            start = [0.25, 0.25, 0.25]
            start[axis] = 0.25 if sign > 0 else 3.75
            beam = np.zeros((2, 3), F32)
            beam[0, axis], beam[1, axis] = 3.0 * sign, 1.5 * sign
            st = integrate_both(dev, want, beam, at(*start), 0.0, 10.0, what="axis %d, sign %+d" % (axis, sign))
            assert (st["cells_hit"], st["cells_freed"], st["longest"]) == (2, 5, 6)


@pytest.mark.parametrize("k", range(len(QUARTER)))
def test_quarter_turn_poses_with_half_integer_coordinates_tie_and_go_lowest_axis_first(k):
    """exact arithmetic on both sides: the sensor on a lattice corner, returns on half-integer coordinates at leaf 0.5 — beams through
    edges and corners.  Every beam is a band beam by the rule; equality must hold all the same."""
    T = QUARTER[k]
    rng = np.random.default_rng(31 + k)
    p = np.unique(rng.integers(-16, 17, (600, 3)), axis=0).astype(np.float64) * 0.5
    diag = np.array([[s * a, s * a, s * a] for a in (1.0, 2.5, 4.0) for s in (1.0, -1.0)] + [[3.0, 3.0, 0.0], [0.0, -2.0, -2.0], [1.5, 0.0, 1.5], [2.0, 1.0, 0.5]])
    p = np.concatenate([diag, p[np.abs(p).sum(axis=1) > 0]])
    rho = np.linalg.norm(p, axis=1)
    assert np.abs(rho - 0.3).min() > 1e-6 and np.abs(rho - 7.3).min() > 1e-6  # no range sits on a limit
    dev, want = new_grids((-12.0, -12.0, -12.0), 0.5, (48, 48, 48))
    st = integrate_both(dev, want, p.astype(F32), T, 0.3, 7.3, what="quarter turn %d" % k, max_band=None)
    assert st["ties"] > 100 and st["truncated"] > 50 and st["hits"] > 100 and st["band"] == st["hits"] + st["truncated"]
    st = integrate_both(dev, want, p.astype(F32)[::-1].copy(), QUARTER[(k + 1) % len(QUARTER)], 0.3, 7.3, what="quarter turn %d, the next pose" % k, max_band=None)
    check_export(dev, want, what="quarter turn %d" % k)


def test_the_diagonal_through_lattice_corners():
    dev, want = new_grids((0, 0, 0), 0.5, (4, 4, 4))
    st = integrate_both(dev, want, cloud([1.0, 1.0, 1.0]), at(0.25, 0.25, 0.25), 0.0, 10.0, what="the diagonal", max_band=None)
    lin = lambda x, y, z: (z * 4 + y) * 4 + x
    assert st["ties"] == 1 and np.nonzero(want.stamp == 2)[0].tolist() == sorted([lin(0, 0, 0), lin(1, 0, 0), lin(1, 1, 0), lin(1, 1, 1), lin(2, 1, 1), lin(2, 2, 1)])
    dev, want = new_grids((0, 0, 0), 0.5, (4, 4, 4))
    integrate_both(dev, want, cloud([-1.0, -1.0, -1.0]), at(1.25, 1.25, 1.25), 0.0, 10.0, what="the diagonal, backwards", max_band=None)
    assert np.nonzero(want.stamp == 3)[0].tolist() == [0]


# ---- 3. ranges, clamping ----------------------------------------------------------------------------------------------------------------------
def test_min_range_ignores_returns_and_truncated_beams_end_inside_and_outside_the_box():
    origin, leaf, dims = cases.CASES["C"][:3]
    dev, want = new_grids(origin, leaf, dims)
    st = integrate_both(dev, want, cases.scan_of(1, 0), cases.POSES[0], 3.0, 12.0, what="min_range 3")
    assert st["ignored"] > 100
    st = integrate_both(dev, want, cases.scan_of(1, 1), cases.POSES[1], 0.5, 4.0, what="max_range 4")  # most beams are cut: inside the box and outside it
    assert st["truncated"] > 1000 and st["hits"] > 100
    scan_rel = cases.scan_of(1, 2).copy()
    scan_rel[5] = [np.nan, 0.0, 1.0]
    scan_rel[77] = [np.inf, -np.inf, 0.0]
    scan_rel[640, 2] = -np.inf
    st = integrate_both(dev, want, scan_rel, cases.POSES[2], 0.5, 12.0, what="non-finite returns")
    assert st["ignored"] >= 3
    check_export(dev, want, what="ranges")


def test_the_same_scan_eight_times_reaches_the_clamps_exactly():
    origin, leaf, dims = cases.CASES["F"][:3]
    dev, want = new_grids(origin, leaf, dims)
    for k in range(8):
        integrate_both(dev, want, cases.scan_of(5, 0, 340, 50), cases.POSES[0], *cases.RANGES, what="repeat %d" % k)
    _, L = dev.download()
    assert L.max() == F32(3.5) and L.min() == F32(-2.0) and int((L == F32(3.5)).sum()) == 498 and int((L == F32(-2.0)).sum()) == 2362  # (case F's first scan)
    # other log-odds parameters
    dev, want = new_grids(origin, leaf, dims, l_hit=0.7, l_miss=-0.3, l_min=-0.5, l_max=1.0)
    for k in range(3):
        integrate_both(dev, want, cases.scan_of(5, k, 340, 50), cases.POSES[k], *cases.RANGES, what="other log-odds, scan %d" % k)
    check_export(dev, want, threshold=0.5, what="other log-odds")
    check_classify(dev, want, cases.scene(5, 340, 50), None, threshold=0.5, masks=[None, 5], what="threshold 0.5")


# ---- 4. frames ------------------------------------------------------------------------------------------------------------------------------
def test_a_scan_on_an_origin_4000_km_out_with_the_grid_beside_it():
    """the pose and the grid's origin carry FAR; the scan's records are relative to an origin of its own that the kernel adds back in
    double (the sensor frame is where the scan's records plus its origin are: at (3000, -7000, 500) the records sit on fp32's grid of a
    quarter to half a millimetre, and the restatement sees the same records)"""
    origin, leaf, dims = cases.CASES["A"][:3]
    o_s = np.array([3000.0, -7000.0, 500.0])
    dev, want = new_grids(np.asarray(origin) + FAR, leaf, dims)
    for k, T0 in enumerate(cases.POSES):
        T = T0.copy()
        T[:3, 3] += FAR
        scan_rel = (cases.scan_of(1, k).astype(np.float64) - o_s).astype(F32)
        integrate_both(dev, want, scan_rel, T, *cases.RANGES, o_c=o_s, what="far frames, scan %d" % k)
    plain, _ = cases.exact_reference("A")
    counts = dev.stats()
    assert all(abs(counts[w] - plain[2][3][w]) < 0.02 * plain[2][3]["occupied"] for w in NAMES)  # the same geometry
    # the scene relative to FAR classifies against the grid, and the export's centres carry the grid's origin
    check_classify(dev, want, cases.scene(1), pose(t=FAR), masks=[None, 5], what="far frames")
    rel = cases.scene(1)
    check_classify(dev, want, rel, None, o_c=FAR, masks=[None, 5], what="a cloud on the far origin")
    check_export(dev, want, whiches=("occupied",), what="far frames")


# ---- 5. refusals that need live handles, ordering across contexts ---------------------------------------------------------------------------
def test_refusals_with_live_handles():
    dev, _ = new_grids((0, 0, 0), 0.5, (8, 1, 1))
    scan = upload_relative(cloud([3.0, 0.0, 0.0]), None, None, ZERO)
    before = (sga.occupancy_launches(), sga.occupancy_waits())
    with pytest.raises(sga.SgaError, match="more than 4096 cells"):
        dev.integrate(scan, None, 0.0, 2048.5)
    assert dev.epoch == 0 and (sga.occupancy_launches(), sga.occupancy_waits()) == before
    dev.integrate(scan, None, 0.0, 2048.0)  # 4096 cells exactly
    assert dev.epoch == 1


def test_a_cloud_or_grid_on_another_device_is_refused():
    if sga.load().sga_device_count() < 2:
        pytest.skip("ONE DEVICE ONLY: the refusal of a cloud or a grid that lives on another device was NOT exercised")
    other = sga.Context(1)
    here, there = upload_relative(cloud([3.0, 0.0, 0.0]), None, None, ZERO), upload_relative(cloud([3.0, 0.0, 0.0]), None, None, ZERO, other)
    dev = sga.OccupancyGrid((0, 0, 0), 0.5, (8, 1, 1))
    before = sga.occupancy_launches()
    with pytest.raises(sga.SgaError, match="scan lives on another device"):
        dev.integrate(there)
    with pytest.raises(sga.SgaError, match="cloud lives on another device"):
        dev.classify(there)
    for call in (lambda: dev.integrate(there, ctx=other), lambda: dev.classify(there, ctx=other), lambda: dev.stats(ctx=other), lambda: dev.export(ctx=other), lambda: dev.download(ctx=other), lambda: dev.clear(ctx=other)):
        with pytest.raises(sga.SgaError, match="the grid lives on another device"):
            call()
    assert sga.occupancy_launches() == before and dev.epoch == 0
    dev.integrate(here)


def test_clouds_and_grids_across_stream_ordered_contexts():
    origin, leaf, dims = cases.CASES["A"][:3]
    plain, _ = cases.exact_reference("A")
    want = ref.Grid(origin, leaf, dims)
    ctx, other = sga.Context(0), sga.Context(0)
    ctx.set_stream_ordered(True)
    other.set_stream_ordered(True)
    try:
        dev = sga.OccupancyGrid(origin, leaf, dims, ctx=other)  # its fills are in flight on the other context's stream
        for k, T in enumerate(cases.POSES):
            scan = upload_relative(cases.scan_of(1, k), None, None, ZERO, other)  # returns with its kernels in flight
            integrate_both(dev, want, cases.scan_of(1, k), T, *cases.RANGES, what="another context, scan %d" % k, ctx=ctx if k != 1 else other, scan=scan)
        assert np.array_equal(want.stamp, plain[2][1]) and want.L.tobytes() == plain[2][2].tobytes()
        counts, out, kept = dev.classify(upload_relative(cases.scene(1), None, None, ZERO, other), None, keep=5, return_kept=True, ctx=ctx)
        w = want.classify(cases.scene(1))
        assert counts == w["counts"] and np.array_equal(kept, np.nonzero(w["state"] != 1)[0]) and out.size() == len(kept)
        res = dev.export(ctx=ctx)
        assert np.array_equal(res["indices"], want.export()[0])
    finally:
        ctx.set_stream_ordered(False)
        other.set_stream_ordered(False)


# ---- 6. the launch and wait counters --------------------------------------------------------------------------------------------------------
def test_the_counters_rise_by_the_documented_amounts():
    others = (sga.cloud_crop_launches(), sga.cloud_visibility_launches(), sga.cloud_outliers_launches())
    origin, leaf, dims = cases.CASES["F"][:3]

    def delta(call):
        a = (sga.occupancy_launches(), sga.occupancy_waits())
        call()
        return sga.occupancy_launches() - a[0], sga.occupancy_waits() - a[1]

    made = []
    assert delta(lambda: made.append(sga.OccupancyGrid(origin, leaf, dims))) == (2, 0)  # the fills of the cells and of the counter block
    dev = made[0]
    scan, cl = upload_relative(cases.scan_of(5, 0, 340, 50), None, None, ZERO), upload_relative(cases.scene(5, 340, 50), None, None, ZERO)
    T = cases.POSES[0]
    assert delta(lambda: dev.integrate(scan, T, *cases.RANGES)) == (2, 0)  # the endpoints, the walk; no host wait
    assert delta(lambda: dev.integrate(scan, T, *cases.RANGES, return_stats=True)) == (2, 1)
    assert delta(lambda: dev.integrate(scan, T, *cases.RANGES, mode=1)) == (1, 0)
    assert delta(lambda: dev.integrate(scan, T, *cases.RANGES, mode=1, return_stats=True)) == (1, 1)
    assert delta(lambda: dev.classify(cl)) == (1, 1)
    assert delta(lambda: dev.classify(cl, return_state=True)) == (1, 1)
    assert delta(lambda: dev.classify(cl, keep=5, return_kept=True)) == (3, 1)  # ... the compaction's table copy, the compaction; its wait
    assert delta(lambda: dev.stats()) == (1, 1)
    assert delta(lambda: dev.export()) == (3, 2)  # the count and its wait; the offsets, the fill and theirs
    assert delta(lambda: dev.export(threshold=100.0)) == (1, 1)  # nothing is occupied: no fill
    assert delta(lambda: dev.download()) == (0, 1)
    assert delta(lambda: dev.clear()) == (1, 0)
    assert (sga.cloud_crop_launches(), sga.cloud_visibility_launches(), sga.cloud_outliers_launches()) == others


# ---- 7. meaning -----------------------------------------------------------------------------------------------------------------------------
def test_free_space_clears_the_trail_of_a_mover_and_no_static_wall_cell():
    M = cases.MEANING
    frames, origin = cases.meaning_frames()
    ghosts = {}
    for mode in (0, 1):
        want, _ = cases.meaning_reference(mode)
        dev = sga.OccupancyGrid(origin, M["leaf"], M["dims"])
        probe = ref.Grid(origin, M["leaf"], M["dims"])
        for f, (pts, _, Tws) in enumerate(frames):
            integrate_both(dev, probe, pts, Tws, M["min_range"], M["max_range"], mode, what="mover, mode %d, frame %d" % (mode, f))
        same_cells(dev, want, "the meaning case, mode %d" % mode)
        counts = dev.stats()
        assert tuple(counts[w] for w in NAMES) == M["cells"][mode]
        res = dev.export()
        ghosts[mode] = cases.ghost_cells(res["indices"], cell_records(res["cloud"]), origin)
        assert len(ghosts[mode]) == M["ghosts"][mode]  # the pinned figures: 24 with free space, 74 with the endpoints alone
        if mode == 0:
            wall = cases.static_wall_cells(want)
            stamp, L = dev.download()
            assert len(wall) == M["wall_cells"] and np.all(stamp.reshape(-1)[wall] != 0) and np.all(L.reshape(-1)[wall] >= 0.0)  # no cell on the static wall turns free
    assert ghosts[0] <= ghosts[1]
    print("occupied cells on the mover's trail: %d with the endpoints alone, %d with free space" % (len(ghosts[1]), len(ghosts[0])))


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------------------
def test_the_driver_reports_the_trail_for_both_modes():
    from small_gicp_amd import odometry, synthetic

    M = cases.MEANING
    frames, origin = cases.meaning_frames()
    kw = dict(leaf=M["leaf"], extent=tuple(d * M["leaf"] for d in M["dims"]), offset=M["offset"], min_range=M["min_range"], max_range=M["max_range"], poses=[Tws for _, _, Tws in frames],
              n_rings=M["n_rings"], n_az=M["n_az"])
    out = {mode: odometry.run_synthetic_occupancy(M["frames"], mover=True, mode=mode, **kw) for mode in (0, 1)}
    for mode in (0, 1):  # at the generator's poses: the meaning case's figures
        assert out[mode]["ghost_cells"] == M["ghosts"][mode] and tuple(out[mode]["cells"][w] for w in NAMES) == M["cells"][mode] and out[mode]["cells"]["epoch"] == M["frames"]
    assert set(out[0]["ghost_indices"].tolist()) <= set(out[1]["ghost_indices"].tolist())
    assert odometry.run_synthetic_occupancy(3, mover=False, **dict(kw, poses=kw["poses"][:3]))["ghost_cells"] == 0
    # at the estimated poses (the odometry runs on the scans with the mover in them)
    est = {mode: odometry.run_synthetic_occupancy(4, mover=True, mode=mode, n_rings=32, n_az=1000) for mode in (0, 1)}
    for f in range(1, 4):
        rel = np.linalg.inv(est[0]["poses"][f - 1]) @ est[0]["poses"][f]
        assert abs(np.linalg.norm(rel[:3, 3]) - 1.0) < 0.05  # each relative motion is the simulated 1 m
    assert est[0]["ghost_cells"] <= est[1]["ghost_cells"] and est[1]["ghost_cells"] > 0 and est[0]["cells"]["free"] > 0 and est[1]["cells"]["free"] == 0
    print("estimated poses, 4 frames: %d ghost cells with the endpoints alone, %d with free space" % (est[1]["ghost_cells"], est[0]["ghost_cells"]))


# ---- 9. the C++ header ----------------------------------------------------------------------------------------------------------------------
def test_cpp_occupancy(tmp_path):
    """include/small_gicp_amd.hpp: OccupancyParams and OccupancyGrid against the C calls and the restatement (tests/cpp/test_cpp_occupancy.cpp,
    compiled with g++ as test_cloud_visibility_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_occupancy"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_occupancy.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    origin, leaf, dims = cases.CASES["C"][:3]
    scan_rel = cases.scan_of(1, 0)
    (tmp_path / "scan.f32").write_bytes(scan_rel.tobytes())
    args = [str(exe), str(tmp_path / "scan.f32")] + [repr(float(v)) for v in origin] + [repr(leaf)] + [str(d) for d in dims] + ["0.5", "12.0"]
    p = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    want = ref.Grid(origin, leaf, dims)
    turn = np.array([[0, -1, 0, 1], [1, 0, 0, -2], [0, 0, 1, 0.5], [0, 0, 0, 1]], dtype=np.float64)
    stats = [want.integrate(scan_rel, T, 0.5, 12.0) for T in (None, turn)]
    assert all(st["band"] == 0 for st in stats)
    scans = [r for r in rows if r[0] == "SCAN"]
    assert len(scans) == 2
    for r, st in zip(scans, stats):  # SCAN k beams b ignored i hits h truncated t cells_hit c cells_freed f
        assert [int(v) for v in r[3::2]] == [st[w] for w in SCAN_NAMES], r
    counts = want.stats()
    assert [r for r in rows if r[0] == "STATS"] == [["STATS", "total", str(counts["total"]), "unknown", str(counts["unknown"]), "free", str(counts["free"]), "occupied", str(counts["occupied"]), "epoch", "2"]]
    assert [r for r in rows if r[0] == "ABI"] == [["ABI", "equal", "1"]]
    w = want.classify(scan_rel, turn)
    assert len(w["band"]) == 0
    cl = [r for r in rows if r[0] == "CLASSIFY"]
    assert [r[2] for r in cl] == ["0", "5", "2"]
    for r in cl:  # CLASSIFY mask m total n unknown u free f occupied o cloud c consistent k
        mask = int(r[2])
        assert [int(r[4]), int(r[6]), int(r[8]), int(r[10])] == [w["counts"][s] for s in ("total",) + NAMES] and r[14] == "1", r
        assert int(r[12]) == int((((mask >> w["state"].astype(np.int64)) & 1) != 0).sum()), r
    idx, _, _ = want.export()
    assert [r for r in rows if r[0] == "EXPORT"] == [["EXPORT", "count", str(len(idx)), "written", str(len(idx)), "ascending", "1", "occupied", "1", "cloud", str(len(idx)), "capped", "1"]]
    assert [r for r in rows if r[0] == "CLEAR"] == [["CLEAR", "epoch", "0", "unknown", str(want.cells)]]
    assert [r for r in rows if r[0] == "REFUSE"] == [["REFUSE", "leaf", "1", "range", "1"]]

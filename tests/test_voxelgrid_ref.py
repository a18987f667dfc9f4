"""CPU tests of tests/voxelgrid_ref.py: the restatement of the voxel grid agrees with the oracle (voxel count, order, means) on real scans,
on a geo-referenced copy and on designed clouds of the GPU matrix; the checker accepts correctly rounded centroids and rejects each kind
of defect it exists to find; the clouds of tests/test_voxelgrid_matrix.py have the shapes their cases are named after.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
import test_voxelgrid_matrix as vm
from voxelgrid_ref import centroid_bound, check_grid, downsample_ref, group_means, ulp32, voxel_coords

F32 = np.float32


def host_upload(points):
    """What an upload makes of `points` (float32 or float64), on the host: the origin sga_choose_origin picks for the box of the finite
    coordinates, and the fp32 records relative to it (the subtraction in double)."""
    p = np.asarray(points)
    p64 = p.astype(np.float64)
    fin = np.isfinite(p64)
    lo = np.ascontiguousarray(np.where(fin, p64, np.inf).min(axis=0))
    hi = np.ascontiguousarray(np.where(fin, p64, -np.inf).max(axis=0))
    origin = np.zeros(3)
    dp = C.POINTER(C.c_double)
    sga.load().sga_choose_origin(lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), origin.ctypes.data_as(dp))
    with np.errstate(over="ignore", invalid="ignore"):
        return (p64 - origin).astype(F32), origin


def rounded(ref):
    """the centroids a correct device returns: the means rounded once to fp32"""
    return ref.means.astype(F32)


def against_oracle(orc, points, leaf):
    """The restatement on the records of an upload against the oracle on the very same numbers in the caller's frame: same voxels in the
    same order; the means are two float64-or-better sums in different orders: |difference| <= 1e-12 x the largest coordinate of the voxel
    (caller's frame; relative to the mean itself the sums of a voxel that straddles 0 cancel)."""
    rec, origin = host_upload(points)
    ref = downsample_ref(rec, origin, leaf)
    out = orc.voxelgrid_sampling(rec.astype(np.float64) + origin, leaf)
    assert len(out) == len(ref.counts), (len(out), len(ref.counts))
    err = np.abs(out - (ref.means + origin))
    tol = 1e-12 * (ref.maxabs + np.abs(origin))
    assert (err <= tol).all(), (int(np.argmax((err / np.maximum(tol, 1e-300)).max(axis=1))), float((err / np.maximum(tol, 1e-300)).max()))
    return ref


@pytest.mark.parametrize("leaf", [0.1, 0.25, 1.0])
@pytest.mark.parametrize("which", ["target", "source"])
def test_restatement_agrees_with_the_oracle_on_c1(orc, c1_raw, which, leaf):
    pts = c1_raw[0] if which == "target" else c1_raw[1]
    ref = against_oracle(orc, pts, leaf)
    assert len(ref.dropped) == 0 and 0 < len(ref.counts) < len(pts)


def test_restatement_agrees_with_the_oracle_on_a_geo_referenced_copy(orc, c1_raw):
    pts = c1_raw[0].astype(np.float64) + np.array([1e5, 2e5, 300.0])
    rec, origin = host_upload(pts)
    assert origin.all() and np.abs(rec).max() < 200.0
    against_oracle(orc, pts, 0.25)


@pytest.mark.parametrize("name", ["run shapes", "lattice points", "outliers"])
def test_restatement_agrees_with_the_oracle_on_designed_clouds(orc, name):
    pts = {"run shapes": vm.run_shapes_cloud, "lattice points": vm.boundary_cloud,
           "outliers": lambda: vm.with_bad(vm.scan(20_000, 6), [[3e5, 0, 0], [-3e5, 0, 0], [0, 2.7e5, 1], [0, -2.7e5, 1]])}[name]()
    for leaf in (0.25, 0.1):
        ref = against_oracle(orc, pts, leaf)
        if name == "outliers" and leaf == 0.25:
            assert len(ref.dropped) == 4
        if name == "run shapes" and leaf == 0.25:
            assert sorted(ref.counts.tolist()) == vm.RUNS


def test_reciprocal_multiply_not_division(orc):
    """the coordinate is floor(p * (1 / leaf)): on the lattice of leaf 0.7 that is not floor(p / leaf) everywhere, and the oracle agrees"""
    rec = vm.reciprocal_cloud()
    c, keep = voxel_coords(rec, np.zeros(3), 0.7)
    x = rec[:, 0].astype(np.float64)
    assert keep.all() and (c[:, 0] == np.floor(x * (1.0 / 0.7))).all()
    differ = c[:, 0] != np.floor(x / 0.7)
    assert differ.sum() > 1000 and np.abs(x[differ]).min() == 10.5
    against_oracle(orc, rec, 0.7)


def test_drop_rule_and_order():
    leaf = 0.5
    rec = np.array([[0, 0, 0], [-(2**20) * leaf, 0, 0], [np.nextafter(F32(-(2**20) * leaf), F32(-np.inf)), 0, 0], [(2**20) * leaf, 0, 0], [np.nextafter(F32((2**20) * leaf), F32(0)), 0, 0],
                    [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1, 0, 1e9], [0, -3e38, 0], [0.7, 0, -0.2], [-0.2, 0.7, 0], [0.2, 0.2, 0.2]], F32)
    ref = downsample_ref(rec, np.zeros(3), leaf)
    assert ref.dropped.tolist() == [2, 3, 5, 6, 7, 8, 9]
    # ascending (z, y, x)
    assert ref.coords.tolist() == [[1, 0, -1], [-(2**20), 0, 0], [0, 0, 0], [2**20 - 1, 0, 0], [-1, 1, 0]]
    assert ref.counts.tolist() == [1, 1, 2, 1, 1] and ref.means[2].tolist() == [0.10000000149011612 / 1, 0.10000000149011612, 0.10000000149011612]
    # the origin takes part: the same records one voxel further along x
    assert downsample_ref(rec[[0, 12]], np.array([leaf, 0, 0]), leaf).coords.tolist() == [[1, 0, 0]]
    empty = downsample_ref(rec[[5, 6]], np.zeros(3), leaf)
    assert len(empty.counts) == 0 and empty.means.shape == (0, 3) and check_grid(np.zeros((0, 3), F32), empty) == 0.0


def test_ulp32():
    for x in (1.0, 1.5, 60.0, 2.0**-100, 3e38, 0.75):
        assert ulp32(x) == float(np.spacing(F32(x)))
    assert ulp32(2.0) == 2.0**-22 and ulp32(np.nextafter(2.0, 0.0)) == 2.0**-23
    assert ulp32(0.0) == 2.0**-126 and ulp32(1e-45) == 2.0**-126 and ulp32(2.0**-103) == 2.0**-126 and ulp32(2.0**-102) == 2.0**-125


# ---- the checker -----------------------------------------------------------------------------------------------------------------------
def _scene():
    pts = vm.with_bad(vm.scan(30_000, 3), [[3e5, 0, 0], [-3e5, 0, 0], [np.nan, 1, 1]])
    rec, origin = host_upload(pts)
    assert not origin.any()
    return rec, origin, 0.25


def test_checker_accepts_the_rounded_means_on_every_cloud_of_the_matrix_but_the_largest():
    for c in vm.CASES:
        pts = c.make() if not c.label.startswith("size") or int(c.label.split()[1]) <= 4097 else None
        if pts is None:
            continue
        rec, origin = host_upload(pts)
        ref = downsample_ref(rec, origin, c.leaf)
        assert check_grid(rounded(ref), ref, c.label) <= 1.0
        vm.assert_shape(c.label, len(pts), ref)


def test_checker_rejects_a_point_moved_to_the_neighbouring_voxel():
    rec, origin, leaf = _scene()
    ref = downsample_ref(rec, origin, leaf)
    c, keep = voxel_coords(rec, origin, leaf)
    c = np.where(keep[:, None], c, 0.0)
    # a point of a voxel whose x-neighbour is occupied as well, so that the number of voxels stays what it was
    occupied = {tuple(v) for v in ref.coords.tolist()}
    i = next(k for k in np.flatnonzero(keep) if (c[k, 0] + 1, c[k, 1], c[k, 2]) in occupied and ref.counts[ref.coords.tolist().index(c[k].astype(int).tolist())] > 1)
    c[i, 0] += 1
    wrong = group_means(rec, c, keep)
    assert len(wrong.counts) == len(ref.counts)
    with pytest.raises(AssertionError, match="centroid outside the bound"):
        check_grid(rounded(wrong), ref)


def test_checker_rejects_two_rows_swapped():
    rec, origin, leaf = _scene()
    ref = downsample_ref(rec, origin, leaf)
    out = rounded(ref)
    out[[100, 101]] = out[[101, 100]]
    with pytest.raises(AssertionError, match=r"centroid outside the bound.*\(100, "):
        check_grid(out, ref)


def test_checker_rejects_a_centroid_one_ulp_off():
    """One fp32 step AWAY from the mean is outside the bound for every coordinate of every row (a step towards it may land on the other
    fp32 neighbour of a mean that lies between two floats: that one is as good)."""
    rec, origin, leaf = _scene()
    ref = downsample_ref(rec, origin, leaf)
    good = rounded(ref)
    away = np.where(good.astype(np.float64) >= ref.means, np.nextafter(good, F32(np.inf)), np.nextafter(good, F32(-np.inf)))
    assert (np.abs(away.astype(np.float64) - ref.means) > centroid_bound(away, ref)).all()
    out = good.copy()
    out[777, 2] = away[777, 2]
    with pytest.raises(AssertionError, match=r"centroid outside the bound.*\(777, 2\)"):
        check_grid(out, ref)
    # and so is one step anywhere on a single-point voxel, whose mean is a float
    single = int(np.flatnonzero(ref.counts == 1)[5])
    for direction in (np.inf, -np.inf):
        out = good.copy()
        out[single, 0] = np.nextafter(out[single, 0], F32(direction))
        with pytest.raises(AssertionError, match="centroid outside the bound"):
            check_grid(out, ref)


def test_checker_rejects_a_dropped_point_kept():
    rec, origin, leaf = _scene()
    ref = downsample_ref(rec, origin, leaf)
    c, keep = voxel_coords(rec, origin, leaf)
    far = int(np.flatnonzero(rec[:, 0] == F32(3e5))[0])
    assert not keep[far]
    keep2 = keep.copy()
    keep2[far] = True
    # kept in a voxel of its own: one row too many
    c2 = np.where(keep2[:, None], c, 0.0)
    with pytest.raises(AssertionError, match="voxels"):
        check_grid(rounded(group_means(rec, c2, keep2)), ref)
    # kept in the last voxel of the grid along x (clamped), which a point occupies already: a centroid moves
    rec3 = np.r_[rec, [[np.nextafter(F32(2**20 * leaf), F32(0)), 0.1, 0.1]]].astype(F32)
    ref3 = downsample_ref(rec3, origin, leaf)
    c3, keep3 = voxel_coords(rec3, origin, leaf)
    keep3[far] = True
    c3 = np.where(keep3[:, None], c3, 0.0)
    c3[far] = c3[-1]
    wrong = group_means(rec3, c3, keep3)
    assert len(wrong.counts) == len(ref3.counts)
    with pytest.raises(AssertionError, match="centroid outside the bound"):
        check_grid(rounded(wrong), ref3)


def test_checker_rejects_a_kept_point_dropped():
    rec, origin, leaf = _scene()
    ref = downsample_ref(rec, origin, leaf)
    c, keep = voxel_coords(rec, origin, leaf)
    c = np.where(keep[:, None], c, 0.0)
    rows = ref.coords.tolist()
    many = next(int(k) for k in np.flatnonzero(keep) if ref.counts[rows.index(c[k].astype(int).tolist())] > 1)
    alone = next(int(k) for k in np.flatnonzero(keep) if ref.counts[rows.index(c[k].astype(int).tolist())] == 1)
    for k, what in ((many, "centroid outside the bound"), (alone, "voxels")):
        keep2 = keep.copy()
        keep2[k] = False
        with pytest.raises(AssertionError, match=what):
            check_grid(rounded(group_means(rec, c, keep2)), ref)


def test_checker_rejects_other_types_and_non_finite_rows():
    rec, origin, leaf = _scene()
    ref = downsample_ref(rec, origin, leaf)
    with pytest.raises(AssertionError):
        check_grid(ref.means, ref)  # float64: not what the device returns
    out = rounded(ref)
    out[3, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check_grid(out, ref)

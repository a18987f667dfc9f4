"""tests/voxelgrid_ref.py — the definition of sga_voxelgrid_sampling (csrc/preprocess.hip; util/downsampling.hpp:23-78 as this project
implements it), restated in numpy float64, and the checker of any cloud the device hands out.  Numpy only.

The grid.  The device holds fp32 records p' = fl32(p - origin) and the origin (double) of their frame.  The voxel of a point is decided in
the CALLER's frame, on the numbers the device holds: c = floor((float64(p') + origin) * (1.0 / leaf)) per axis — a multiplication by the
reciprocal, as the reference does, not a division (the two differ at lattice points of a leaf like 0.1).  A point is dropped when any of
its coordinates is not finite or when c + 2^20 lies outside [0, 2^21 - 1] on any axis.  The output has one row per occupied voxel, in
ascending order of the reference's key x | y << 21 | z << 42: (z, y, x) lexicographic.  A row is the mean of the voxel's RECORDS (the
output stays in the input's device frame and keeps its origin), summed here in extended precision.  Everything dropped: an empty cloud.

The bound a device centroid must meet (check_grid), per coordinate, N = points of the voxel:

    |out - mean| <= ulp32(max(|out|, |mean|)) / 2 + 2 (N + 2) 2^-53 max|p_i|

the single rounding of the fp64 quotient to fp32, plus the device's fp64 accumulation of N terms and its reciprocal multiply, doubled to
cover the summation of this file (which is far more accurate than that: 64-bit mantissas, or math.fsum).  ulp32 is floored at 2^-126."""
import math
from typing import NamedTuple

import numpy as np

OFFSET = 1 << 20  # coord_offset
TOP = (1 << 21) - 1  # coord_bit_mask


class VoxelGrid(NamedTuple):
    coords: np.ndarray   # (M, 3) int64 voxel coordinates (without the 2^20 offset), in output order
    counts: np.ndarray   # (M,) points per voxel
    means: np.ndarray    # (M, 3) float64 mean of the voxel's records
    maxabs: np.ndarray   # (M, 3) float64 max |record| per axis
    dropped: np.ndarray  # indices of the points without a voxel, ascending


def voxel_coords(records32, origin, leaf):
    """((n, 3) float64 floor coordinates — not finite / huge where the point has none —, (n,) bool: the point is kept)."""
    rec = np.asarray(records32, dtype=np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor((rec.astype(np.float64) + np.asarray(origin, dtype=np.float64)) * (1.0 / float(leaf)))
        keep = np.isfinite(rec).all(axis=1) & ((c + OFFSET >= 0) & (c + OFFSET <= TOP)).all(axis=1)
    return c, keep


def group_means(records32, coords, keep):
    """The grid of the kept points under the given per-point voxel coordinates (the partition is an argument so that the tests of the
    checker can hand in a wrong one)."""
    rec = np.asarray(records32, dtype=np.float32).reshape(-1, 3)
    idx = np.flatnonzero(keep)
    dropped = np.flatnonzero(~np.asarray(keep))
    if len(idx) == 0:
        z = np.zeros((0, 3))
        return VoxelGrid(z.astype(np.int64), np.zeros(0, np.int64), z, z.copy(), dropped)
    c = np.asarray(coords)[idx].astype(np.int64)
    perm = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))  # z is the most significant, x the least
    c, r = c[perm], rec[idx[perm]].astype(np.float64)
    starts = np.flatnonzero(np.r_[True, (c[1:] != c[:-1]).any(axis=1)])
    counts = np.diff(np.r_[starts, len(c)])
    if np.finfo(np.longdouble).nmant >= 63:
        sums = np.add.reduceat(r.astype(np.longdouble), starts, axis=0)
        means = (sums / counts[:, None].astype(np.longdouble)).astype(np.float64)
    else:  # no extended precision here: exact sums, one voxel at a time
        ends = starts + counts
        means = np.array([[math.fsum(r[s:e, k]) / (e - s) for k in range(3)] for s, e in zip(starts, ends)])
    maxabs = np.maximum.reduceat(np.abs(r), starts, axis=0)
    return VoxelGrid(c[starts], counts, means, maxabs, dropped)


def downsample_ref(records32, origin, leaf):
    """The voxel grid of the records (n, 3) float32 of a cloud with the given origin."""
    c, keep = voxel_coords(records32, origin, leaf)
    return group_means(records32, np.where(keep[:, None], c, 0.0), keep)


def ulp32(x):
    """The spacing of float32 at |x| (x float64), floored at 2^-126."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    _, e = np.frexp(a)  # |x| = m 2^e, 0.5 <= m < 1 (e = 0 for x = 0)
    return np.ldexp(1.0, np.where(a > 0, np.maximum(e - 24, -126), -126))


def centroid_bound(out, ref):
    """(M, 3) float64: the bound above for every coordinate of `out` (M, 3) against the grid `ref`."""
    o = np.asarray(out, dtype=np.float64)
    return 0.5 * ulp32(np.maximum(np.abs(o), np.abs(ref.means))) + 2.0 * (ref.counts[:, None] + 2.0) * 2.0**-53 * ref.maxabs


def check_grid(out, ref, label=""):
    """Assert that `out` (M', 3) float32 — device-frame centroids as the device returned them — is the grid `ref`: as many rows, every
    coordinate of every row within centroid_bound (which also proves the order: a row out of place is another voxel's centroid).
    Returns the largest |out - mean| / bound."""
    o = np.asarray(out)
    assert o.dtype == np.float32 and o.ndim == 2 and o.shape[1] == 3, (label, o.dtype, o.shape)
    assert len(o) == len(ref.counts), (label, "voxels", len(o), "expected", len(ref.counts), "dropped points", len(ref.dropped))
    if len(o) == 0:
        return 0.0
    assert np.isfinite(o).all(), (label, "non-finite centroid in row", int(np.flatnonzero(~np.isfinite(o).all(axis=1))[0]))
    err = np.abs(o.astype(np.float64) - ref.means)
    ratio = err / centroid_bound(o, ref)
    bad = ratio > 1.0
    if bad.any():
        i, k = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError((label, "centroid outside the bound: row, axis", (i, k), "of", len(o), "voxel", ref.coords[i].tolist(), "points", int(ref.counts[i]), "got", float(o[i, k]), "mean",
                              float(ref.means[i, k]), "error / bound", float(ratio[i, k]), "rows outside", int(bad.any(axis=1).sum())))
    return float(ratio.max())

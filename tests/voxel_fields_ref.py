"""tests/voxel_fields_ref.py — the definition of sga_voxelgrid_sampling_fields (csrc/preprocess.hip) restated in
numpy float64, and the checker of what the device hands out.  Numpy only.

The partition is voxelgrid_ref's: downsample_ref decides which points are kept, which voxel a kept point falls into and the order of the
voxels; voxel v is row v.  The members of a voxel are taken in ascending original index.  Per column, under its op:

    MEAN     the mean of the N values, summed in extended precision.  The device's fl32(S / N), S summed in double, must meet
             |out - mean| <= ulp32(max(|out|, |mean|)) / 2 + 2 (N + 2) 2^-53 max|v_i|   (voxelgrid_ref's bound for a centroid coordinate);
             a NaN among the values makes the mean NaN on both sides.
    MIN/MAX  the least / greatest value that is not NaN; NaN when all are.  Compared with == (the sign of a zero is free).
    FIRST    the value of the member of lowest index, compared bit for bit.
    NEAREST  the value, bit for bit, of the member that minimises d2 = (dx dx + dy dy) + dz dz, d = float64(record) - float64(centroid),
             every product and sum rounded to double, ties to the lowest index.  The centroid is an ARGUMENT (the fp32 records the
             device wrote for the voxels: what the call itself is defined by); reduce_ref also reports, per voxel, whether the best d2 and
             the best d2 among the members whose record is not bit-identical to the winner's differ by less than 1e-12 relative — a
             voxel where the choice would hang on the last bits of the arithmetic.  The GPU tests fail on such a voxel (their seeds are
             chosen so that there is none), they do not skip it.

counts[v] = N; voxel_of[i] = the row of point i, -1 for a dropped point."""
from typing import NamedTuple

import numpy as np

from voxelgrid_ref import OFFSET, downsample_ref, ulp32, voxel_coords

MEAN, MIN, MAX, FIRST, NEAREST = range(5)
NEAR_TIE = 1e-12


class Partition(NamedTuple):
    grid: object          # voxelgrid_ref.VoxelGrid: coords, counts, means (float64), maxabs, dropped
    counts: np.ndarray    # (M,) int32
    voxel_of: np.ndarray  # (n,) int64, -1: dropped
    order: np.ndarray     # the kept points sorted by (row, index)
    starts: np.ndarray    # (M,) where row v begins in `order`


def _key(c):
    c = np.asarray(c, dtype=np.int64) + OFFSET
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def partition_ref(records32, origin, leaf, coords=None, keep=None):
    """Which row every point falls into.  coords / keep: another assignment than the definition's (the tests of the checker hand in a
    wrong one); the rows are then the occupied voxels of THAT assignment in ascending key order."""
    rec = np.asarray(records32, dtype=np.float32).reshape(-1, 3)
    if coords is None:
        grid = downsample_ref(rec, origin, leaf)
        coords, keep = voxel_coords(rec, origin, leaf)
    else:
        from voxelgrid_ref import group_means

        grid = group_means(rec, np.where(np.asarray(keep)[:, None], coords, 0.0), keep)
    voxel_of = np.full(len(rec), -1, np.int64)
    idx = np.flatnonzero(keep)
    if len(idx):
        voxel_of[idx] = np.searchsorted(_key(grid.coords), _key(np.asarray(coords)[idx].astype(np.int64)))
    order = idx[np.argsort(voxel_of[idx], kind="stable")]  # ascending index inside a row
    counts = np.asarray(grid.counts, dtype=np.int32)
    starts = np.r_[0, np.cumsum(counts)[:-1]].astype(np.int64) if len(counts) else np.zeros(0, np.int64)
    return Partition(grid, counts, voxel_of, order, starts)


class Reduced(NamedTuple):
    values: np.ndarray    # (M, dim) float64: the mean (MEAN), else the float32 value chosen, widened
    maxabs: np.ndarray    # (M, dim) float64: max |v_i| of the members (the MEAN bound's)
    near_tie: np.ndarray  # (M,) bool: NEAREST hangs on the last bits (see above); all False without a NEAREST column
    winner: np.ndarray    # (M,) int64: the member NEAREST chooses (-1 without a NEAREST column)


def reduce_ref(part, fields32, ops, records32=None, centroids32=None):
    f = np.asarray(fields32, dtype=np.float32)
    f = f.reshape(len(f), -1)
    M, dim = len(part.counts), f.shape[1]
    assert len(ops) == dim
    values, maxabs = np.zeros((M, dim)), np.zeros((M, dim))
    near, winner = np.zeros(M, bool), np.full(M, -1, np.int64)
    if M == 0:
        return Reduced(values, maxabs, near, winner)
    o, s = part.order, part.starts
    seg = np.repeat(np.arange(M), part.counts)
    if NEAREST in list(ops):
        rec = np.asarray(records32, dtype=np.float32).reshape(-1, 3)
        cen = np.asarray(centroids32, dtype=np.float32).reshape(-1, 3)
        assert len(cen) == M
        d = rec[o].astype(np.float64) - cen[seg].astype(np.float64)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        best = np.minimum.reduceat(d2, s)
        pos = np.where(d2 == best[seg], np.arange(len(o)), len(o))
        wpos = np.minimum.reduceat(pos, s)  # the first member (lowest index) at the least distance
        winner = o[wpos]
        same = (rec[o].view(np.uint32) == rec[winner][seg].view(np.uint32)).all(axis=1)
        second = np.minimum.reduceat(np.where(same, np.inf, d2), s)
        near = np.isfinite(second) & (second - best <= NEAR_TIE * second)
    fs = f[o].astype(np.float64)
    for c, op in enumerate(ops):
        col = fs[:, c]
        with np.errstate(invalid="ignore"):
            maxabs[:, c] = np.fmax.reduceat(np.abs(col), s)
        if op == MEAN:
            if np.finfo(np.longdouble).nmant >= 63:
                values[:, c] = (np.add.reduceat(col.astype(np.longdouble), s) / part.counts.astype(np.longdouble)).astype(np.float64)
            else:
                import math

                values[:, c] = [math.fsum(col[a:a + k]) / k if np.isfinite(col[a:a + k]).all() else np.nan for a, k in zip(s, part.counts)]
        elif op == MIN:
            values[:, c] = np.fmin.reduceat(col, s)
        elif op == MAX:
            values[:, c] = np.fmax.reduceat(col, s)
        elif op == FIRST:
            values[:, c] = col[s]
        elif op == NEAREST:
            values[:, c] = f[winner, c].astype(np.float64)
        else:
            raise ValueError(op)
    return Reduced(values, maxabs, near, winner)


def mean_bound(out, ref_mean, counts, maxabs):
    o = np.asarray(out, dtype=np.float64)
    return 0.5 * ulp32(np.maximum(np.abs(o), np.abs(ref_mean))) + 2.0 * (np.asarray(counts, dtype=np.float64) + 2.0) * 2.0**-53 * maxabs


def check_fields(part, red, ops, out_fields, counts=None, voxel_of=None, label=""):
    """Assert that what the device returned is the restatement: counts and voxel_of equal (and consistent with each other), every MEAN
    column inside its bound, every other column equal (== for MIN / MAX, bits for FIRST / NEAREST), no NEAREST voxel on a near tie.
    out_fields None: membership only.  Returns the largest |out - mean| / bound of the MEAN columns (0.0 without one)."""
    M = len(part.counts)
    if counts is not None:
        c = np.asarray(counts)
        assert c.dtype == np.int32 and c.shape == (M,), (label, "counts", c.dtype, c.shape, "voxels", M)
        assert np.array_equal(c, part.counts), (label, "counts differ in row", int(np.flatnonzero(c != part.counts)[0]))
    if voxel_of is not None:
        v = np.asarray(voxel_of)
        assert v.dtype == np.int64 and v.shape == part.voxel_of.shape, (label, "voxel_of", v.dtype, v.shape)
        bad = np.flatnonzero(v != part.voxel_of)
        assert len(bad) == 0, (label, "voxel_of differs at point", int(bad[0]), "got", int(v[bad[0]]), "expected", int(part.voxel_of[bad[0]]), "points off", len(bad))
        if counts is not None:
            assert np.array_equal(np.bincount(v[v >= 0], minlength=M), np.asarray(counts)), (label, "bincount(voxel_of) != counts")
    if out_fields is None:
        return 0.0
    o = np.asarray(out_fields)
    assert o.dtype == np.float32 and o.shape == (M, len(ops)), (label, o.dtype, o.shape, "expected", (M, len(ops)))
    assert not red.near_tie.any(), (label, "NEAREST hangs on the last bits in voxel", int(np.flatnonzero(red.near_tie)[0]), "voxels", int(red.near_tie.sum()), "of", M)
    worst = 0.0
    for c, op in enumerate(ops):
        got, ref = o[:, c], red.values[:, c]
        if op == MEAN:
            nan_ref = np.isnan(ref)
            assert np.array_equal(np.isnan(got), nan_ref), (label, "column", c, "NaN means differ")
            with np.errstate(invalid="ignore"):
                ratio = np.where(nan_ref, 0.0, np.abs(got.astype(np.float64) - ref) / mean_bound(got, ref, part.counts, red.maxabs[:, c]))
            bad = np.flatnonzero(~(ratio <= 1.0))
            assert len(bad) == 0, (label, "MEAN outside the bound: column, row", (c, int(bad[0])), "points", int(part.counts[bad[0]]), "got", float(got[bad[0]]), "mean", float(ref[bad[0]]), "error / bound", float(ratio[bad[0]]), "rows outside", len(bad))
            worst = max(worst, float(ratio.max()) if M else 0.0)
        elif op in (MIN, MAX):
            ok = (got.astype(np.float64) == ref) | (np.isnan(got) & np.isnan(ref))
            assert ok.all(), (label, "MIN" if op == MIN else "MAX", "column, row", (c, int(np.flatnonzero(~ok)[0])), "got", float(got[~ok][0]), "expected", float(ref[~ok][0]), "rows off", int((~ok).sum()))
        else:
            ok = got.view(np.uint32) == ref.astype(np.float32).view(np.uint32)
            assert ok.all(), (label, "FIRST" if op == FIRST else "NEAREST", "column, row", (c, int(np.flatnonzero(~ok)[0])), "got", float(got[~ok][0]), "expected", float(ref[~ok][0]), "rows off", int((~ok).sum()))
    return worst


# ---- the clouds of the tests -----------------------------------------------------------------------------------------------------------
# NEAREST on random data: a voxel of exactly TWO members has them at (nearly) the same distance from their mean — exactly the same
# whenever the fp32 midpoint is exact on all three axes, which for random fp32 coordinates is about one such voxel in eight — so no
# seed of a scene with thousands of two-member voxels is free of near ties.  The clouds below therefore place their points voxel by
# voxel, with member counts drawn from 1, 3, 4, ... 9 (about five on average, never two); three or more random members tie to 1e-12
# with a probability of that order.  The points with a NaN coordinate are extra points, not members.
MEMBER_COUNTS = np.array([1, 3, 4, 5, 6, 7, 8, 9])


def grouped_cloud(n, seed, leaf, base=(0.0, 0.0, 0.0), clump=300, nan_share=0.01):
    """(points (n, 3) float64 in the caller's frame, fields (n, 3) float32: a time in [0, 1], an intensity, an integer label).  n points
    in shuffled order: n * nan_share with one NaN coordinate, `clump` in one voxel, the rest in voxels of 1, 3, 4, .. 9 members strictly
    inside them (5 % to 95 % of the edge), the voxels scattered over a cube four times their number."""
    rng = np.random.default_rng(seed)
    n_nan = int(n * nan_share)
    clump = min(clump, max(n - n_nan - 1, 0))
    rest = n - n_nan - clump
    counts = []
    while rest > 0:
        k = int(rng.choice(MEMBER_COUNTS))
        if k > rest:
            k = rest
        if k == 2:
            k = 1
        counts.append(k)
        rest -= k
    counts = np.array(counts + ([clump] if clump else []), dtype=np.int64)
    V = len(counts)
    side = int(np.ceil((4.0 * V) ** (1.0 / 3.0))) + 1
    cells = rng.choice(side**3, V, replace=False)
    coords = np.stack([cells % side, cells // side % side, cells // side**2], axis=1) - side // 2
    c = np.repeat(coords.astype(np.float64), counts, axis=0)
    p = (c + rng.uniform(0.05, 0.95, c.shape)) * leaf
    bad = (rng.uniform(-1.0, 1.0, (n_nan, 3)) * side * leaf / 2)
    bad[np.arange(n_nan), rng.integers(0, 3, n_nan)] = np.nan
    p = np.r_[p, bad][rng.permutation(n)] + np.asarray(base, dtype=np.float64)
    fields = np.stack([rng.random(n), rng.random(n) * 255.0, rng.integers(0, 20, n)], axis=1).astype(np.float32)
    assert p.shape == (n, 3)
    return p, fields

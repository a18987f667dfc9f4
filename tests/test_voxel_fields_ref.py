"""The checker of tests/voxel_fields_ref.py checks: it accepts the restatement's own output and rejects a wrong partition, a MEAN outside
its bound, a MIN that is another voxel's, a NEAREST that is the second nearest, a voxel_of off by one row and a NEAREST voxel on a near
tie.  No device."""
import numpy as np
import pytest

from voxel_fields_ref import FIRST, MAX, MEAN, MIN, NEAREST, check_fields, grouped_cloud, partition_ref, reduce_ref
from voxelgrid_ref import voxel_coords

LEAF = 0.5
OPS = [MEAN, MIN, MAX, FIRST, NEAREST]


def make(seed=3, n=1500):
    p, fields3 = grouped_cloud(n, seed, LEAF)
    rec = p.astype(np.float32)
    rng = np.random.default_rng(seed + 1)
    fields = np.c_[fields3, rng.standard_normal(n), rng.random(n)].astype(np.float32)[:, [0, 1, 3, 2, 4]]
    return rec, np.zeros(3), fields


def own_output(rec, origin, fields, part=None):
    part = part or partition_ref(rec, origin, LEAF)
    cen = part.grid.means.astype(np.float32)
    red = reduce_ref(part, fields, OPS, rec, cen)
    out = red.values.astype(np.float32)
    return part, red, out


def test_accepts_its_own_output():
    rec, origin, fields = make()
    part, red, out = own_output(rec, origin, fields)
    assert len(part.counts) > 100 and part.counts.max() == 300 and (part.voxel_of < 0).sum() == 15 and 2 not in part.counts
    assert not red.near_tie.any()
    ratio = check_fields(part, red, OPS, out, part.counts.copy(), part.voxel_of.copy())
    assert ratio <= 1.0
    assert check_fields(part, red, OPS, None, part.counts, part.voxel_of) == 0.0  # membership only


def test_rejects_a_wrong_partition():
    rec, origin, fields = make()
    part, red, _ = own_output(rec, origin, fields)
    c, keep = voxel_coords(rec, origin, LEAF)
    wrong = partition_ref(rec, origin, LEAF, coords=np.floor(np.where(keep[:, None], c, 0.0) / 2.0), keep=keep)  # voxels of twice the leaf
    _, _, wout = own_output(rec, origin, fields, wrong)
    with pytest.raises(AssertionError):
        check_fields(part, red, OPS, wout, wrong.counts, wrong.voxel_of)
    with pytest.raises(AssertionError, match="voxel_of"):
        check_fields(part, red, OPS, None, None, wrong.voxel_of)


def test_rejects_a_mean_outside_the_bound():
    rec, origin, fields = make()
    part, red, out = own_output(rec, origin, fields)
    v = int(np.argmax(part.counts))
    bad = out.copy()
    bad[v, 0] = np.nextafter(np.nextafter(bad[v, 0], np.float32(np.inf)), np.float32(np.inf))  # two ulps: the bound is half of one plus 1e-15
    with pytest.raises(AssertionError, match="MEAN outside the bound"):
        check_fields(part, red, OPS, bad)


def test_rejects_a_min_of_another_voxel():
    rec, origin, fields = make()
    part, red, out = own_output(rec, origin, fields)
    bad = out.copy()
    bad[3, 1] = out[4, 1]
    assert bad[3, 1] != out[3, 1]
    with pytest.raises(AssertionError, match="MIN"):
        check_fields(part, red, OPS, bad)


def test_rejects_the_second_nearest():
    rec, origin, fields = make()
    part, red, out = own_output(rec, origin, fields)
    v = int(np.argmax(part.counts))
    members = part.order[part.starts[v]:part.starts[v] + part.counts[v]]
    cen = part.grid.means.astype(np.float32)[v].astype(np.float64)
    d2 = ((rec[members].astype(np.float64) - cen) ** 2).sum(axis=1)
    second = members[np.argsort(d2, kind="stable")[1]]
    assert members[np.argmin(d2)] == red.winner[v]
    bad = out.copy()
    bad[v, 4] = fields[second, 4]
    assert bad[v, 4] != out[v, 4]
    with pytest.raises(AssertionError, match="NEAREST"):
        check_fields(part, red, OPS, bad)


def test_rejects_voxel_of_off_by_one_row():
    rec, origin, fields = make()
    part, red, out = own_output(rec, origin, fields)
    bad = part.voxel_of.copy()
    i = int(np.flatnonzero(bad >= 0)[5])
    bad[i] += 1
    with pytest.raises(AssertionError, match="voxel_of differs at point"):
        check_fields(part, red, OPS, out, part.counts, bad)


def test_flags_a_near_tie_but_not_a_duplicate():
    rec = np.array([[0.125, 0.125, 0.125], [0.375, 0.125, 0.125], [0.125, 0.125, 0.125], [0.375, 0.125, 0.125]], np.float32)  # two pairs of duplicates, mirror images about the centroid
    fields = np.arange(4, dtype=np.float32)
    part = partition_ref(rec, np.zeros(3), LEAF)
    assert list(part.counts) == [4]
    red = reduce_ref(part, fields, [NEAREST], rec, part.grid.means.astype(np.float32))
    assert red.near_tie[0]  # the two distinct records are equally far: the choice hangs on the last bits
    with pytest.raises(AssertionError, match="hangs on the last bits"):
        check_fields(part, red, [NEAREST], red.values.astype(np.float32))
    rec2 = np.array([[0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [0.4, 0.1, 0.1]], np.float32)
    part2 = partition_ref(rec2, np.zeros(3), LEAF)
    red2 = reduce_ref(part2, fields[:3], [NEAREST], rec2, part2.grid.means.astype(np.float32))
    assert not red2.near_tie[0] and red2.winner[0] == 0 and red2.values[0, 0] == 0.0  # a real tie goes to the lowest index


def test_nan_columns():
    rec = np.full((5, 3), 0.1, np.float32) + np.arange(5, dtype=np.float32)[:, None] * 0.01
    f = np.stack([np.full(5, np.nan), [1, np.nan, 3, -2, 0]], axis=1).astype(np.float32)
    part = partition_ref(rec, np.zeros(3), LEAF)
    for op, want in ((MIN, -2.0), (MAX, 3.0), (FIRST, 1.0)):
        red = reduce_ref(part, f, [op, op], rec, None)
        assert np.isnan(red.values[0, 0]) and red.values[0, 1] == want
        check_fields(part, red, [op, op], red.values.astype(np.float32))
    red = reduce_ref(part, f, [MEAN, MEAN], rec, None)
    assert np.isnan(red.values).all()
    check_fields(part, red, [MEAN, MEAN], red.values.astype(np.float32))

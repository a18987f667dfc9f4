"""The row sum that ends every linearization pass (csrc/reduce_rows.hpp: reduce_rows_kernel through launch_reduce) adds its rows in ONE
documented, fixed order — the results of a registration are bit-reproducible because of it.  This file states that order in numpy and
compares the kernel with it BITWISE, on rows of mixed magnitude (any other order of the additions changes bits):

  G = reduce_groups(rows) workgroups, 8 slices each.  Chain (g, s) takes rows g + G s, g + G (s + 8), g + G (s + 16), ... in that
  order: while four or more rows remain, the next four go to the accumulators a0, a1, a2, a3 (all starting at +0.0); the (up to three)
  rows left at the end go to a0 one after the other; the chain's value is (a0 + a1) + (a2 + a3).  The eight slices of a workgroup are
  folded in order 0 .. 7 starting from +0.0: one stage row per workgroup.  With G > 1 slice s then adds the stage rows s, s + 8, ...
  in order starting from +0.0, and the eight slices are folded again in order.  Columns 0 .. 94 are summed, column 95 is 0.

The restatement was checked once against the build of the parent commit on an MI355X (the kernels untouched, only the entry point
sga_debug_reduce_rows added) before any kernel was edited: all cases below were bit-equal.  It is a yardstick, not a copy of the
code under test.  The same was done for the restatement of the derived columns (restated_derived) at the end of the file.
"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga

pytestmark = pytest.mark.gpu

ROW, COLS, SLICES, MAX_GROUPS = 96, 95, 8, 64


def reduce_groups(nrows):
    return min(MAX_GROUPS, max(8, nrows // 128)) if nrows > 256 else 1


def chain_sum(rows):
    a = [np.zeros(rows.shape[1]) for _ in range(4)]
    full = len(rows) // 4 * 4
    for i in range(full):
        a[i % 4] = a[i % 4] + rows[i]
    for i in range(full, len(rows)):
        a[0] = a[0] + rows[i]
    return (a[0] + a[1]) + (a[2] + a[3])


def fold(slices):
    t = np.zeros(slices[0].shape[0])
    for v in slices:
        t = t + v
    return t


def restated_sum(rows):
    G = reduce_groups(len(rows))
    stage = [fold([chain_sum(rows[g + G * s :: G * SLICES]) for s in range(SLICES)]) for g in range(G)]
    total = stage[0]
    if G > 1:
        parts = []
        for s in range(SLICES):
            t = np.zeros(rows.shape[1])
            for k in range(MAX_GROUPS // SLICES):
                t = t + (stage[s + k * SLICES] if s + k * SLICES < G else 0.0)
            parts.append(t)
        total = fold(parts)
    out = np.zeros(ROW)
    out[:COLS] = total[:COLS]
    return out


def make_rows(nrows, seed):
    rng = np.random.default_rng(seed)
    rows = rng.standard_normal((nrows, ROW)) * 10.0 ** rng.uniform(-8.0, 8.0, (nrows, ROW))
    rows[rng.random((nrows, ROW)) < 0.03] = -0.0  # signed zeros: a sum that starts at +0.0 never returns -0.0
    rows[:, 7] = -0.0
    return np.ascontiguousarray(rows)


def device_sum(ctx, rows, derive=0):
    out = np.full(ROW, np.nan)
    sga._lib.check(sga.load().sga_debug_reduce_rows(ctx.h, rows.ctypes.data_as(C.c_void_p), len(rows), derive, out.ctypes.data_as(C.c_void_p)))
    return out


def assert_bits_equal(got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


# the one-workgroup boundary, 8 -> 9 workgroups, the row counts of the headline's passes (977 certify, 3 907 queue-fed, 15 625 cold), the
# 64-workgroup cap; then chains with 0 .. 3 leftover rows next to chains with one row less (5: chains of one row and empty chains;
# 37, 46, 55, 64: one workgroup, chains of 5 | 4, 6 | 5, 7 | 6, 8 rows; 300 ... 20 000: 8 ... 64 workgroups, chains of 4 to 40 rows)
ROW_COUNTS = [1, 3, 8, 255, 256, 257, 1023, 1024, 1025, 977, 3907, 8191, 15625, 5, 37, 46, 55, 64, 300, 581, 721, 1151, 2000, 5000, 10000, 11000, 17000, 20000]


@pytest.fixture(scope="module")
def ctx():
    return sga.default_context()


@pytest.mark.parametrize("nrows", ROW_COUNTS)
def test_row_sum_is_the_documented_order_bit_for_bit(ctx, nrows):
    rows = make_rows(nrows, nrows)
    want = restated_sum(rows)
    got = device_sum(ctx, rows)
    assert_bits_equal(got, want, nrows)
    assert not np.signbit(got[7])  # the column of -0.0


def test_leftover_residues_are_covered():
    """The cases above reach every number of leftover rows (chain length mod 4) with and without a hand-off between workgroups, empty
    chains, and chains longer than 16 and than 32 rows."""
    seen = set()
    for n in ROW_COUNTS:
        G = reduce_groups(n)
        for chain in range(G * SLICES):
            k = len(range(chain, n, G * SLICES))
            seen.add((G > 1, k % 4 if k else "empty", min(k // 16, 2)))
    for multi in (False, True):
        for left in range(4):
            assert any(s[0] == multi and s[1] == left for s in seen), (multi, left)
    assert (False, "empty", 0) in seen and any(s[2] == 1 for s in seen) and any(s[2] == 2 for s in seen)


def test_two_sums_back_to_back_share_the_ticket(ctx):
    """The arrival counter is left at zero for the next launch on the stream: a second and a third sum with a hand-off between workgroups
    (and another number of them) are still complete and bit-equal."""
    for n in (3907, 977, 15625, 977):
        rows = make_rows(n, 1000 + n)
        assert_bits_equal(device_sum(ctx, rows), restated_sum(rows), n)


def test_derived_columns_leave_the_summed_ones_alone(ctx):
    """derive = 1 (what a pass asks for) replaces the derived columns 0 .. 14 and 21 .. 23 by functions of the totals; every other column is
    the same sum, bit for bit."""
    rows = make_rows(3907, 99)
    got, want = device_sum(ctx, rows, 1), restated_sum(rows)
    keep = np.array([c for c in range(ROW) if not (c < 15 or 21 <= c < 24)])
    assert_bits_equal(got[keep], want[keep], "derive")


# The derived columns of a row in moment form (csrc/reduce_rows.hpp: derived_entry), restated from the layout of a row: with SYM the position
# of (j, k) in a packed symmetric 3x3, G(a, j) = m[32 + 3 a + j] (sum p_a g_j), A(a, j, k) = m[41 + 6 a + SYM[j][k]] (sum p_a M'_jk) and
# B(a, b, j, k) = m[59 + 6 SYM[a][b] + SYM[j][k]] (sum p_a p_b M'_jk):  b_r[i] = G(i2, i1) - G(i1, i2) (columns 21 .. 23),
# H_rt[i][k] = A(i1, i2, k) - A(i2, i1, k), H_rr[i][j] = PK(j1, i, j2) - PK(j2, i, j1) with PK(l, i, k) = B(l, i1, i2, k) - B(l, i2, i1, k),
# x1 = x + 1 mod 3, x2 = x + 2 mod 3; H is stored as the upper triangle of the 6x6, row by row (columns 0 .. 20, of which rows 0 .. 2 are derived).
SYM = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]


def restated_derived(m):
    def G(a, j):
        return m[32 + 3 * a + j]

    def A(a, j, k):
        return m[41 + 6 * a + SYM[j][k]]

    def B(a, b, j, k):
        return m[59 + 6 * SYM[a][b] + SYM[j][k]]

    def PK(l, i, k):
        return B(l, (i + 1) % 3, (i + 2) % 3, k) - B(l, (i + 2) % 3, (i + 1) % 3, k)

    out = m.copy()
    col = 0
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(i, 6):
            if j < 3:
                out[col] = PK((j + 1) % 3, i, (j + 2) % 3) - PK((j + 2) % 3, i, (j + 1) % 3)
            else:
                out[col] = A(i1, i2, j - 3) - A(i2, i1, j - 3)
            col += 1
        out[21 + i] = G(i2, i1) - G(i1, i2)
    assert col == 15
    return out


@pytest.mark.parametrize("nrows", [8, 977, 3907])
def test_derived_columns_are_the_documented_functions_of_the_totals(ctx, nrows):
    """derive = 1: columns 0 .. 14 and 21 .. 23 are differences of totals of the moment columns, bit for bit.  The totals are random and
    all different, and the derived columns read 42 of them through every off-diagonal and diagonal position of the packed symmetric
    matrices: a wrong position reads another total and changes bits."""
    rows = make_rows(nrows, 7000 + nrows)
    want = restated_derived(restated_sum(rows))
    assert_bits_equal(device_sum(ctx, rows, 1), want, nrows)

"""tests/kd_ref.py — the definition of the implicit balanced kd-tree that sga_index_build_kdtree builds (csrc/index_build.hip:
build_kdtree; layout in csrc/kd_search.hpp), as a checker of any tree the device hands out (KdTree._tree). Numpy only.

The tree.  D = kd_depth(n): the least depth whose leaves hold at most 8 points.  Node k of depth d (d < D, k < 2^d) owns the kd
positions [B(d, k), B(d, k + 1)) with B(d, k) = floor(k n / 2^d) (kd_bound); its children own [B(d, k), m) and [m, B(d, k + 1)) with
m = B(d + 1, 2k + 1).  The split axis is the longest fp32 extent (hi - lo, rounded to fp32) of the node's own points, ties by
v0 >= v1 ? (v0 >= v2 ? 0 : 2) : (v1 >= v2 ? 1 : 2); the threshold is the median: the axis coordinate of the point at kd position m
when the node is split (the device writes the decoded median key there), i.e. the smallest coordinate of the right half — the deeper
levels move other points of the right half to position m, so the finished tree is checked against that minimum, bit for bit; every left
coordinate is <= the threshold <= every right coordinate.  Coordinates compare as the device's keys do (ordered_from_float: -0 < +0,
else the float order).  The order inside a half is not part of the definition.

build_tree is a plain numpy builder under the same rule (a stable sort per segment); it exists so that the CPU tests can show that
check_tree accepts a correct tree."""
import numpy as np

LEAF_MAX = 8  # kKdLeafMax


def kd_depth(n):
    """The least D with ceil(n / 2^D) <= LEAF_MAX."""
    d = 0
    while (n + (1 << d) - 1) >> d > LEAF_MAX:
        d += 1
    return d


def kd_bound(n, d, k):
    """B(d, k) = floor(k n / 2^d); k may be an array."""
    return (np.asarray(k, dtype=np.int64) * int(n)) >> d


def split_axis(ext):
    """The device's tie rule over the extents (..., 3) (kd_longest_axis)."""
    v0, v1, v2 = ext[..., 0], ext[..., 1], ext[..., 2]
    return np.where(v0 >= v1, np.where(v0 >= v2, 0, 2), np.where(v1 >= v2, 1, 2)).astype(np.int32)


def ordered(c):
    """The device's order-preserving int32 encoding of float32 coordinates (index_build.hip: ordered_from_float)."""
    b = np.ascontiguousarray(c, dtype=np.float32).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def _first(bad):
    return int(np.flatnonzero(bad)[0])


def check_tree(points_kd, order, depth, thr, axis, n):
    """Assert that (points_kd (n, 3) float32 in kd order, order (n,) original indices, depth, thr (2^D,) float32, axis (2^D,) int) is the
    tree the definition above gives for its points.  Every failure names the node (d, k)."""
    pts = np.asarray(points_kd, dtype=np.float32).reshape(-1, 3)
    order = np.asarray(order, dtype=np.int64)
    thr = np.asarray(thr, dtype=np.float32)
    axis = np.asarray(axis).astype(np.int64)
    assert len(pts) == n and len(order) == n, ("sizes", len(pts), len(order), n)
    assert np.array_equal(np.sort(order), np.arange(n)), "order is not a permutation of 0..n-1"
    assert depth == kd_depth(n), ("depth", depth, kd_depth(n))
    assert len(thr) >= (1 << depth) and len(axis) >= (1 << depth), ("node arrays", len(thr), len(axis), 1 << depth)
    for d in range(depth):
        K = 1 << d
        ks = np.arange(K)
        first = kd_bound(n, d, ks)
        cb = kd_bound(n, d + 1, np.arange(2 * K))  # children: left 2k at B(d, k), right 2k + 1 at m
        mid = cb[1::2]
        assert (np.diff(np.append(cb, n)) > 0).all(), ("empty child at depth", d + 1)  # (d < D: every child holds >= 4 points)
        lo = np.minimum.reduceat(pts, first, axis=0)
        hi = np.maximum.reduceat(pts, first, axis=0)
        want = split_axis(hi - lo)  # float32 arithmetic, like the device
        got = axis[K + ks]
        bad = got != want
        assert not bad.any(), ("axis", (d, _first(bad)), int(got[_first(bad)]), int(want[_first(bad)]), (hi - lo)[_first(bad)])
        t = ordered(thr[K + ks])
        seg = np.repeat(ks, np.diff(np.append(first, n)))
        c = ordered(pts[np.arange(n), want[seg]])  # every point's coordinate along its node's axis
        left_max = np.maximum.reduceat(c, cb)[0::2]
        right_min = np.minimum.reduceat(c, cb)[1::2]
        bad = left_max > t
        assert not bad.any(), ("left side above the threshold", (d, _first(bad)), int(left_max[_first(bad)]), int(t[_first(bad)]))
        bad = right_min != t
        assert not bad.any(), ("threshold is not the median (the right side's minimum)", (d, _first(bad)), int(t[_first(bad)]), int(right_min[_first(bad)]))


def build_tree(points):
    """(points_kd, order, depth, thr, axis): a valid tree over points (n, 3) float32 — every node's points stably sorted along its axis
    (by the device's key order)."""
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(pts)
    D = kd_depth(n)
    thr = np.zeros(1 << D, np.float32)
    axis = np.zeros(1 << D, np.int32)
    order = np.arange(n, dtype=np.int64)
    for d in range(D):
        K = 1 << d
        ks = np.arange(K)
        first = kd_bound(n, d, ks)
        cur = pts[order]
        ext = np.maximum.reduceat(cur, first, axis=0) - np.minimum.reduceat(cur, first, axis=0)
        ax = split_axis(ext)
        seg = np.repeat(ks, np.diff(np.append(first, n)))
        c = ordered(cur[np.arange(n), ax[seg]])
        perm = np.lexsort((c, seg))  # stable: by segment, then coordinate, then current position
        order = order[perm]
        mid = kd_bound(n, d + 1, 2 * ks + 1)
        thr[K + ks] = pts[order[mid], ax]
        axis[K + ks] = ax
    return pts[order], order, D, thr, axis

"""CPU tests of tests/kd_ref.py: check_tree accepts the trees build_tree makes under the kd-tree's definition, on every kind of cloud the
GPU tests build trees over, and rejects each kind of defect it exists to find.  No GPU."""
import numpy as np
import pytest

from kd_ref import build_tree, check_tree, kd_bound, kd_depth

SIZES = list(range(1, 10)) + [255, 256, 257, 40_000]


def cloud(kind, n, rng):
    if kind == "random":
        return rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    if kind == "duplicates":
        return rng.integers(0, 3, (n, 3)).astype(np.float32)[rng.integers(0, max(1, n // 4), n) % n]
    if kind == "lattice":
        g = np.arange(8, dtype=np.float32)
        lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
        return lat[np.arange(n) % len(lat)]
    if kind == "line":
        return np.c_[rng.uniform(-100, 100, n), np.zeros(n), np.zeros(n)].astype(np.float32)
    if kind == "single point":
        return np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (n, 1))
    raise ValueError(kind)


KINDS = ["random", "duplicates", "lattice", "line", "single point"]


def test_depth_and_bounds():
    assert [kd_depth(n) for n in (0, 1, 8, 9, 16, 17, 256, 257, 1_000_000)] == [0, 0, 0, 1, 1, 2, 5, 6, 17]
    assert list(kd_bound(10, 2, np.arange(5))) == [0, 2, 5, 7, 10]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_checker_accepts_a_valid_tree(kind, n):
    pts = cloud(kind, n, np.random.default_rng(n))
    tree = build_tree(pts)
    assert np.array_equal(tree[0], pts[tree[1]])
    check_tree(*tree, n)


def _random_tree(n=4096, seed=5):
    pts = cloud("random", n, np.random.default_rng(seed))
    pk, order, D, thr, axis = build_tree(pts)
    check_tree(pk, order, D, thr, axis, n)
    return pk.copy(), order.copy(), D, thr.copy(), axis.copy(), n


def test_checker_rejects_two_points_swapped_across_a_split():
    pk, order, D, thr, axis, n = _random_tree()
    d, k = 3, 5
    first, end, mid = kd_bound(n, d, k), kd_bound(n, d, k + 1), kd_bound(n, d + 1, 2 * k + 1)
    a = axis[(1 << d) + k]
    i = first + int(np.argmin(pk[first:mid, a]))  # far below the threshold, on the left
    j = mid + 1 + int(np.argmax(pk[mid + 1 : end, a]))  # far above it, on the right (not the point at m, which gives the threshold)
    pk[[i, j]] = pk[[j, i]]
    order[[i, j]] = order[[j, i]]
    with pytest.raises(AssertionError, match=r"left side above the threshold.*\(3, 5\)"):
        check_tree(pk, order, D, thr, axis, n)


def test_checker_rejects_a_changed_axis():
    pk, order, D, thr, axis, n = _random_tree()
    axis[(1 << 4) + 9] = (axis[(1 << 4) + 9] + 1) % 3
    with pytest.raises(AssertionError, match=r"axis.*\(4, 9\)"):
        check_tree(pk, order, D, thr, axis, n)


def test_checker_rejects_a_threshold_one_ulp_off():
    pk, order, D, thr, axis, n = _random_tree()
    thr[(1 << 6) + 17] = np.nextafter(thr[(1 << 6) + 17], np.float32(np.inf))
    with pytest.raises(AssertionError, match=r"median.*\(6, 17\)"):
        check_tree(pk, order, D, thr, axis, n)


def test_checker_rejects_a_duplicated_index():
    pk, order, D, thr, axis, n = _random_tree()
    order[7] = order[8]
    with pytest.raises(AssertionError, match="permutation"):
        check_tree(pk, order, D, thr, axis, n)


def test_checker_rejects_a_depth_one_too_small():
    pk, order, D, thr, axis, n = _random_tree()
    with pytest.raises(AssertionError, match="depth"):
        check_tree(pk, order, D - 1, thr, axis, n)

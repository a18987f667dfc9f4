"""Hand cases for the restatement itself (tests/cluster_ref.py): the rule of DESIGN.md section 3.26 on inputs whose answer is known
without a computer.  No device, no library."""
import numpy as np

from cluster_ref import cluster, neighbours


def pts(*rows):
    return np.array(rows, np.float32)


def test_two_points_at_exactly_eps_are_neighbours_and_in_the_band():
    r = cluster(pts([0, 0, 0], [0.5, 0, 0]), 0.5)  # 0.5 and 0.25 are exactly representable: d2 == eps^2, and <= holds
    assert r["labels"].tolist() == [0, 0] and r["num_clusters"] == 1 and r["sizes"].tolist() == [2] and r["seeds"].tolist() == [0]
    assert r["band"]["pairs"] == 1
    lists, band = neighbours(pts([0, 0, 0], [0.5, 0, 0]), np.array([[0.0, 0, 0]]), 0.5)
    assert lists[0][0].tolist() == [0, 1] and lists[0][1].tolist() == [0.0, 0.25] and band == 1
    r = cluster(pts([0, 0, 0], [0.5, 0, 0]), 0.4999)
    assert r["labels"].tolist() == [0, 1] and r["band"] == {"pairs": 0, "points": 0, "ties": 0}


def test_a_chain_is_one_cluster_whatever_the_order_of_its_indices():
    x = np.arange(10) * 0.9
    order = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    p = np.zeros((10, 3), np.float32)
    p[:, 0] = x[order]
    r = cluster(p, 1.0)
    assert r["labels"].tolist() == [0] * 10 and r["seeds"].tolist() == [0] and r["sizes"].tolist() == [10]
    assert np.array_equal(r["boxes"][0], [[0, 0, 0], [np.float32(8.1), 0, 0]])
    q = p.copy()
    q[order.index(5), 0] = 100.0  # the chain is cut: 0 .. 4 and 6 .. 9 and the far point
    r = cluster(q, 1.0)
    assert r["num_clusters"] == 3 and sorted(r["sizes"].tolist()) == [1, 4, 5]
    assert r["seeds"].tolist() == sorted(r["seeds"].tolist())


def test_a_border_point_joins_its_nearest_core_point_and_a_tie_goes_to_the_lower_index():
    # two groups of four core points (min_points 4, eps 0.9; every coordinate exactly representable) and a point between them that has
    # three records within eps — itself, x = 0.75 (index 3) and x = 2.25 (index 7) — and is nearer to the right group
    left = [[0, 0, 0], [0.25, 0, 0], [0.5, 0, 0], [0.75, 0, 0]]
    right = [[3.0, 0, 0], [2.5, 0, 0], [2.75, 0, 0], [2.25, 0, 0]]
    r = cluster(pts(*left, *right, [1.5625, 0, 0]), 0.9, min_points=4)
    assert r["core"].tolist() == [True] * 8 + [False]
    assert r["labels"].tolist() == [0] * 4 + [1] * 4 + [1] and r["sizes"].tolist() == [4, 5] and r["band"] == {"pairs": 0, "points": 0, "ties": 0}
    # exactly in the middle between index 3 and index 7: the lower index wins, and the tie is reported
    mid = cluster(pts(*left, *right, [1.5, 0, 0]), 0.9, min_points=4)
    assert mid["core"].tolist() == [True] * 8 + [False]
    assert mid["labels"].tolist() == [0] * 4 + [1] * 4 + [0] and mid["band"]["ties"] == 1 and mid["sizes"].tolist() == [5, 4]
    # no core point within eps: noise
    far = cluster(pts(*left, *right, [1.5625, 5, 0]), 0.9, min_points=4)
    assert far["labels"].tolist() == [0] * 4 + [1] * 4 + [-1] and far["noise"] == 1 and far["dropped"] == 0


def test_min_points_larger_than_any_neighbourhood_is_all_noise():
    p = np.random.default_rng(1).normal(size=(40, 3)).astype(np.float32)
    r = cluster(p, 0.5, min_points=41)
    assert (r["labels"] == -1).all() and r["num_clusters"] == 0 and r["noise"] == 40 and r["dropped"] == 0 and r["boxes"].shape == (0, 2, 3)


def test_max_size_drops_the_big_cluster_and_the_rest_is_renumbered():
    big = [[0.1 * k, 0, 0] for k in range(6)]
    small = [[10, 0, 0], [10.1, 0, 0]]
    lone = [[20, 0, 0]]
    r = cluster(pts(*lone, *big, *small), 0.2)
    assert r["labels"].tolist() == [0] + [1] * 6 + [2] * 2 and r["seeds"].tolist() == [0, 1, 7]
    r = cluster(pts(*lone, *big, *small), 0.2, max_size=5)
    assert r["labels"].tolist() == [0] + [-1] * 6 + [1] * 2 and r["seeds"].tolist() == [0, 7] and r["dropped"] == 6 and r["noise"] == 0
    r = cluster(pts(*lone, *big, *small), 0.2, min_size=2, max_size=5)
    assert r["labels"].tolist() == [-1] * 7 + [0] * 2 and r["dropped"] == 7 and r["num_clusters"] == 1
    assert np.array_equal(r["boxes"][0], np.array([[10, 0, 0], [np.float32(10.1), 0, 0]], np.float64))


def test_duplicates_count_as_records_and_share_a_cluster():
    p = pts([1, 1, 1], [1, 1, 1], [1, 1, 1], [5, 5, 5])
    r = cluster(p, 0.1, min_points=3)
    assert r["core"].tolist() == [True, True, True, False] and r["labels"].tolist() == [0, 0, 0, -1] and r["noise"] == 1
    r = cluster(p, 0.1, origin=(128.0, 0.0, -256.0))
    assert r["labels"].tolist() == [0, 0, 0, 1] and np.array_equal(r["boxes"][0], [[129, 1, -255], [129, 1, -255]])

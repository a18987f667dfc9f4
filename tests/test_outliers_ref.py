"""tests/outliers_ref.py — the fp64 restatement that tests/test_cloud_outliers_gpu.py compares the device against — on cases that can
be checked by hand, and the edge rules of the definitions (small n, n <= k, radius mode with n <= k).  No device is needed."""
import numpy as np

import outliers_ref as ref

INF = float("inf")


def line(xs):
    return np.array([[x, 0.0, 0.0] for x in xs], dtype=np.float32)


def test_five_collinear_points_statistical():
    # x = 0, 1, 2, 3, 10 with k = 2: the two nearest OTHER records of each point are at (1,2) (1,1) (1,1) (1,2) (7,8)
    r = ref.restate(line([0, 1, 2, 3, 10]), k=2, std_mul=1.0)
    assert np.array_equal(r["stat"], [1.5, 1.0, 1.0, 1.5, 7.5])
    assert r["mean"] == 2.5
    assert r["stddev"] == np.sqrt((1.0 + 2.25 + 2.25 + 1.0 + 25.0) / 4)
    assert r["threshold"] == 2.5 + r["stddev"]
    assert np.array_equal(r["kept"], [0, 1, 2, 3]) and r["kept"].dtype == np.int64
    # std_mul = 0: the threshold is the mean, and "<=" keeps a point that sits on it
    r0 = ref.restate(line([0, 1, 2, 3, 10]), k=2, std_mul=0.0)
    assert r0["threshold"] == 2.5 and np.array_equal(r0["kept"], [0, 1, 2, 3])
    eq = ref.restate(line([0, 1, 2, 3]), k=1, std_mul=0.0)  # every d_i = 1 = mean
    assert np.array_equal(eq["stat"], [1, 1, 1, 1]) and eq["stddev"] == 0.0 and len(eq["kept"]) == 4


def test_five_collinear_points_radius():
    r = ref.restate(line([0, 1, 2, 3, 10]), k=2, radius=2.0)
    assert np.array_equal(r["stat"], [2.0, 1.0, 1.0, 2.0, 8.0])  # s_i(2)
    assert r["threshold"] == 2.0 and np.array_equal(r["kept"], [0, 1, 2, 3])  # closed: s_i(k) == radius keeps
    assert r["mean"] == 14.0 / 5
    r = ref.restate(line([0, 1, 2, 3, 10]), k=1, radius=0.5)
    assert len(r["kept"]) == 0


def test_ties_do_not_matter():
    # four corners of a unit square: every point has two neighbours at 1 and one at sqrt 2, whichever comes "first"
    sq = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], dtype=np.float32)
    r = ref.restate(sq, k=2)
    assert np.array_equal(r["stat"], [1.0] * 4) and len(r["kept"]) == 4
    dup = np.array([[0, 0, 0], [0, 0, 0], [3, 0, 0]], dtype=np.float32)  # a duplicate is a neighbour at distance 0
    assert np.array_equal(ref.restate(dup, k=1)["stat"], [0.0, 0.0, 3.0])


def test_one_point():
    r = ref.restate(line([4]), k=10)
    assert np.array_equal(r["stat"], [0.0]) and r["mean"] == 0.0 and r["stddev"] == 0.0 and r["threshold"] == 0.0
    assert np.array_equal(r["kept"], [0])


def test_two_points():
    r = ref.restate(line([0, 3]), k=10, std_mul=1.0)  # k' = 1
    assert np.array_equal(r["stat"], [3.0, 3.0]) and r["mean"] == 3.0 and r["stddev"] == 0.0
    assert np.array_equal(r["kept"], [0, 1])


def test_fewer_points_than_k_average_over_what_there_is():
    r = ref.restate(line([0, 1, 3]), k=5)  # k' = 2
    assert np.array_equal(r["stat"], [2.0, 1.5, 2.5])
    full = ref.restate(line([0, 1, 3]), k=2)  # n = k + 1: the same
    assert np.array_equal(full["stat"], r["stat"])


def test_radius_mode_with_no_more_points_than_k_removes_everything():
    for n in (1, 2, 3):
        r = ref.restate(line(range(n)), k=3, radius=100.0)
        assert np.all(r["stat"] == INF) and len(r["kept"]) == 0 and r["threshold"] == 100.0
        assert r["mean"] == INF
    r = ref.restate(line(range(4)), k=3, radius=100.0)  # n = k + 1: every point has its three
    assert np.array_equal(r["stat"], [3.0, 2.0, 2.0, 3.0]) and len(r["kept"]) == 4


def test_empty_cloud():
    r = ref.restate(np.zeros((0, 3), np.float32), k=10)
    assert len(r["stat"]) == 0 and len(r["kept"]) == 0 and r["mean"] == 0.0 and r["threshold"] == 0.0


def test_band_and_the_test_clouds():
    r = ref.restate(line([0, 1, 2, 3, 10]), k=2, std_mul=0.0)
    assert len(ref.band(r)) == 0
    r["threshold"] = 1.5 * (1 + 0.5e-5)
    assert np.array_equal(ref.band(r), [0, 3])
    pts = ref.planes_with_scatter(1)
    assert pts.shape == (3000, 3) and pts.dtype == np.float32
    assert pts.tobytes() == ref.planes_with_scatter(1).tobytes() and pts.tobytes() != ref.planes_with_scatter(2).tobytes()
    assert ref.planes_with_scatter(3, 340, 50).shape == (730, 3) and ref.planes_with_scatter(4, 2000, 0).shape == (4000, 3)

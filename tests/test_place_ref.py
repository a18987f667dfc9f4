"""Hand cases for the restatement of the place recognition (tests/place_ref.py) — the yardstick of
tests/test_places_gpu.py must itself be right: the descriptor's cells, limits and skipped records, the distance of turned copies, of
images with empty columns and of empty images, the order of a query's result, and the band."""
import numpy as np
import pytest

import place_ref as ref

F32 = np.float32


def polar(rho, theta, z):
    return [rho * np.cos(theta), rho * np.sin(theta), z]


def test_one_point_per_cell():
    R, S, L = 3, 8, 30.0
    pts, want = [], np.zeros((R, S), F32)
    for r in range(R):
        for s in range(S):
            z = 0.25 * (1 + r * S + s)
            pts.append(polar((r + 0.5) * L / R, (s + 0.5) * 2 * np.pi / S, z))
            want[r, s] = F32(np.float64(F32(pts[-1][2])) + 1.5)
    rec = np.array(pts, F32)
    D, band = ref.descriptor(rec, R=R, S=S, L=L, height=1.5, return_band=True)
    assert D.dtype == F32 and D.shape == (R, S)
    assert np.array_equal(D, want) and not band.any()
    # the greatest value of a cell wins, whatever the order; a lower point changes nothing
    more = np.concatenate([rec, rec - F32([0, 0, 0.125])])
    assert np.array_equal(ref.descriptor(more[::-1], R=R, S=S, L=L, height=1.5), want)


def test_center_origin_and_the_centre_point():
    # a point at the sensor's own position: rho = 0, atan2(0, 0) = 0 -> cell (0, 0)
    D = ref.descriptor(np.array([[0, 0, 1.0]], F32), R=4, S=6, L=10.0, height=2.0)
    assert D[0, 0] == 3.0 and np.count_nonzero(D) == 1
    # the same through a centre and an origin: p = (record + origin) - center
    D = ref.descriptor(np.array([[1.0, -2.0, 0.5]], F32), origin=[128.0, 256.0, 0.0], center=[129.0, 254.0, -0.5], R=4, S=6, L=10.0, height=2.0)
    assert D[0, 0] == 3.0 and np.count_nonzero(D) == 1
    # a point on the negative y axis: theta = 3 pi / 2 -> sector floor(0.75 S)
    D = ref.descriptor(np.array([[0, -4.0, 0]], F32), R=4, S=8, L=10.0, height=1.0)
    assert D[1, 6] == 1.0 and np.count_nonzero(D) == 1


def test_range_limit_and_skipped_records():
    R, S, L = 5, 4, 10.0
    rec = np.array([[10.0, 0, 5.0], [0, 12.0, 5.0], [np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [9.999, 0, 1.0]], F32)
    D = ref.descriptor(rec, R=R, S=S, L=L, height=0.0)
    assert D[R - 1, 0] == 1.0 and np.count_nonzero(D) == 1  # exactly L and beyond: skipped; non-finite: skipped
    # the record at exactly L is a band point: its cell is a band cell
    band = ref.band_cells(rec, R=R, S=S, L=L, height=0.0)
    assert band[R - 1, 0] and band[R - 1, S - 1]  # (theta = 0 is on a sector boundary as well: sectors 0 and S - 1)
    assert not band[: R - 1].any()
    assert np.array_equal(ref.descriptor(np.zeros((0, 3), F32), R=R, S=S, L=L), np.zeros((R, S), F32))
    assert np.array_equal(ref.descriptor(rec[:5], R=R, S=S, L=L), np.zeros((R, S), F32))


def test_negative_heights_are_zero():
    rec = np.array([[1.0, 1.0, -3.0], [-1.0, 1.0, -2.0], [-1.0, -1.0, -1.5], [1.0, -1.0, 0.0]], F32)
    D = ref.descriptor(rec, R=1, S=4, L=5.0, height=2.0)
    assert np.array_equal(D, F32([[0.0, 0.0, 0.5, 2.0]])) and not np.signbit(D).any()
    # pz + height == 0 exactly: a band point, its cell a band cell, its value 0
    band = ref.band_cells(rec, R=1, S=4, L=5.0, height=2.0)
    assert np.array_equal(band, [[False, True, False, False]])


def test_band_marks_ring_and_sector_boundaries():
    R, S, L = 4, 8, 8.0
    inside = np.array([polar(3.0, 0.4, 1.0), polar(5.0, 2.0, 1.0)], F32)
    assert not ref.band_cells(inside, R=R, S=S, L=L).any()
    on_ring = np.array([[2.0, 0.0, 1.0]], F32)  # rho / L * R = 1 exactly, theta = 0 exactly
    band = ref.band_cells(on_ring, R=R, S=S, L=L)
    assert set(map(tuple, np.argwhere(band))) == {(0, 0), (1, 0), (0, S - 1), (1, S - 1)}
    on_sector = np.array([[0.0, 3.0, 1.0]], F32)  # theta = pi / 2: sector boundary 2 of 8
    band = ref.band_cells(on_sector, R=R, S=S, L=L)
    assert set(map(tuple, np.argwhere(band))) == {(1, 1), (1, 2)}


def random_image(rng, R, S, empty_columns=()):
    img = rng.uniform(0.0, 5.0, (R, S)).astype(F32)
    img[rng.uniform(size=(R, S)) < 0.3] = 0.0
    img[:, list(empty_columns)] = 0.0
    if not img.any():
        img[0, S - 1] = 1.0
    return img


@pytest.mark.parametrize("R, S", [(1, 1), (3, 7), (20, 60), (16, 256)])
def test_a_turned_copy_has_distance_zero_at_its_shift(R, S):
    rng = np.random.default_rng(R * 1000 + S)
    img = random_image(rng, R, S)
    for shift in sorted({0, 1, S // 2, S - 1}):
        d, s = ref.distance(ref.turned(img, shift), img)
        assert abs(d) <= ref.DISTANCE_TOL and (s == shift or S == 1)
    assert ref.expected_shift(np.deg2rad(150.0), 60) == 25 and ref.expected_shift(np.deg2rad(-75.0), 60) == 47 and ref.expected_shift(np.deg2rad(180.0), 60) == 30


def test_distance_by_hand():
    # two columns, one ring: q = [3, 4], c = [4, 3] -> every column pair has cosine 1: d = 0 at shift 0 already
    assert ref.distance(F32([[3, 4]]), F32([[4, 3]])) == (0.0, 0)
    # two rings: q columns (1, 0) and (0, 1); c columns (0, 2) and (2, 0): shift 0 pairs orthogonal columns (d = 1), shift 1 parallel ones (d = 0)
    q, c = F32([[1, 0], [0, 1]]), F32([[0, 2], [2, 0]])
    assert np.array_equal(ref.shift_distances(q, c), [[1.0, 0.0]])
    assert ref.distance(q, c) == (0.0, 1)
    # cos = 0.6 and 0.8 at shift 0
    q, c = F32([[1, 1], [0, 0]]), F32([[3, 4], [4, 3]])
    np.testing.assert_allclose(ref.shift_distances(q, c), [[1 - 0.7, 1 - 0.7]], rtol=0, atol=1e-15)
    assert ref.distance(q, c)[1] == 0  # a tie goes to the lowest shift


def test_empty_columns_do_not_count():
    # q has an empty column 1: only column 0 counts.  c = [[2, 0, 5]]: shift 0 pairs q0 with c0 (cos 1) -> d = 0
    q, c = F32([[1, 0, 0]]), F32([[2, 0, 5]])
    ds = ref.shift_distances(q, c)[0]
    assert np.array_equal(ds, [0.0, 1.0, 0.0])  # shift 1 pairs q0 with the empty c1: count 0 -> 1
    assert ref.distance(q, c) == (0.0, 0)
    rng = np.random.default_rng(5)
    img = random_image(rng, 6, 12, empty_columns=(0, 5, 6))
    d, s = ref.distance(ref.turned(img, 4), img)
    assert abs(d) <= ref.DISTANCE_TOL and s == 4
    assert np.array_equal(ref.column_norms(img)[[0, 5, 6]], [0, 0, 0])


def test_all_empty_images():
    z = np.zeros((4, 9), F32)
    img = random_image(np.random.default_rng(1), 4, 9)
    assert ref.distance(z, img) == (1.0, 0) and ref.distance(img, z) == (1.0, 0) and ref.distance(z, z) == (1.0, 0)
    r = ref.query(z, np.stack([img, z, img]), k=5)
    assert r["index"].tolist() == [0, 1, 2] and r["shift"].tolist() == [0, 0, 0] and r["distance"].tolist() == [1.0, 1.0, 1.0]
    assert r["order_band"].tolist() == [True, True, False]  # equal distances: the index decides, and the restatement says so


def test_query_order_and_range():
    rng = np.random.default_rng(9)
    R, S = 5, 16
    entries = np.stack([random_image(rng, R, S) for _ in range(12)])
    q = ref.turned(entries[7], 3)
    r = ref.query(q, entries, k=4)
    assert r["index"][0] == 7 and r["shift"][0] == 3 and abs(r["distance"][0]) <= ref.DISTANCE_TOL
    assert (np.diff(r["distance"]) >= 0).all() and len(r["index"]) == 4
    d, s, _ = ref.best_shifts(q, entries)
    assert np.array_equal(r["all_distance"], d) and np.array_equal(r["all_shift"], s)
    assert np.array_equal(r["index"], np.lexsort((np.arange(12), d))[:4])
    sub = ref.query(q, entries, first=8, count=3, k=32)
    assert sorted(sub["index"].tolist()) == [8, 9, 10] and np.array_equal(sub["distance"], np.sort(d[8:11]))
    assert len(ref.query(q, entries, first=12, count=0, k=3)["index"]) == 0
    # two equal entries: the lower index first, flagged as a decision in band
    twins = np.stack([entries[2], entries[7], entries[7]])
    r = ref.query(q, twins, k=2)
    assert r["index"].tolist() == [1, 2] and r["distance"][0] == r["distance"][1] and r["order_band"][0]

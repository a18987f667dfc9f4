"""Place recognition on the device (csrc/places.hip) against the float64 restatement of tests/place_ref.py,
which never goes through the library.

The comparison rule.  The restatement marks its band (place_ref.py says how): the cells a record within 1e-9 of a ring or sector
boundary, or within 1e-12 of height 0, could enter or leave, and the decisions (the best shift of an entry, the order of two
neighbours of the ranking) whose two restated distances lie closer than 2e-12.  Every case first asserts ON THE RESTATEMENT that the
band holds at most 1 % of the cells and of the decisions (if it ever fails: another seed, never a looser comparison).  Outside the band:
  descriptor   every cell bit-exact.
  query        every distance within 1e-12 of the restatement: the products of fp32 values are exact in double, what remains is at most
               R + S + 8 roundings of 2^-53 on terms at most 1, about 4e-14 at (16, 256); 1e-12 leaves 25 x over that.  Indices and
               shifts equal.  Greatest deviation measured on the MI355X: see DESIGN.md section 3.25.
The cases planted on purpose inside the band (points at the centre, equal entries, identical columns, empty queries) are asserted
directly against what the rule says about them."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import place_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import _lib, api, odometry, synthetic
from conftest import ROOT
from test_cloud_merge_gpu import records, upload_relative

pytestmark = pytest.mark.gpu

F32 = np.float32
U32 = np.uint32
ZERO = np.zeros(3)
DEFAULT = dict(R=20, S=60, L=80.0, height=2.0)
SHAPES = [(1, 1), (3, 7), (20, 60), (64, 64), (16, 256)]
SIZES = [0, 1, 2, 63, 64, 65, 300]
DEVIATION = {"max": 0.0}  # the greatest |device - restatement| of a distance seen in this run (printed by the tests that add to it)


def cloud_points(n, seed, L=80.0):
    """n records scattered over a disc of 1.2 L (so that some lie beyond the range), heights from 4 m below to 6 m above the sensor"""
    rng = np.random.default_rng(seed)
    rho, th = 1.2 * L * np.sqrt(rng.uniform(size=n)), rng.uniform(-np.pi, np.pi, n)
    p = np.stack([rho * np.cos(th), rho * np.sin(th), rng.uniform(-4.0, 6.0, n)], axis=1).astype(F32)
    p.setflags(write=False)
    return p


def device_descriptor(rec, origin=ZERO, center=None, R=20, S=60, L=80.0, height=2.0):
    return upload_relative(rec, None, None, origin).scan_context(R, S, L, height, center)


def check_descriptor(got, rec, origin=ZERO, center=None, what="", **g):
    g = {**DEFAULT, **g}
    want, band = ref.descriptor(rec, origin, center, return_band=True, **g)
    assert band.sum() <= 0.01 * band.size, "%s: %d of %d cells in band" % (what, band.sum(), band.size)  # the cap, on the restatement alone
    assert got.dtype == F32 and got.shape == want.shape
    bad = (got.view(U32) != want.view(U32)) & ~band
    print("%s: %d records, %d non-zero cells, %d band cells, %d cells differ" % (what, len(rec), np.count_nonzero(want), band.sum(), bad.sum()))
    assert not bad.any(), (what, np.argwhere(bad)[:5], got[bad][:5], want[bad][:5])
    return want, band


# ---- the descriptor -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_descriptor_sizes(n):
    """(a workgroup takes 2048 records: 2047 / 2048 / 2049 stand on both sides of the second workgroup, 5000 takes three)"""
    rec = cloud_points(n, 10 + n)
    got = device_descriptor(rec)
    want, _ = check_descriptor(got, rec, what="n = %d" % n)
    assert n == 0 or n == 1 or np.count_nonzero(want) > 0
    if n == 0:
        assert not got.view(U32).any()


@functools.lru_cache(maxsize=None)
def scan(frame=12, n_az=600):
    p = synthetic.scan_at(synthetic._sensor_pose(frame), n_az=n_az)
    p.setflags(write=False)
    return p


def test_descriptor_of_a_scan():
    """A scan in the world frame with the sensor's position as the centre, as a mapping loop holds its keyframes.  (In its own sensor
    frame the generator's rays at azimuth 0, +-pi / 2 and pi run along sector boundaries: 78 of the 1200 cells are band cells there.)"""
    T = synthetic._sensor_pose(12)
    world = (scan().astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F32)
    cloud = sga.PointCloud(world)
    rec, _ = records(cloud)
    want, _ = check_descriptor(cloud.scan_context(center=T[:3, 3]), rec, cloud.origin(), T[:3, 3], what="scan_at")
    assert np.count_nonzero(want) > 300


@pytest.mark.parametrize("R, S", SHAPES)
def test_descriptor_shapes(R, S):
    rec = cloud_points(5000, 100 * R + S, L=30.0)
    check_descriptor(device_descriptor(rec, R=R, S=S, L=30.0, height=1.0), rec, what="(%d, %d)" % (R, S), R=R, S=S, L=30.0, height=1.0)


def test_descriptor_edge_records():
    rng = np.random.default_rng(3)
    # all points beyond L: an all-zero image
    far = cloud_points(3000, 4)
    far = far[np.hypot(far[:, 0].astype(np.float64), far[:, 1].astype(np.float64)) > 80.001]
    assert len(far) > 500
    got = device_descriptor(far)
    check_descriptor(got, far, what="beyond L")
    assert not got.view(U32).any()
    # NaN and inf records are skipped
    rec = cloud_points(4000, 5).copy()
    bad = rng.choice(4000, 400, replace=False)
    rec[bad[:100], 0], rec[bad[100:200], 1], rec[bad[200:300], 2], rec[bad[300:], rng.integers(0, 3, 100)] = np.nan, np.inf, -np.inf, np.nan
    want, _ = check_descriptor(device_descriptor(rec), rec, what="NaN and inf records")
    assert np.array_equal(want, ref.descriptor(np.delete(rec, bad, axis=0)))
    # points at the centre: atan2(0, 0) = 0, so cell (0, 0) — a band cell of the restatement (theta = 0 is a sector boundary), asserted by hand
    rec = np.concatenate([cloud_points(500, 6), F32([[0, 0, 1.5], [0, 0, -1.0], [0, 0, 7.25]])])
    got = device_descriptor(rec)
    _, band = check_descriptor(got, rec, what="centre points")
    assert band[0, 0] and got[0, 0] == F32(9.25)
    # negative heights: zero, never -0
    low = cloud_points(2000, 7).copy()
    low[:, 2] = -np.abs(low[:, 2]) - 2.0
    got = device_descriptor(low)
    check_descriptor(got, low, what="below the floor")
    assert not got.view(U32).any()


def test_descriptor_center_and_far_origin():
    rec = cloud_points(5000, 8)
    center = np.array([3.25, -7.5, 0.75])
    a, _ = check_descriptor(device_descriptor(rec, center=center), rec, center=center, what="center")
    assert not np.array_equal(a, ref.descriptor(rec))
    # an origin 256 km away, the centre beside it: (record + origin) - center in double
    origin = np.array([256000.0, -128000.0, 512.0])
    c = origin + [1.5, 2.5, -0.25]
    b, _ = check_descriptor(device_descriptor(rec, origin=origin, center=c), rec, origin=origin, center=c, what="origin 256 km away")
    assert np.count_nonzero(b) > 500
    # NULL center with a far origin: everything is beyond the range
    assert not device_descriptor(rec, origin=origin).view(U32).any()


def test_scan_context_and_add_download_give_the_same_bytes():
    for R, S in ((20, 60), (3, 7)):
        db = sga.PlaceDatabase(rings=R, sectors=S, max_range=50.0, height=1.0)
        clouds = [upload_relative(cloud_points(n, 20 + n), None, None, ZERO) for n in (0, 1, 700, 5000)]
        center = [1.0, -2.0, 0.5]
        for i, c in enumerate(clouds):
            assert db.add(c, center) == i
        images = db.descriptors()
        assert images.shape == (4, R, S) and len(db) == 4
        for i, c in enumerate(clouds):
            assert np.array_equal(images[i].view(U32), c.scan_context(R, S, 50.0, 1.0, center).view(U32))
        assert np.array_equal(db.descriptors(1, 2), images[1:3]) and db.descriptors(4, 0).shape == (0, R, S)


# ---- the database -------------------------------------------------------------------------------------------------------------------------
def random_image(rng, R, S):
    img = rng.uniform(0.0, 5.0, (R, S)).astype(F32)
    img[rng.uniform(size=(R, S)) < 0.3] = 0.0
    if not img.any():
        img[0, 0] = 1.0
    return img


@functools.lru_cache(maxsize=None)
def pool(R=20, S=60, n=300, seed=42):
    """n random images; every seventh has three empty columns"""
    rng = np.random.default_rng(seed)
    imgs = np.stack([random_image(rng, R, S) for _ in range(n)])
    for i in range(0, n, 7):
        imgs[i][:, rng.choice(S, min(3, S - 1), replace=False)] = 0.0
    imgs.setflags(write=False)
    return imgs


@functools.lru_cache(maxsize=None)
def database(N, R=20, S=60):
    db = sga.PlaceDatabase(rings=R, sectors=S)
    for i in range(N):
        assert db.add_descriptor(pool(R, S)[i]) == i
    return db


@pytest.mark.parametrize("N", SIZES)
def test_database_sizes_and_round_trip(N):
    db = database(N)
    assert len(db) == N
    got = db.descriptors()
    assert got.shape == (N, 20, 60) and np.array_equal(got.view(U32), pool()[:N].view(U32))


def test_entries_survive_growth_bytewise():
    db = sga.PlaceDatabase()
    clouds = [upload_relative(cloud_points(800, 300 + i), None, None, ZERO) for i in range(3)]
    before_launches = api.places_add_launches()
    for i in range(64):  # the initial capacity: no copy so far
        db.add(clouds[i % 3]) if i % 2 else db.add_descriptor(pool()[i])
    assert api.places_add_launches() - before_launches == 32 * 3 + 32 * 1
    before = db.descriptors()
    q = ref.turned(before[40], 9)
    r0 = db.query(q, k=5, return_all=True)
    assert db.add(clouds[0]) == 64  # grows: one device-to-device copy more
    assert api.places_add_launches() - before_launches == 32 * 3 + 32 * 1 + 4
    for i in range(65, 130):  # and again at 128
        db.add_descriptor(pool()[i])
    after = db.descriptors()
    assert len(db) == 130 and np.array_equal(after[:64].view(U32), before.view(U32))
    assert np.array_equal(after[64].view(U32), before[3].view(U32)) and np.array_equal(after[65:], pool()[65:130])  # (entry 3 was clouds[0] as well)
    # the norms kept beside the entries came along: the same query over the old entries gives the same bytes
    r1 = db.query(q, k=5, first=0, count=64, return_all=True)
    for key in ("index", "shift", "distance", "all_distance", "all_shift"):
        assert r0[key].tobytes() == r1[key].tobytes(), key
    assert r1["index"][0] == 40 and r1["shift"][0] == 9


# ---- queries ------------------------------------------------------------------------------------------------------------------------------
def check_query(got, want, what=""):
    """the device's result against the restatement's, outside the decisions in band (at most 1 % of them, asserted first)"""
    n_dec = len(want["all_shift_band"]) + len(want["order_band"])
    n_band = int(want["all_shift_band"].sum() + want["order_band"].sum())
    assert n_band <= 0.01 * n_dec, "%s: %d of %d decisions in band" % (what, n_band, n_dec)
    m = len(want["index"])
    assert len(got["index"]) == m and len(got["shift"]) == m and len(got["distance"]) == m
    if "all_distance" in got:
        dev = np.abs(got["all_distance"] - want["all_distance"])
        DEVIATION["max"] = max(DEVIATION["max"], float(dev.max()) if len(dev) else 0.0)
        assert (dev <= ref.DISTANCE_TOL).all(), (what, dev.max())
        ok = ~want["all_shift_band"]
        assert np.array_equal(got["all_shift"][ok], want["all_shift"][ok]), what
    if m == 0:
        return
    settled = ~want["order_band"] & ~np.concatenate([[False], want["order_band"][:-1]])  # neither side of the entry's place is a close call
    assert np.array_equal(got["index"][settled], want["index"][settled]), what
    dev = np.abs(got["distance"] - want["distance"])[settled]
    DEVIATION["max"] = max(DEVIATION["max"], float(dev.max()) if len(dev) else 0.0)
    assert (dev <= ref.DISTANCE_TOL).all(), (what, dev.max())
    ok = settled & ~want["shift_band"]
    assert np.array_equal(got["shift"][ok], want["shift"][ok]), what
    print("%s: %d results, greatest deviation of a distance so far %.3g" % (what, m, DEVIATION["max"]))


@pytest.mark.parametrize("N", SIZES)
def test_query_sizes(N):
    db = database(N)
    rng = np.random.default_rng(N)
    q = random_image(rng, 20, 60) if N < 10 else (0.5 * pool()[N // 2] + 0.5 * random_image(rng, 20, 60)).astype(F32)
    for k in (1, 5, 32):
        got = db.query(q, k=k, return_all=True)
        want = ref.query(q, pool()[:N], k=k)
        assert len(got["index"]) == min(k, N)  # k > the number of candidates: fewer results
        check_query(got, want, "N = %d, k = %d" % (N, k))
    if N >= 10:
        assert db.query(q, k=1)["index"][0] == N // 2


@pytest.mark.parametrize("first, count", [(10, 40), (64, 1), (299, 1), (0, 300), (300, 0), (17, 0), (60, 10)])
def test_query_ranges(first, count):
    db = database(300)
    q = ref.turned(pool()[first + count // 2 if count else 0], 11)
    before = (api.places_query_launches(), api.places_waits())
    got = db.query(q, k=5, first=first, count=count, return_all=True)
    check_query(got, ref.query(q, pool(), first, count, 5), "[%d, %d + %d)" % (first, first, count))
    if count == 0:  # an empty range launches nothing and waits for nothing
        assert len(got["index"]) == 0 and (api.places_query_launches(), api.places_waits()) == before
    else:
        assert got["index"][0] == first + count // 2 and got["shift"][0] == 11 and abs(got["distance"][0]) <= ref.DISTANCE_TOL
        assert (got["index"] >= first).all() and (got["index"] < first + count).all()
    # exclude_recent leaves the latest entries out
    r = db.query(q, k=32, exclude_recent=290)
    assert (r["index"] < 10).all() and len(r["index"]) == 10


@pytest.mark.parametrize("R, S", SHAPES[1:])
def test_query_shapes(R, S):
    """(four slices of ceil(S / 4) columns, 4 S work items over 256 threads: S = 7, 60, 64, 256 take every path of the match kernel)"""
    N = 9
    db = database(N, R, S)
    rng = np.random.default_rng(R + S)
    for q in ((0.7 * pool(R, S)[4] + 0.3 * random_image(rng, R, S)).astype(F32), ref.turned(pool(R, S)[6], S // 3)):
        got = db.query(q, k=N, return_all=True)
        check_query(got, ref.query(q, pool(R, S)[:N], k=N), "(%d, %d)" % (R, S))
    assert got["index"][0] == 6 and got["shift"][0] == S // 3 and abs(got["distance"][0]) <= ref.DISTANCE_TOL
    np.testing.assert_array_equal(got["yaw"], got["shift"] * (2 * np.pi / S))


def test_query_of_one_cell():
    """(1, 1): every pair of non-empty images has cosine 1, so every distance is 0 up to a rounding and every order decision of the
    restatement is in band; what the rule says is asserted directly: shift 0, distances within the tolerance of 0, an empty entry exactly 1"""
    db = sga.PlaceDatabase(rings=1, sectors=1)
    for v in (2.5, 0.0, 1e-3, 7.0):
        db.add_descriptor(F32([[v]]))
    r = db.query(F32([[3.0]]), k=4, return_all=True)
    assert (r["all_shift"] == 0).all() and r["all_distance"][1] == 1.0 and (np.abs(r["all_distance"][[0, 2, 3]]) <= ref.DISTANCE_TOL).all()
    assert r["index"][-1] == 1 and sorted(r["index"].tolist()) == [0, 1, 2, 3] and (np.diff(r["distance"]) >= 0).all()
    assert np.abs(r["all_distance"] - ref.shift_distances(F32([[3.0]]), db.descriptors())[:, 0]).max() <= ref.DISTANCE_TOL


def test_query_by_cloud_and_by_image_agree():
    db = sga.PlaceDatabase(max_range=60.0)
    clouds = [upload_relative(cloud_points(3000, 500 + i, L=60.0), None, None, ZERO) for i in range(6)]
    for c in clouds:
        db.add(c)
    probe = upload_relative(cloud_points(3000, 502, L=60.0)[::-1] + F32([0.05, 0.0, 0.0]), None, None, ZERO)
    by_cloud = db.query(probe, k=6, return_all=True)
    image = probe.scan_context(max_range=60.0)
    by_image = db.query(image, k=6, return_all=True)
    for key in ("index", "shift", "distance", "all_distance", "all_shift"):
        assert by_cloud[key].tobytes() == by_image[key].tobytes(), key
    assert by_cloud["index"][0] == 2
    check_query(by_cloud, ref.query(image, db.descriptors(), k=6), "by cloud")
    # with a centre: the cloud moved and the centre moved with it give the same descriptor, hence the same result
    moved = upload_relative(cloud_points(3000, 502, L=60.0)[::-1] + F32([0.05, 0.0, 0.0]) + F32([8.0, -16.0, 2.0]), None, None, ZERO)
    r = db.query(moved, k=6, center=[8.0, -16.0, 2.0], return_all=True)
    assert r["index"].tobytes() == by_cloud["index"].tobytes() and r["shift"].tobytes() == by_cloud["shift"].tobytes()


def test_query_ordering():
    R, S = 20, 60
    rng = np.random.default_rng(77)
    a, b = random_image(rng, R, S), random_image(rng, R, S)
    columns = np.repeat(random_image(rng, R, 1), S, axis=1)  # identical columns
    holes = random_image(rng, R, S)  # (an image of its own: with a's columns it would lie at distance 0 from a as well — empty columns do not count)
    holes[:, [0, 1, 17, 40, 59]] = 0.0
    db = sga.PlaceDatabase()
    for img in (a, b, a, columns, holes, np.zeros((R, S), F32), ref.turned(a, 13)):
        db.add_descriptor(img)
    # two bytewise-equal entries: the lower index first, equal distance bits (entry 6, the turned copy, lies within a rounding of them:
    # before or behind the two, never between)
    mix = (0.9 * a + 0.1 * b).astype(F32)
    r = db.query(mix, k=7, return_all=True)
    order = r["index"].tolist()
    assert order.index(2) == order.index(0) + 1 and r["all_distance"][0].tobytes() == r["all_distance"][2].tobytes() and r["all_shift"][0] == r["all_shift"][2] == 0
    assert r["distance"][order.index(0)].tobytes() == r["distance"][order.index(2)].tobytes()
    assert (np.diff(r["distance"]) >= 0).all() and sorted(order) == list(range(7))
    assert order[-1] == 5 and r["distance"][-1] == 1.0 and r["all_shift"][5] == 0  # the empty entry: distance exactly 1, shift 0
    want = ref.shift_distances(mix, db.descriptors())
    assert np.abs(r["all_distance"] - want.min(axis=1)).max() <= ref.DISTANCE_TOL
    # an image of identical columns against itself: every shift adds the same terms, so every d(s) has the same bits and the shift is 0
    r = db.query(columns, k=7, return_all=True)
    assert r["all_shift"][3] == 0 and r["index"][0] == 3 and r["shift"][0] == 0 and abs(r["distance"][0]) <= ref.DISTANCE_TOL
    # an all-empty query: distance exactly 1, shift 0, index order
    r = db.query(np.zeros((R, S), F32), k=7, return_all=True)
    assert r["index"].tolist() == list(range(7)) and (r["distance"] == 1.0).all() and (r["shift"] == 0).all() and (r["all_distance"] == 1.0).all()
    # entries with some empty columns
    r = db.query(ref.turned(holes, 21), k=3, return_all=True)
    assert r["index"][0] == 4 and r["shift"][0] == 21 and abs(r["distance"][0]) <= ref.DISTANCE_TOL
    plain = sga.PlaceDatabase()  # (against the restatement in a database without the ties planted above: those are decisions in band)
    stored = np.stack([b, holes, random_image(rng, R, S), a])
    stored[2][:, 30:36] = 0.0
    for img in stored:
        plain.add_descriptor(img)
    partly = ref.turned(holes, 21).copy()
    partly[:, 5:9] = 0.0  # a query with empty columns of its own as well
    for q in (ref.turned(holes, 21), partly):
        r = plain.query(q, k=4, return_all=True)
        check_query(r, ref.query(q, stored, k=4), "empty columns")
        assert r["index"][0] == 1 and r["shift"][0] == 21 and abs(r["distance"][0]) <= ref.DISTANCE_TOL
    # a turned copy: distance 0 within tolerance at the expected shift, in both directions (the three copies lie within a rounding of
    # each other: the equal two keep their order, the third may stand on either side)
    r = db.query(a, k=3, return_all=True)
    order = r["index"].tolist()
    assert sorted(order) == [0, 2, 6] and order.index(2) == order.index(0) + 1 and (np.abs(r["distance"]) <= ref.DISTANCE_TOL).all()
    assert r["all_shift"][[0, 2, 6]].tolist() == [0, 0, S - 13]
    r = db.query(ref.turned(a, 13), k=3, return_all=True)
    assert sorted(r["index"].tolist()) == [0, 2, 6] and r["all_shift"][[0, 2, 6]].tolist() == [13, 13, 0] and (np.abs(r["distance"]) <= ref.DISTANCE_TOL).all()


def test_two_calls_give_the_same_bytes():
    cloud = sga.PointCloud(scan())
    assert cloud.scan_context().tobytes() == cloud.scan_context().tobytes()
    db1, db2 = sga.PlaceDatabase(), sga.PlaceDatabase()
    clouds = [upload_relative(cloud_points(4000, 900 + i), None, None, ZERO) for i in range(5)]
    for db in (db1, db2):
        for c in clouds:
            db.add(c)
        for i in range(70):
            db.add_descriptor(pool()[i])
    assert db1.descriptors().tobytes() == db2.descriptors().tobytes()
    probe = upload_relative(cloud_points(4000, 903) + F32([0.1, 0.1, 0.0]), None, None, ZERO)
    results = [db.query(probe, k=32, return_all=True) for db in (db1, db2, db1)]
    for key in ("index", "shift", "distance", "all_distance", "all_shift"):
        assert results[0][key].tobytes() == results[1][key].tobytes() == results[2][key].tobytes(), key
    assert results[0]["index"][0] == 3


# ---- commands and waits -------------------------------------------------------------------------------------------------------------------
def counters():
    return np.array([api.places_add_launches(), api.places_query_launches(), api.places_waits()])


def test_launch_and_wait_counts():
    """an add is three commands (fill, descriptor, norms), one for an empty cloud, one for an image, one more when
    the database grows; no host wait on a stream-ordered context, one on a blocking one.  A query is four commands by cloud (three for an
    empty cloud), two by image, and exactly one wait; over zero candidates nothing.  scan_context: three (two for an empty cloud), one wait."""
    pts, image = cloud_points(3000, 1), pool()[0]
    for ordered in (False, True):
        ctx = sga.Context()
        ctx.set_stream_ordered(ordered)
        cloud, empty = sga.PointCloud(pts, ctx=ctx), sga.PointCloud(np.zeros((0, 3), F32), ctx=ctx)
        ctx.synchronize()
        db = sga.PlaceDatabase(ctx)
        wait = 0 if ordered else 1
        c = counters()
        db.add(cloud)
        assert (counters() - c).tolist() == [3, 0, wait]
        c = counters()
        db.add(empty)
        assert (counters() - c).tolist() == [1, 0, wait]
        c = counters()
        db.add_descriptor(image)
        assert (counters() - c).tolist() == [1, 0, wait]
        c = counters()
        r = db.query(cloud, k=3)
        assert (counters() - c).tolist() == [0, 4, 1] and r["index"][0] == 0
        c = counters()
        r = db.query(empty, k=3)
        assert (counters() - c).tolist() == [0, 3, 1] and (r["distance"] == 1.0).all()
        c = counters()
        r = db.query(image, k=3, return_all=True)
        assert (counters() - c).tolist() == [0, 2, 1] and r["index"][0] == 2
        c = counters()
        assert len(db.query(cloud, k=3, first=1, count=0)["index"]) == 0 and len(db.query(image, k=3, first=3, count=0)["index"]) == 0
        assert (counters() - c).tolist() == [0, 0, 0]
        c = counters()
        cloud.scan_context()
        assert (counters() - c).tolist() == [3, 0, 1]
        c = counters()
        assert not empty.scan_context().any()
        assert (counters() - c).tolist() == [2, 0, 1]
        for i in range(3, 64):
            db.add_descriptor(image)
        c = counters()
        db.add(cloud)  # the 65th entry: the database grows by one device-to-device copy
        assert (counters() - c).tolist() == [4, 0, wait]
        # what a stream-ordered add left in flight is what the next call finds
        assert np.array_equal(db.descriptors(64, 1)[0].view(U32), db.descriptors(0, 1)[0].view(U32)) and not db.descriptors(1, 1).any()
        ctx.synchronize()


# ---- refusals on real handles -------------------------------------------------------------------------------------------------------------
def message():
    return sga.load().sga_last_error().decode()


def test_refusals_on_real_handles():
    db = database(65)
    lib, ctx = sga.load(), db.ctx
    out = (_lib.PlaceMatch * 32)()
    out[0].index = 0xDEAD
    found = C.c_size_t(0xDEAD)
    image = np.ascontiguousarray(pool()[0])
    fp, pm = C.POINTER(C.c_float), C.POINTER(_lib.PlaceMatch)
    cloud = sga.PointCloud(cloud_points(100, 2))
    before = counters()
    for first, count in ((0, 66), (65, 1), (66, 0), (1 << 63, 1 << 63), (3, (1 << 64) - 2)):
        assert lib.sga_places_query_descriptor(ctx.h, db.h, image.ctypes.data_as(fp), first, count, 1, C.cast(out, pm), C.byref(found), None, None) == 1
        assert "reach beyond the database's 65" in message()
        assert lib.sga_places_query(ctx.h, db.h, cloud.h, None, first, count, 1, C.cast(out, pm), C.byref(found), None, None) == 1
        assert "reach beyond the database's 65" in message()
        assert lib.sga_places_download(ctx.h, db.h, first, count, image.ctypes.data_as(fp)) == 1 and "reach beyond" in message()
    for pos, value in ((0, np.nan), (61, -1.0), (1199, np.inf), (600, -np.inf), (7, -1e-30)):
        bad = image.copy()
        bad.reshape(-1)[pos] = value
        index = C.c_size_t(0xDEAD)
        assert lib.sga_places_add_descriptor(ctx.h, db.h, bad.ctypes.data_as(fp), C.byref(index)) == 1 and index.value == 0xDEAD
        assert "image value %d (ring %d, sector %d)" % (pos, pos // 60, pos % 60) in message(), message()
        assert lib.sga_places_query_descriptor(ctx.h, db.h, bad.ctypes.data_as(fp), 0, 65, 1, C.cast(out, pm), C.byref(found), None, None) == 1
        assert "image value %d (ring %d, sector %d)" % (pos, pos // 60, pos % 60) in message(), message()
    assert out[0].index == 0xDEAD and found.value == 0xDEAD and len(db) == 65  # outputs untouched, nothing added
    assert (counters() == before).all()
    with pytest.raises(ValueError):
        db.add_descriptor(np.zeros((60, 20), F32))
    with pytest.raises(sga.SgaError, match="k 0 outside"):
        db.query(image, k=0)


@pytest.mark.skipif(sga.load().sga_device_count() < 2, reason="needs a second GPU")
def test_another_device_is_refused():
    other = sga.Context(device=1)
    db, cloud = database(2), sga.PointCloud(cloud_points(100, 2))
    far_cloud, far_db = sga.PointCloud(cloud_points(100, 2), ctx=other), sga.PlaceDatabase(other)
    index, found, out = C.c_size_t(0xDEAD), C.c_size_t(0xDEAD), (_lib.PlaceMatch * 1)()
    lib = sga.load()
    before = counters()
    assert lib.sga_places_add(other.h, db.h, far_cloud.h, None, C.byref(index)) == 1 and "database lives on another device" in message()
    assert lib.sga_places_add(db.ctx.h, db.h, far_cloud.h, None, C.byref(index)) == 1 and "cloud lives on another device" in message()
    assert lib.sga_places_add(db.ctx.h, far_db.h, cloud.h, None, C.byref(index)) == 1 and "database lives on another device" in message()
    assert lib.sga_places_query(db.ctx.h, db.h, far_cloud.h, None, 0, 2, 1, out, C.byref(found), None, None) == 1 and "cloud lives on another device" in message()
    assert lib.sga_places_query(other.h, db.h, far_cloud.h, None, 0, 2, 1, out, C.byref(found), None, None) == 1 and "database lives on another device" in message()
    img = np.zeros((20, 60), F32)
    assert lib.sga_cloud_scan_context(other.h, cloud.h, C.byref(api._place_params()), None, img.ctypes.data_as(C.POINTER(C.c_float))) == 1 and "cloud lives on another device" in message()
    assert index.value == 0xDEAD and found.value == 0xDEAD and (counters() == before).all()


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_places(tmp_path):
    """include/small_gicp_amd.hpp: PlaceParams, Places and PointCloud::scan_context (tests/cpp/test_cpp_places.cpp, compiled with g++ as
    test_cloud_outliers_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_places"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_places.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd", "-Wl,-rpath," + libdir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    frames = [4, 8, 12, 16, 20]
    files = []
    for f in frames:
        files.append(str(tmp_path / ("k%d.f32" % f)))
        open(files[-1], "wb").write(scan(f).tobytes())
    Tq = synthetic._sensor_pose(12)
    Tq[:3, :3] = Tq[:3, :3] @ synthetic._rot([0, 0, 1], np.deg2rad(90.0))
    revisit = synthetic.scan_at(Tq, n_az=600, seed=5)
    open(tmp_path / "q.f32", "wb").write(revisit.tobytes())
    p = subprocess.run([str(exe), "20", "60", "3", str(tmp_path / "q.f32")] + files, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    lines = [ln.split() for ln in p.stdout.splitlines()]
    assert lines[0] == ["PLACES", "size", "5", "cells", "1200"]
    assert lines[-2] == ["IMAGE", "same", "1", "descriptor", "1", "reloaded", "1"]
    assert lines[-1] == ["REFUSE", "k", "1", "image", "1"]
    # the same through Python gives the same numbers
    db = sga.PlaceDatabase()
    for f in frames:
        db.add(sga.PointCloud(scan(f)))
    want = db.query(sga.PointCloud(revisit), k=3)
    got = [ln for ln in lines if ln[0] == "MATCH"]
    assert [int(g[1]) for g in got] == want["index"].tolist() and [int(g[2]) for g in got] == want["shift"].tolist()
    assert [float(g[3]) for g in got] == want["distance"].tolist()
    assert want["index"][0] == 2 and want["shift"][0] == 15  # frame 12, a quarter turn


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def revisit_run():
    """the database of scan_at(_sensor_pose(f)), f = 0, 2, .., 78, and the four revisits of odometry.REVISITS: stored poses moved by at most
    0.3 m and turned by 150, -75, 33 and 180 degrees (computed once for the four cases)"""
    assert [(f, y) for f, y, _ in odometry.REVISITS] == [(10, 150.0), (30, -75.0), (50, 33.0), (70, 180.0)]
    assert max(np.hypot(dx, dy) for _, _, (dx, dy) in odometry.REVISITS) <= 0.3 + 1e-12
    return odometry.run_synthetic_revisit(from_identity=True)


@pytest.mark.parametrize("case", range(4))
def test_end_to_end_revisit(case):
    """Retrieval, the yaw with its sign, and the loop closure GICP reaches from yaw_guess(shift) and not from the identity.  The bounds are
    twice the termination tolerances (1e-3 m, 0.1 degrees) against the generator's relative pose.  The scans keep their 2030 azimuth
    columns: with fewer the registration itself, started at the truth, no longer lies within 2 mm of the generator's pose on every revisit
    (DESIGN.md section 3.25 has the figures, the CPU oracle's among them)."""
    run = revisit_run()
    r = run["revisits"][case]
    frame, yaw_deg, _ = odometry.REVISITS[case]
    assert run["keyframes"] == 40 and r["frame"] == frame
    print("revisit of frame %d turned %g deg: retrieved %d (rank of the true place %d) at %.2f m, shift %d, distance %.3f, yaw error %.4f rad, GICP from the guess %.2e m %.2e rad, from the identity %.2e m %.2e rad"
          % (frame, yaw_deg, r["retrieved"], r["rank"], r["place_error_m"], r["shift"], r["distance"], r["yaw_error_rad"], *r["pose_error"], *r["identity_error"]))
    assert r["place_error_m"] <= 2.5
    # the shift with its sign: T_entry^-1 T_query = rotz(yaw) gives round(yaw / (2 pi / S)) mod S, within one sector
    T_true = r["T_true"]
    yaw = np.arctan2(T_true[1, 0], T_true[0, 0])
    sector = 2 * np.pi / 60
    off = (r["shift"] - yaw / sector + 30) % 60 - 30
    assert abs(off) <= 1.0, (r["shift"], yaw / sector)
    if r["retrieved"] == frame:
        assert abs((r["shift"] - np.deg2rad(yaw_deg) / sector + 30) % 60 - 30) <= 1.0
    setting = sga.make_setting("GICP")
    tol_t, tol_r = 2 * setting.translation_eps, 2 * setting.rotation_eps
    assert (tol_t, round(tol_r, 6)) == (2e-3, 3.491e-3)
    dt, dr = r["pose_error"]
    assert r["converged"] and dt <= 2e-3 and dr <= 3.5e-3
    dt, dr = r["identity_error"]
    assert not (dt <= 2e-3 and dr <= 3.5e-3), "align from the identity reached the pose: the case proves nothing"

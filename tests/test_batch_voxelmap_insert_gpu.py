"""The batched incremental voxel-map insert (sga_voxelmap_insert_batch) against the lone sga_voxelmap_insert.

Every case feeds the same sequence of (cloud, T) rounds to two sets of maps: one set through insert_batch, one call per round, and a twin
set through the lone insert, one call per member and round.  After EVERY round every member is compared with its twin as bit equality of
download() (coordinates, fp32 means and covariances, counts), size(), sga_index_origin, and sga_index_knn over 1 / 7 / 27 search offsets
(queries: the round's points in the map's frame plus a handful far outside).  No tolerance appears except in the oracle case, which uses
the assertions and the 2e-7 bounds of tests/test_gpu_parity.py::test_incremental_voxelmap_matches_oracle.  LRU stamps and the insert
counter are observed through the sweeps: a member whose counter or stamps were off would sweep in another round or drop other voxels.
The shapes are the smallest at which each mechanism of the chain can fail."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from conftest import ROOT
from small_gicp_amd import api
from test_batch_maps_gpu import SHIFT

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 1  # SGA_ERR_INVALID
FAR = np.array([[5e3, 5e3, 5e3], [-7e3, 1.0, 2.0], [0.0, 0.0, 4e5], [3e6, 0.0, 0.0], [-3e6, -3e6, 1.0]])
FLAT_KINDS = [sga.IncrementalVoxelMap, sga.IncrementalVoxelMapNormal, sga.IncrementalVoxelMapCov, sga.IncrementalVoxelMapNormalCov]


def scan(n, seed, lo=(-20, -20, -2), hi=(20, 20, 2)):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F32)


def cloud_of(points, ctx=None, normals=False):
    """a device cloud with covariances (and normals) from the estimation at k = 10"""
    c = sga.PointCloud(np.ascontiguousarray(points), ctx=ctx)
    if c.size() == 0:
        return cloud_of(scan(16, 99), ctx, normals).slice(0, 0)  # an empty cloud that has the attributes
    (sga.estimate_normals_covariances if normals else sga.estimate_covariances)(c, None, 10)
    return c


def with_points(cloud, points):
    """the covariances of `cloud` under other points: how a cloud gets NaN points (no neighbour search accepts them)"""
    c6 = np.empty((cloud.size(), 6), F32)
    api.check(sga.load().sga_cloud_download(cloud.ctx.h, cloud.h, None, None, api._fp(c6)))
    return sga.PointCloud(np.ascontiguousarray(points), covs=c6, ctx=cloud.ctx)


def pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def grid_points(n, step=2.0):
    """n points, each in a voxel of its own at a 1 m leaf under any of the test's poses (rotations of a few degrees, spacing 2 m)"""
    g = np.arange(12, dtype=F32)
    return (np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:n] * step + 0.5).astype(F32)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def origin_of(m):
    o = np.zeros(3)
    api.check(sga.load().sga_index_origin(m.h, api._dp(o)))
    return o


def assert_same(label, got, want, queries=None):
    assert got.size() == want.size(), (label, "size", got.size(), want.size())
    a, b = got.download(), want.download()
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and np.array_equal(raw(x), raw(y)), (label, "download()[%d] differs from the lone insert" % i)
    assert np.array_equal(origin_of(got), origin_of(want)), (label, "origin", origin_of(got), origin_of(want))
    if queries is None or got.size() == 0:
        return
    for offsets in (1, 7, 27):
        got.set_search_offsets(offsets)
        want.set_search_offsets(offsets)
        (ia, da), (ib, db) = got.batch_knn_search(queries, 1), want.batch_knn_search(queries, 1)
        assert np.array_equal(np.asarray(ia), np.asarray(ib)) and np.array_equal(raw(np.asarray(da)), raw(np.asarray(db))), (label, "search over", offsets, "voxels differs")
    got.set_search_offsets(1)
    want.set_search_offsets(1)


def new_maps(specs, ctx=None):
    """specs: (kind or None = GaussianVoxelMap, leaf, (horizon, clear_cycle) or None) per member"""
    maps = []
    for kind, leaf, lru in specs:
        m = (kind or sga.GaussianVoxelMap)(leaf, ctx=ctx)
        if lru:
            m.set_lru(*lru)
        maps.append(m)
    return maps


def run_rounds(label, specs, rounds, ctx=None, want_plans=None):
    """rounds: per round a list of (cloud, T or None) per member.  Returns (batch maps, twins, sizes per round)."""
    batch, twins = new_maps(specs, ctx), new_maps(specs, ctx)
    sizes = []
    for r, members in enumerate(rounds):
        clouds = [c for c, _ in members]
        Ts = [np.eye(4) if T is None else T for _, T in members]
        if want_plans and want_plans[r]:
            plan = api._voxelmap_insert_batch_plan(batch, clouds)
            for key, want in want_plans[r].items():
                assert plan[key] == want, (label, r, key, plan)
        sga.insert_batch(batch, clouds, None if all(T is None for _, T in members) else Ts)
        for m, (c, T) in zip(twins, members):
            m.insert(c, T)
        for k, (c, T) in enumerate(zip(clouds, Ts)):
            q = None
            if c.size():
                p = c.xyz64()[:600]
                p = p[np.isfinite(p).all(axis=1)]
                q = np.concatenate([p @ T[:3, :3].T + T[:3, 3], FAR])
            assert_same("%s round %d member %d" % (label, r, k), batch[k], twins[k], q)
        sizes.append([m.size() for m in batch])
        print("%-30s round %d sizes %s" % (label, r, sizes[-1]))
    return batch, twins, sizes


T1 = pose(0.01, -0.02, 0.05, [0.3, -0.2, 0.1])
T2 = pose(-0.02, 0.01, 0.11, [6.5, 3.2, -0.4])
T3 = pose(0.03, 0.02, -0.07, [-4.1, 7.7, 0.6])


# ---- block edges -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_clouds():
    pts = [scan(255, 1), scan(256, 2), scan(257, 3), grid_points(127), grid_points(128), grid_points(129), scan(2049, 4), scan(1, 5)]
    return [cloud_of(p) for p in pts], [cloud_of(p) for p in [scan(257, 6), scan(255, 7), scan(256, 8), grid_points(129, 2.5), grid_points(127, 2.5), grid_points(128, 2.5), scan(700, 9), scan(3, 10)]]


def test_block_edges(edge_clouds):
    """Members of 255 / 256 / 257 points around the 256-point key workgroup and of 127 / 128 / 129 runs around the 128-run update block in
    one call of eight; every one of them alone (B = 1); one member first and last of its call."""
    first, second = edge_clouds
    B = len(first)
    specs = [(None, 1.0, None)] * B
    rounds = [[(c, T1) for c in first], [(c, T2) for c in second]]
    _, _, sizes = run_rounds("edges B=8", specs, rounds, want_plans=[{"forest": B, "lone": 0, "empty": 0, "member_bits": 3, "end_bit": 52, "points": sum(c.size() for c in first)}, None])
    assert sizes[0][3:6] == [127, 128, 129]  # one run per point: exactly these run counts reached the update launch
    for k in range(B):
        run_rounds("edges alone %d" % k, specs[:1], [[(first[k], T1)], [(second[k], T2)]], want_plans=[{"forest": 1, "member_bits": 0, "end_bit": 49}, None])
    order = [2, 0, 1, 3, 4, 5, 6, 7]  # member 2 (257 points) first ...
    run_rounds("edges, 257 first", specs, [[(first[k], T1) for k in order], [(second[k], T2) for k in order]])
    order = order[1:] + order[:1]  # ... and last
    run_rounds("edges, 257 last", specs, [[(first[k], T1) for k in order], [(second[k], T2) for k in order]])


# ---- three rounds: creation, growth + rehash, sweep --------------------------------------------------------------------------------------
def test_three_rounds_cross_growth_rehash_and_sweep():
    """Round 1 creates every voxel (at most 512: the arrays get 1024 places, the table 2048 slots); round 2 mixes existing and new voxels and
    leaves more than 1024 (n_total > vcap: the arrays grow; 2 n_total > 2048: the table is rebuilt); round 3 falls on the sweep of the members
    with clear_cycle 3 (horizon 1: the voxels last touched in round 1 go) and adds few voxels: their size drops.  The members have different
    clear cycles: some sweep in round 2, some in round 3, some not at all."""
    lrus = [(1, 3), None, (1, 2), (1, 3), (100, 10)]
    specs = [(None, 1.0, lru) for lru in lrus]
    B = len(specs)
    r1 = [cloud_of(scan(3000, 20 + k, lo=(0, 0, 0), hi=(6, 7, 5))) for k in range(B)]  # posed by T1 (shift and spread below 1 m each): at most 8 x 9 x 7 = 504 voxels
    r2 = [cloud_of(scan(7000, 30 + k, lo=(-2, -2, 0), hi=(10, 10, 8))) for k in range(B)]  # 1152 voxels before T2, a fifth of them over round 1's
    r3 = [cloud_of(scan(300, 40 + k, lo=(0, 0, 0), hi=(4, 4, 2))) for k in range(B)]
    far3 = pose(0.03, 0.02, -0.07, [40.0, 40.0, 0.0])  # away from every earlier voxel
    _, _, sizes = run_rounds("three rounds", specs, [[(c, T1) for c in r1], [(c, T2) for c in r2], [(c, far3) for c in r3]])
    for k in range(B):
        assert sizes[0][k] <= 512, (k, sizes)
        assert sizes[1][k] > 1024 or lrus[k] == (1, 2), (k, sizes)  # (the member that sweeps in round 2 grew before it swept)
    assert sizes[1][2] < sizes[1][1]
    for k in (0, 3):
        assert sizes[2][k] < sizes[1][k], (k, sizes)  # the sweep removed voxels
    for k in (1, 4):
        assert sizes[2][k] > sizes[1][k], (k, sizes)  # no sweep: the map only grows


# ---- keys --------------------------------------------------------------------------------------------------------------------------------
def test_keys_across_members_frames_and_leaves():
    """The same cloud in three members and a slightly moved copy (equal voxel coordinates across member boundaries), an octant whose first
    voxel is (0, 0, 0) behind a member with dropped points (adjacent keys), negative coordinates, maps of different leaf sizes in one call,
    a geo-referenced cloud beside its twin at the origin, and a pose with a translation of kilometres."""
    a = scan(1500, 50, lo=(-20, -20, -6), hi=(20, 20, 6))
    a[:300] = np.round(a[:300])  # on the faces of voxels, negative ones included
    b = (a + np.random.default_rng(51).uniform(-0.01, 0.01, a.shape)).astype(F32)
    tail = scan(700, 52)
    tail[-150:] = [3e6, 1.0, 1.0]  # beyond 2^20 voxels at every leaf of this test
    octant = scan(900, 53, lo=(0, 0, 0), hi=(12, 12, 3))
    octant[0] = [0.5, 0.5, 0.5]
    ca, cb, ct, co = cloud_of(a), cloud_of(b), cloud_of(tail), cloud_of(octant)
    geo = with_points(ca, a.astype(np.float64) + SHIFT)
    assert np.abs(geo.origin()).max() > 9e5
    km = pose(0.02, -0.01, 0.4, [5321.7, -2250.3, 12.5])
    specs = [(None, leaf, None) for leaf in (1.0, 1.0, 1.0, 1.0, 1.0, 0.5, 2.0, 4.0, 4.0, 2.0)]
    members = [ca, cb, ca, ct, co, ca, ca, geo, ca, cb]
    rounds = [[(c, None) for c in members], [(c, T2) for c in members[::-1]], [(c, km) for c in members]]
    batch, _, sizes = run_rounds("keys", specs, rounds, want_plans=[{"forest": 10, "lone": 0, "member_bits": 4, "end_bit": 53}, None, None])
    down = [m.download() for m in batch]
    assert (down[0][0] < 0).any() and (down[4][0] == 0).all(axis=1).any()
    assert sizes[2][0] > sizes[1][0] > sizes[0][0]


def test_identity_poses_as_null():
    """Ts = None hands the C call a NULL pose array: identities."""
    c = [cloud_of(scan(900, 60 + k)) for k in range(3)]
    run_rounds("null poses", [(None, 1.0, None)] * 3, [[(x, None) for x in c], [(x, None) for x in c[::-1]]])


# ---- dropped points ------------------------------------------------------------------------------------------------------------------------
def test_dropped_points_and_empty_clouds():
    """NaN points, points beyond +-2^20 voxels, a member that is all dropped, and a member with an empty cloud whose insert counter still
    advances: with clear_cycle 2 (horizon 1) its sweep falls into the round in which it receives nothing and removes every voxel."""
    base = cloud_of(scan(2000, 70))
    some = base.xyz().astype(F32).copy()
    some[::7] = [3e6, -3e6, 0.0]
    nans = base.xyz().astype(F32).copy()
    nans[::5, 1] = np.nan
    nans[3] = np.nan
    gone = np.full((500, 3), 3e6, F32) + np.arange(500, dtype=F32)[:, None]
    c_some, c_nan, c_gone = with_points(base, some), with_points(base, nans), with_points(cloud_of(scan(500, 71)), gone)
    empty = cloud_of(np.zeros((0, 3), F32))
    fresh = cloud_of(scan(800, 72, lo=(30, 30, 0), hi=(40, 40, 3)))
    specs = [(None, 1.0, None), (None, 1.0, None), (None, 1.0, None), (None, 1.0, (1, 2)), (None, 1.0, (1, 2))]
    rounds = [[(c_some, T1), (c_nan, T1), (c_gone, T1), (base, T1), (base, T1)],
              [(c_nan, T2), (c_gone, T2), (base, T2), (empty, T2), (fresh, T2)],
              [(empty, None), (empty, None), (empty, None), (empty, None), (empty, None)]]
    plans = [{"forest": 5, "empty": 0}, {"forest": 4, "empty": 1, "points": 2000 + 500 + 2000 + 800}, {"forest": 0, "empty": 5, "end_bit": 0}]
    _, _, sizes = run_rounds("dropped", specs, rounds, want_plans=plans)
    assert sizes[0][2] == 0 and sizes[1][1] == sizes[0][1]  # the all-dropped member creates nothing
    assert sizes[0][3] > 0 and sizes[1][3] == 0  # the sweep due in the empty round removed every voxel of round 1
    assert 0 < sizes[1][4] <= 800 and sizes[2] == sizes[1]  # beside it: only the voxels of round 2's cloud are left


# ---- fallbacks -----------------------------------------------------------------------------------------------------------------------------
def test_fallbacks_overflow_point_cap_and_flat_maps():
    cluster = scan(800, 80, lo=(0, 0, 0), hi=(30, 30, 3))
    far = cluster.copy()
    far[400:, 1] += 70000.0  # two clusters 70 000 voxels apart: within the lone key, beyond the batch key's 16 bits per axis
    below = cluster.copy()
    below[400:, 0] += 65000.0  # spans fewer than 65 536 voxels: stays in the chain
    wide, near, plain = cloud_of(far), cloud_of(below), cloud_of(scan(500, 81))
    specs = [(None, 1.0, None)] * 4
    _, _, sizes = run_rounds("overflow", specs, [[(plain, T1), (wide, T1), (near, T1), (wide, None)], [(wide, T2), (plain, T2), (wide, T2), (near, T2)]],
                             want_plans=[{"forest": 4, "lone": 0}, {"forest": 4, "lone": 0}])
    assert sizes[0][1] > 0 and sizes[1][0] > sizes[0][0]
    big = cloud_of(scan(262145, 82, lo=(-60, -60, -3), hi=(60, 60, 3)))
    most = big.slice(0, 262144)
    run_rounds("point cap", [(None, 1.0, None)] * 3, [[(plain, T1), (big, T1), (most, T1)], [(big, T2), (plain, T2), (plain, T2)]],
               want_plans=[{"forest": 2, "lone": 1, "points": 500 + 262144, "member_bits": 1}, {"forest": 2, "lone": 1, "points": 1000}])
    full = cloud_of(scan(1500, 83), normals=True)
    full2 = cloud_of(scan(1200, 84), normals=True)
    specs = [(None, 1.0, None)]
    for kind in FLAT_KINDS:
        specs += [(kind, 1.0, None), (None, 0.5, None)]
    B = len(specs)
    run_rounds("flat members", specs, [[(full, T1)] * B, [(full2, T2)] * B], want_plans=[{"forest": 5, "lone": 4, "empty": 0}, None])


# ---- status before any work ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_map_unchanged():
    lib = sga.load()
    good, other = cloud_of(scan(600, 90)), cloud_of(scan(500, 91))
    bare = sga.PointCloud(scan(400, 92))  # no covariances
    ctx = good.ctx
    maps = new_maps([(None, 1.0, None)] * 3)
    sga.insert_batch(maps, [good, other, good], [T1, T1, T2])
    before = [m.download() for m in maps]
    origins = [origin_of(m) for m in maps]
    launches = sga.voxelmap_insert_batch_launches()
    one_shot = sga.GaussianVoxelMap.from_cloud(good, 1.0)
    T = np.ascontiguousarray(np.stack([api._T16(T3)] * 3))

    def call(ms, cs, count=3):
        mh = (C.c_void_p * 3)(*[None if m is None else m.h.value for m in ms])
        ch = (C.c_void_p * 3)(*[None if c is None else c.h.value for c in cs])
        return lib.sga_voxelmap_insert_batch(ctx.h, mh, ch, api._dp(T), count), lib.sga_last_error().decode()

    cases = [
        ([maps[0], maps[1], maps[0]], [good, other, other], "map 2 appears twice"),
        ([maps[0], one_shot, maps[2]], [good, other, other], "not an incremental voxel map"),
        ([maps[0], maps[1], maps[2]], [good, other, bare], "needs point covariances"),
        ([maps[0], None, maps[2]], [good, other, other], "maps[1] is NULL"),
        ([maps[0], maps[1], maps[2]], [good, None, other], "clouds[1] is NULL"),
    ]
    for ms, cs, text in cases:
        rc, msg = call(ms, cs)
        assert rc == INVALID and text in msg, (rc, msg, text)
        if "NULL" not in text and "twice" not in text:
            assert "member" in msg, msg  # the member's number
    with pytest.raises(sga.SgaError):
        sga.insert_batch([maps[0], maps[0]], [good, other])
    assert call([None, None, None], [None, None, None], count=0)[0] == 0  # count == 0: SGA_OK, nothing looked at
    sga.insert_batch([], [])
    assert sga.voxelmap_insert_batch_launches() == launches  # refused before any device work
    for m, b, o in zip(maps, before, origins):
        assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(m.download(), b)) and np.array_equal(origin_of(m), o)
    # the maps are still usable, and a refusal did not advance a counter: the sweep of clear_cycle 2 falls on the next insert
    twins = new_maps([(None, 1.0, None)] * 3)
    for m, (c, Tm) in zip(twins, [(good, T1), (other, T1), (good, T2)]):
        m.insert(c, Tm)
    for m in maps + twins:
        m.set_lru(1, 2)
    sga.insert_batch(maps, [other, good, other], [T3, T3, T3])
    for k, (m, c) in enumerate(zip(twins, [other, good, other])):
        m.insert(c, T3)
        assert_same("after the refusals %d" % k, maps[k], m)
    assert 0 < maps[0].size() <= other.size()  # the sweep fell on this insert: only the voxels it touched are left


# ---- company -------------------------------------------------------------------------------------------------------------------------------
def test_interleaved_with_lone_inserts_and_other_batched_calls():
    """Batch calls and lone inserts alternating on the same maps; batched voxel grids, kd-tree forests and one-shot map builds (which share
    the box block and the staging ring) between them, in blocking and stream-ordered mode; one cloud made by another context of the device."""
    for ordered in (False, True):
        ctx, other = sga.Context(0), sga.Context(0)
        prev, prev_other = ctx.set_stream_ordered(ordered), other.set_stream_ordered(ordered)
        try:
            raws = [sga.PointCloud(scan(5000 + 400 * k, 100 + k), ctx=ctx) for k in range(3)]
            down = sga.voxelgrid_sampling_batch(raws, 0.5)
            sga.preprocess_batch(down, 10)
            batch, twins = new_maps([(None, 1.0, (1, 2))] * 3, ctx), new_maps([(None, 1.0, (1, 2))] * 3, ctx)
            sga.insert_batch(batch, down, [T1, T1, T1])
            one_shot = sga.build_gaussian_voxelmaps(down, 1.0)
            batch[1].insert(down[0], T2)  # a lone insert into a map of the batch
            down2 = sga.voxelgrid_sampling_batch(raws, 1.0)
            sga.preprocess_batch(down2, 10)
            foreign = sga.PointCloud(scan(3000, 110), ctx=other)
            sga.estimate_covariances(foreign, None, 10)  # in flight on the other context's stream when the call below takes it
            hs = (C.c_void_p * 3)(*[m.h.value for m in batch])
            cs = (C.c_void_p * 3)(down2[0].h.value, foreign.h.value, down2[2].h.value)
            T = np.ascontiguousarray(np.stack([api._T16(T3)] * 3))
            api.check(sga.load().sga_voxelmap_insert_batch(ctx.h, hs, cs, api._dp(T), 3))
            sga.insert_batch(batch[::-1], down, [T2, T2, T2])
            for m, seq in zip(twins, ([(down[0], T1), (down2[0], T3), (down[2], T2)], [(down[1], T1), (down[0], T2), (foreign, T3), (down[1], T2)], [(down[2], T1), (down2[2], T3), (down[0], T2)])):
                for c, Tm in seq:
                    m.insert(c, Tm)
            for k in range(3):
                assert_same("company ordered=%s member %d" % (ordered, k), batch[k], twins[k], np.concatenate([down[k].xyz64()[:500], FAR]))
            assert [m.size() for m in one_shot] == [sga.GaussianVoxelMap.from_cloud(c, 1.0).size() for c in down]
        finally:
            ctx.set_stream_ordered(prev)
            other.set_stream_ordered(prev_other)
        ctx.synchronize()
        other.synchronize()


def test_launch_count_does_not_grow_with_the_batch():
    """a round without growth and without a sweep: the maps already hold the voxels the round touches (the same clouds at the same pose)"""
    clouds = [cloud_of(scan(1500 + 100 * k, 120 + k)) for k in range(8)]
    maps = new_maps([(None, 1.0, None)] * 8)
    sga.insert_batch(maps, clouds, [T1] * 8)
    sizes = [m.size() for m in maps]
    n0 = sga.voxelmap_insert_batch_launches()
    sga.insert_batch(maps[:1], clouds[:1], [T1])
    n1 = sga.voxelmap_insert_batch_launches()
    sga.insert_batch(maps, clouds, [T1] * 8)
    n8 = sga.voxelmap_insert_batch_launches()
    maps[0].insert(clouds[0], T1)
    assert sga.voxelmap_insert_batch_launches() == n8  # the lone insert counts nothing
    assert [m.size() for m in maps] == sizes  # nothing was created: no growth
    assert n1 - n0 == n8 - n1 and 0 < n1 - n0 <= 12, (n0, n1, n8)


# ---- downstream ----------------------------------------------------------------------------------------------------------------------------
def _same_result(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error"))


def test_align_batch_against_batch_inserted_maps_equals_lone_inserted_maps():
    tgt, src, T = sga.synthetic.registration_pair(12_000)
    sizes = [2000, 5000, 11_000]
    targets = [cloud_of(tgt[:n]) for n in sizes]
    sources = [cloud_of(src[:n]) for n in sizes]
    batch, twins = new_maps([(None, 1.0, None)] * 3), new_maps([(None, 1.0, None)] * 3)
    for Tm, cs in ((None, targets), (pose(0, 0, 0.01, [0.2, 0.1, 0.0]), targets[::-1])):
        sga.insert_batch(batch, cs, None if Tm is None else [Tm] * 3)
        for m, c in zip(twins, cs):
            m.insert(c, Tm)
    st = sga.make_setting("GICP")
    for offsets in (1, 7):
        for m in batch + twins:
            m.set_search_offsets(offsets)
        a = sga.align_batch(batch, sources, [T] * 3, st)
        b = sga.align_batch(twins, sources, [T] * 3, st)
        for k in range(3):
            assert _same_result(a[k], b[k]), (offsets, k, a[k], b[k])
        assert a[-1].num_inliers > 0


def test_model_odometry_streams_with_batched_and_lone_inserts():
    from small_gicp_amd import odometry

    on = odometry.run_synthetic_model_batched(num_frames=6, streams=3, batched_insert=True)
    off = odometry.run_synthetic_model_batched(num_frames=6, streams=3)
    assert len(on["poses"]) == 3 and on["iterations"] == off["iterations"] and on["num_voxels"] == off["num_voxels"]
    for a, b in zip(on["poses"], off["poses"]):
        assert len(a) == len(b) > 1 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert all(len(it) > 0 and min(it) >= 1 for it in on["iterations"])


def test_a_batch_inserted_map_matches_the_oracle(orc):
    """One member's map after its three rounds (the last on a sweep) against orc.VoxelMap fed the same sequence: equal ids, coordinates and
    counts; means and covariances within the bounds of test_gpu_parity.py::test_incremental_voxelmap_matches_oracle (fp32 export of
    identical fp64 state)."""
    rounds = [[cloud_of(scan(3000, 130 + 10 * r + k, lo=(-12, -12, -2), hi=(12, 12, 2))) for k in range(3)] for r in range(3)]
    Ts = [T1, T2, T3]
    maps = new_maps([(None, 1.0, (1, 3))] * 3)
    ov = orc.VoxelMap(None, 1.0)
    ov.set_lru(1, 3)
    sizes = []
    for r in range(3):
        sga.insert_batch(maps, rounds[r], [Ts[r]] * 3)
        c = rounds[r][1]
        ov.insert(orc.Cloud(c.xyz().astype(np.float64), None, c.covs()[:, :3, :3], tree=False), Ts[r])
        gc, gm, g6, gn = maps[1].download()
        oc, om, ocv, on = ov.get()
        assert maps[1].size() == len(ov) and (gc == oc).all() and (gn == on).all(), r
        scale = max(1.0, float(np.abs(om).max()))
        assert np.abs(gm - om).max() <= 2e-7 * scale, r
        assert np.abs(api.mats_from_sym6(g6.astype(np.float64)) - ocv).max() <= 2e-7, r
        sizes.append(maps[1].size())
    print("oracle member sizes", sizes)


# ---- the C++ header ------------------------------------------------------------------------------------------------------------------------
def test_cpp_insert_batch(tmp_path):
    """include/small_gicp_amd.hpp: insert_batch over the C++ mirror against lone inserts (tests/cpp/test_cpp_voxelmap_insert_batch.cpp,
    compiled with g++ as test_batch_voxelmap_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_voxelmap_insert_batch"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_voxelmap_insert_batch.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = sga.synthetic.kitti_like_scan(0)
    (tmp_path / "p.f32").write_bytes(np.ascontiguousarray(pts[:30000, :3], dtype=F32).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("MEMBER")]
    assert len(rows) == 4, p.stdout
    for tok in rows:
        print(" ".join(tok))
        assert int(tok[3]) == int(tok[4]) > 0 and tok[6] == "1", tok  # voxels: batch, lone; downloads bit-equal

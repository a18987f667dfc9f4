"""The batched voxel grid (sga_voxelgrid_sampling_batch) against the lone call and against the grid's definition.

Every batched case goes through check_batch(), which asserts per member: (a) `n` and the records bit-equal to sga.voxelgrid_sampling on the
same cloud, (b) the input's origin, (c) voxelgrid_ref.check_grid against downsample_ref — the derived bound

    |out - mean| <= ulp32(max(|out|, |mean|)) / 2 + 2 (N + 2) 2^-53 max|p_i|

with no row exempt —, and for the call (d) that the batch plan (the host function the call itself runs) reached the regime the case names.
The shapes are the smallest at which each mechanism of the shared chain can fail: members around the 2048-key tile of the runs kernel,
member boundaries with equal short keys on either side, runs through both loops of the centroid body, a member of more than 64 tiles,
dropped and empty members, both composite key widths, members with different layouts and frames, and the members the chain leaves to the
lone routine.

LARGEST ERROR / BOUND OBSERVED = (not measured yet: this file has not run on an MI355X)"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
import test_voxelgrid_matrix as vm
from small_gicp_amd import api
from voxelgrid_ref import check_grid, downsample_ref

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = vm.TILE
INVALID = 1  # SGA_ERR_INVALID


def bits(cloud):
    return vm.records_of(cloud).view(np.uint32)


def check_batch(label, clouds, leaf, want_plan=None, refs=None):
    """The four checks of the module docstring; returns the outputs' records."""
    clouds = list(clouds)
    plan = api._voxelgrid_batch_plan(clouds, leaf)
    for key, want in (want_plan or {}).items():
        assert plan[key] == want, (label, key, plan[key], "expected", want, plan)
    outs = sga.voxelgrid_sampling_batch(clouds, leaf)
    assert len(outs) == len(clouds)
    got = []
    for k, (cloud, out) in enumerate(zip(clouds, outs)):
        lone = sga.voxelgrid_sampling(cloud, leaf)
        a, b = bits(out), bits(lone)
        assert out.size() == lone.size() and a.shape == b.shape and np.array_equal(a, b), (label, "member", k, "differs from the lone call", out.size(), lone.size())
        assert np.array_equal(out.origin(), cloud.origin()), (label, k, out.origin(), cloud.origin())
        ref = refs[k] if refs is not None else downsample_ref(vm.records_of(cloud), cloud.origin(), leaf)
        worst = check_grid(vm.records_of(out), ref, "%s / member %d" % (label, k))
        print("%-40s member %2d n=%7d voxels=%7d dropped=%6d largest run=%6d  error / bound %.3f" % (label, k, cloud.size(), len(ref.counts), len(ref.dropped), ref.counts.max() if len(ref.counts) else 0, worst))
        got.append(a)
    print("%-40s plan %s" % (label, plan))
    return got


def one_voxel(points, coord=(3, 1, 0), seed=50, leaf=0.25):
    return vm.in_voxels([coord], [points], leaf, np.random.default_rng(seed + points))


# ---- the cases of the shared chain -----------------------------------------------------------------------------------------------------
def test_sizes_around_the_tile():
    sizes = [1, 2047, 2048, 2049, 5000]
    clouds = [sga.PointCloud(vm.sized_scan(n)) for n in sizes]
    refs = [downsample_ref(vm.records_of(c), c.origin(), 0.25) for c in clouds]
    whole = check_batch("sizes around the tile", clouds, 0.25, {"key_bytes": 4, "forest": 5, "lone": 0, "tiles": 1 + 1 + 1 + 2 + 3, "member_bits": 3}, refs)
    for k in range(len(sizes)):  # every member alone, and first / last of the five
        alone = check_batch("size %d alone" % sizes[k], [clouds[k]], 0.25, {"forest": 1, "member_bits": 0, "tiles": (sizes[k] + TILE - 1) // TILE}, [refs[k]])
        assert np.array_equal(alone[0], whole[k])
        order = [(k + j) % len(sizes) for j in range(len(sizes))]  # member k first, member k - 1 last
        turned = check_batch("size %d first" % sizes[k], [clouds[j] for j in order], 0.25, {"forest": 5}, [refs[j] for j in order])
        for j, rec in zip(order, turned):
            assert np.array_equal(rec, whole[j]), (k, j)


def test_member_boundaries():
    """Equal short keys on either side of a member boundary (one-voxel members with equal contents, the same cloud twice), equal clouds
    side by side, and a member whose last run ends exactly on a tile edge — also as the last member, where nothing follows it."""
    dot = np.tile(np.array([[1.5, -2.0, 0.25]], F32), (700, 1))
    pts = vm.scan(3000, 60)
    edge = vm.aligned_run_cloud(TILE, TILE, 0)  # 4096 points: runs of one point, then one run [2048, 4096)
    a, b, c, d, e = sga.PointCloud(dot), sga.PointCloud(dot.copy()), sga.PointCloud(pts), sga.PointCloud(pts.copy()), sga.PointCloud(edge)
    ref = downsample_ref(vm.records_of(e), e.origin(), 0.25)
    assert len(edge) == 2 * TILE and ref.counts[-1] == TILE and ref.counts[:-1].max() == 1 and len(ref.dropped) == 0
    recs = check_batch("member boundaries", [a, b, a, c, d, e, c, e], 0.25, {"key_bytes": 4, "forest": 8, "lone": 0, "tiles": 3 + 2 + 2 + 2 + 2 + 2})
    assert np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2]) and len(recs[0]) == 1
    assert np.array_equal(recs[3], recs[4]) and np.array_equal(recs[3], recs[6]) and np.array_equal(recs[5], recs[7])


def test_long_runs():
    """One voxel holding 1, 8, 9, 33 and 257 points (no trip, the remainder loop alone, the unrolled loop with and without a remainder)
    beside ordinary members."""
    runs = [1, 8, 9, 33, 257]
    clouds = [sga.PointCloud(vm.sized_scan(3000))] + [sga.PointCloud(one_voxel(r)) for r in runs] + [sga.PointCloud(vm.run_shapes_cloud()), sga.PointCloud(vm.sized_scan(2500))]
    recs = check_batch("long runs", clouds, 0.25, {"key_bytes": 4, "forest": 8, "lone": 0})
    for r, rec in zip(runs, recs[1:]):
        assert len(rec) == 1, (r, len(rec))


def test_look_back_beyond_one_window():
    big = sga.PointCloud(vm.sized_scan(65 * TILE + 5))
    small = sga.PointCloud(vm.sized_scan(3000))
    check_batch("look-back: 66 tiles first", [big, small], 0.25, {"key_bytes": 4, "forest": 2, "tiles": 66 + 2})
    runs = sga.PointCloud(vm.two_voxel_cloud(65 * TILE + 5))  # two voxels: more than 64 consecutive tiles without a run head
    check_batch("look-back: 66 tiles of two runs, last", [small, runs], 1.0, {"forest": 2, "tiles": 2 + 66})


def test_dropped_points():
    bad = sga.PointCloud(vm.with_bad(vm.scan(5000, 25), vm.NONFINITE))
    far = sga.PointCloud(np.full((5000, 3), 1e9, F32))      # every row out of the grid: a box, every key the dropped one
    nan = sga.PointCloud(np.full((3000, 3), np.nan, F32))   # no box: the lone routine
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    tail = sga.PointCloud(vm.with_bad(vm.scan(TILE, 27), [[np.nan, 0, 0]] * 100))  # the first dropped point at 2048: the head of a tile
    clouds = [bad, far, empty, nan, tail, empty]
    check_batch("dropped points", clouds, 0.25, {"forest": 3, "lone": 1})
    outs = sga.voxelgrid_sampling_batch(clouds, 0.25)
    assert [o.size() for o in outs[1:4]] == [0, 0, 0] and outs[5].size() == 0 and outs[0].size() > 0
    assert api._voxelgrid_batch_plan([empty, empty], 0.25) == {"key_bytes": 0, "W": 0, "member_bits": 0, "forest": 0, "lone": 0, "tiles": 0}
    assert [o.size() for o in sga.voxelgrid_sampling_batch([empty, empty], 0.25)] == [0, 0]


def test_key_widths():
    scans = [sga.PointCloud(vm.scan(4000, 70 + j)) for j in range(3)]
    one = scans[0]._voxelgrid_plan(0.25)
    totals = [c._voxelgrid_plan(0.25)["total"] for c in scans]
    assert one["key_bytes"] == 4
    check_batch("composite key of 4 bytes", scans, 0.25, {"key_bytes": 4, "W": max(totals) + 1, "member_bits": 2, "forest": 3})
    wide = [sga.PointCloud(vm.layout_cloud(40.0, seed=80 + j, n=6000)) for j in range(2)]  # total 31: a lone 4-byte key, no room for a member number
    assert all(c._voxelgrid_plan(0.25)["total"] == 31 and c._voxelgrid_plan(0.25)["key_bytes"] == 4 for c in wide)
    check_batch("composite key of 8 bytes: W 32 + 1", wide, 0.25, {"key_bytes": 8, "W": 32, "member_bits": 1, "forest": 2})
    check_batch("one member of total 31: 4 bytes", wide[:1], 0.25, {"key_bytes": 4, "W": 32, "member_bits": 0, "forest": 1})
    wider = sga.PointCloud(vm.layout_cloud(80.0, seed=83, n=6000))  # total 32: an 8-byte key on its own
    assert wider._voxelgrid_plan(0.25)["key_bytes"] == 8
    check_batch("8 bytes: members of 4- and 8-byte lone keys", [scans[0], wider, wide[0], vm_outlier()], 0.25, {"key_bytes": 8, "forest": 4, "lone": 0})
    many = [scans[j % 3] for j in range(33)]  # 33 members: 6 bits of member number on 27 or so bits of key
    check_batch("8 bytes by the number of members", many, 0.25, {"key_bytes": 8 if max(totals) + 1 + 6 > 32 else 4, "member_bits": 6, "forest": 33})


def vm_outlier():
    return sga.PointCloud(vm.with_bad(vm.scan(5000, 17), [[2.6e5, 1.0, 0.5]], 17))  # 21 key bits on x: a total of 33 or more


def test_members_with_different_layouts_and_frames():
    geo = vm.geo_cloud(n=5000)
    clouds = [sga.PointCloud(geo), sga.PointCloud(vm.scan(5000, 31)), sga.PointCloud(geo[:2500] + np.array([512.0, -1024.0, 0.0])), sga.PointCloud((vm.scan(3000, 32) * F32(0.05)).astype(F32)),
              sga.PointCloud(vm.limit_cloud(n=3000) / 4.0)]
    assert clouds[0].origin().any() and clouds[2].origin().any() and not clouds[1].origin().any() and not np.array_equal(clouds[0].origin(), clouds[2].origin())
    layouts = {c._voxelgrid_plan(4.0)["bits"] for c in clouds}
    assert len(layouts) >= 2, layouts
    check_batch("different layouts and frames, leaf 4", clouds, 4.0, {"key_bytes": 4, "forest": 5, "lone": 0})
    check_batch("different layouts and frames, leaf 0.25", clouds, 0.25, {"forest": 5, "lone": 0})  # (the geo-referenced members: all dropped)


def test_fallbacks_to_the_lone_routine():
    pts = vm.scan(5000, 33)
    boxed = [sga.PointCloud(pts), sga.PointCloud(vm.scan(2049, 34))]
    sliced = sga.PointCloud(pts).slice(0, len(pts))  # made on the device: no box, the reference's 63-bit key
    large = sga.PointCloud(vm.sized_scan(262_145))
    assert sliced._voxelgrid_plan(0.25)["box"] is False and large._voxelgrid_plan(0.25)["speculative"] is False
    recs = check_batch("fallbacks", [boxed[0], sliced, large, boxed[1]], 0.25, {"key_bytes": 4, "forest": 2, "lone": 2, "tiles": 3 + 2})
    assert np.array_equal(recs[0], recs[1])
    check_batch("lone members only", [sliced], 0.25, {"key_bytes": 0, "forest": 0, "lone": 1, "tiles": 0})


# ---- the state a context keeps between calls ---------------------------------------------------------------------------------------------
def _state_clouds(ctx):
    return [sga.PointCloud(vm.sized_scan(n), ctx=ctx) for n in (5000, 2049, 3 * TILE)]


@pytest.mark.parametrize("stream_ordered", [False, True])
def test_lone_and_batched_calls_interleaved_on_one_context(stream_ordered):
    """One fresh context: lone, batch, lone (check_batch runs the lone call after the batched one for every member; a lone call comes
    first), the status words of each call found by the next under an older epoch."""
    ctx = sga.Context(0)
    ctx.set_stream_ordered(stream_ordered)
    clouds = _state_clouds(ctx)
    first = bits(sga.voxelgrid_sampling(clouds[0], 0.25))
    for rnd in range(2):
        recs = check_batch("interleaved %d%s" % (rnd, ", stream-ordered" if stream_ordered else ""), clouds, 0.25, {"forest": 3, "tiles": 3 + 2 + 3})
        assert np.array_equal(recs[0], first)
    ctx.set_stream_ordered(False)


def test_epoch_wraps_between_a_batched_and_a_lone_call():
    """sga_debug_set_voxelgrid_epoch to 2^30 - 2: the batched call takes the last epoch, 2^30 - 1; the lone call behind it finds the end,
    zeroes the status words (the batched call's among them) and starts again at 1; the batched call after that uses epoch 2 over words a
    lone call of epoch 1 and zeros fill.  (test_voxelgrid_matrix.test_epoch_wraps_at_2_30 has the argument why no look-back waits on a
    stale word; per member it is the same argument.)"""
    ctx = sga.Context(0)
    clouds = _state_clouds(ctx) + [sga.PointCloud(vm.sized_scan(70 * TILE), ctx=ctx)]
    want = [bits(sga.voxelgrid_sampling(c, 0.25)) for c in clouds]
    ctx._set_voxelgrid_epoch(2**30 - 2)
    outs = sga.voxelgrid_sampling_batch(clouds, 0.25)  # epoch 2^30 - 1
    lone = sga.voxelgrid_sampling(clouds[3], 0.25)      # the reset, epoch 1
    again = sga.voxelgrid_sampling_batch(clouds, 0.25)  # epoch 2
    for k in range(len(clouds)):
        assert np.array_equal(bits(outs[k]), want[k]) and np.array_equal(bits(again[k]), want[k]), k
    assert np.array_equal(bits(lone), want[3])
    with pytest.raises(sga.SgaError):
        ctx._set_voxelgrid_epoch(1)  # the epoch is 2: the counter did start again
    ctx._set_voxelgrid_epoch(2**30 - 1)
    outs = sga.voxelgrid_sampling_batch(clouds, 0.25)  # the batched call itself finds the end: the reset, epoch 1
    for k in range(len(clouds)):
        assert np.array_equal(bits(outs[k]), want[k]), k
    ctx._set_voxelgrid_epoch(1)


def test_a_member_made_by_another_context():
    a, b = sga.Context(0), sga.Context(0)
    b.set_stream_ordered(True)
    pts = vm.sized_scan(5000)
    foreign = sga.PointCloud(pts, ctx=b)
    own = sga.PointCloud(vm.sized_scan(2049), ctx=a)
    hs = (C.c_void_p * 2)(foreign.h.value, own.h.value)
    out = (C.c_void_p * 2)()
    assert sga.load().sga_voxelgrid_sampling_batch(a.h, hs, 2, 0.25, out) == 0
    got = [sga.PointCloud(ctx=a, _handle=C.c_void_p(out[k])) for k in range(2)]
    assert np.array_equal(bits(got[0]), bits(sga.voxelgrid_sampling(sga.PointCloud(pts), 0.25)))
    assert np.array_equal(bits(got[1]), bits(sga.voxelgrid_sampling(own, 0.25)))
    with pytest.raises(ValueError):
        sga.voxelgrid_sampling_batch([foreign, own], 0.25)  # the Python layer takes clouds of one context
    b.set_stream_ordered(False)


# ---- launches, errors, down the chain ------------------------------------------------------------------------------------------------------
def test_launch_count_does_not_grow_with_the_batch():
    clouds = [sga.PointCloud(vm.scan(5000, 90 + j)) for j in range(8)]

    def launches(cs):
        before = sga.voxelgrid_batch_launches()
        outs = sga.voxelgrid_sampling_batch(cs, 0.25)
        del outs
        return sga.voxelgrid_batch_launches() - before

    one, eight = launches(clouds[:1]), launches(clouds)
    print("launches of the shared chain: 1 cloud %d, 8 clouds %d" % (one, eight))
    assert one == eight == 4  # keys, the sort, runs, centroids


def test_argument_errors_on_a_live_device():
    lib = sga.load()
    ctx = sga.default_context()
    good = [sga.PointCloud(vm.scan(3000, 95)), sga.PointCloud(vm.scan(2049, 96))]
    want = [bits(sga.voxelgrid_sampling(c, 0.25)) for c in good]

    def raw(handles, leaf):
        hs = (C.c_void_p * len(handles))(*handles)
        out = (C.c_void_p * len(handles))(*[0xDEAD] * len(handles))
        return lib.sga_voxelgrid_sampling_batch(ctx.h, hs, len(handles), leaf, out), out

    rc, out = raw([good[0].h.value, None, good[1].h.value], 0.25)
    assert rc == INVALID and not any(out[k] for k in range(3)) and b"clouds[1] is NULL" in lib.sga_last_error()
    for leaf in (0.0, -1.0, float("nan")):
        rc, out = raw([good[0].h.value, good[1].h.value], leaf)
        assert rc == INVALID and not out[0] and not out[1] and b"leaf size must be positive" in lib.sga_last_error()
    with pytest.raises(sga.SgaError):
        sga.voxelgrid_sampling_batch(good, 0.0)
    assert lib.sga_voxelgrid_sampling_batch(ctx.h, None, 0, 0.25, None) == 0 and sga.voxelgrid_sampling_batch([], 0.25) == []
    assert sga.preprocess_points_batch([], 0.25, 10) == []
    outs = sga.voxelgrid_sampling_batch(good, 0.25)  # a good call after the failures
    assert all(np.array_equal(bits(o), w) for o, w in zip(outs, want))


def test_preprocess_points_batch_equals_the_lone_helper():
    raws = [sga.PointCloud(vm.scan(20_000, 97 + j)) for j in range(2)]
    pairs = sga.preprocess_points_batch(raws, 0.25, 10)
    for raw, (cloud, tree) in zip(raws, pairs):
        down = sga.voxelgrid_sampling(raw, 0.25)
        lone_tree = sga.KdTree(down)
        sga.estimate_covariances(down, lone_tree, 10)
        assert np.array_equal(bits(cloud), bits(down)) and cloud.covs().tobytes() == down.covs().tobytes() and tree.size() == lone_tree.size()


def test_odometry_with_batched_downsampling():
    from small_gicp_amd import odometry

    a = odometry.run_synthetic_batched(num_frames=5, batch=4, batched_preprocessing=True, batched_downsampling=True)
    b = odometry.run_synthetic_batched(num_frames=5, batch=4, batched_preprocessing=True, batched_downsampling=False)
    assert a["iterations"] == b["iterations"] and len(a["relative_poses"]) == 4
    assert all(np.array_equal(x, y) for x, y in zip(a["relative_poses"], b["relative_poses"]))
    assert all(np.array_equal(x, y) for x, y in zip(a["estimated"], b["estimated"]))

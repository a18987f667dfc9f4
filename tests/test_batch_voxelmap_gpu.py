"""The batched Gaussian voxel-map build (sga_index_build_gaussian_voxelmap_batch) against the lone build.

Every batched case goes through check_batch(), which asserts per member against sga_index_build_gaussian_voxelmap on the same cloud:
(a) equal sizes, (b) the arrays of sga_index_voxelmap_download (coords, means, cov6, counts) equal bit for bit, (c) sga_index_knn at k = 1
over 1, 7 and 27 search offsets with identical ids and distances, the queries being the member's own points plus a handful far outside,
and for the call (d) that the plan (the host function the call itself runs) reached the regime the case names.  The shapes are the
smallest at which each mechanism of the shared chain can fail: members around the 256-point key blocks and the 128-voxel finalize blocks,
member boundaries with equal and with numerically adjacent keys, dropped and empty members, negative coordinates, geo-referenced frames,
members whose voxel range overflows the 16 bits per axis of the batch key, and the members the plan leaves to the lone routine.

(This file has not run on an MI355X yet.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from conftest import ROOT, pose_error
from small_gicp_amd import api
from test_batch_maps_gpu import SHIFT, SIZES
from test_batch_gpu import POSE_TOL_R, POSE_TOL_T

pytestmark = pytest.mark.gpu
F32 = np.float32
INVALID = 1  # SGA_ERR_INVALID
FAR = np.array([[5e3, 5e3, 5e3], [-7e3, 1.0, 2.0], [0.0, 0.0, 4e5], [3e6, 0.0, 0.0], [-3e6, -3e6, 1.0]])


def cloud_of(points, ctx=None):
    """a device cloud with covariances from estimate_covariances(k = 10)"""
    c = sga.PointCloud(np.ascontiguousarray(points), ctx=ctx)
    if c.size() == 0:
        return cloud_of(scan(16, 99), ctx).slice(0, 0)  # an empty cloud that has covariances
    sga.estimate_covariances(c, None, 10)
    return c


def scan(n, seed, lo=(-20, -20, -2), hi=(20, 20, 2)):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F32)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def knn_bits(vm, queries):
    idx, d2 = vm.batch_knn_search(queries, 1)
    return np.asarray(idx), raw(np.asarray(d2))


def check_batch(label, clouds, leaf, want_plan=None, maps=None):
    """the checks of the module docstring; returns the downloads of the batch-built maps"""
    clouds = list(clouds)
    plan = api._voxelmap_batch_plan(clouds, leaf)
    for key, want in (want_plan or {}).items():
        assert plan[key] == want, (label, key, plan[key], "expected", want, plan)
    maps = sga.build_gaussian_voxelmaps(clouds, leaf) if maps is None else maps
    assert len(maps) == len(clouds)
    got = []
    for k, (cloud, m) in enumerate(zip(clouds, maps)):
        lone = sga.GaussianVoxelMap.from_cloud(cloud, leaf)
        assert m.size() == lone.size(), (label, "member", k, m.size(), lone.size())
        a, b = m.download(), lone.download()
        for name, x, y in zip(("coords", "means", "cov6", "counts"), a, b):
            assert x.shape == y.shape and np.array_equal(raw(x), raw(y)), (label, "member", k, name, "differs from the lone build")
        o = np.zeros(3)
        sga.api.check(sga.load().sga_index_origin(m.h, sga.api._dp(o)))
        assert np.array_equal(o, cloud.origin()), (label, k, o, cloud.origin())
        queries = np.concatenate([cloud.xyz64()[:3000], FAR + cloud.origin()])
        for offsets in (1, 7, 27):
            m.set_search_offsets(offsets)
            lone.set_search_offsets(offsets)
            (ia, da), (ib, db) = knn_bits(m, queries), knn_bits(lone, queries)
            assert np.array_equal(ia, ib) and np.array_equal(da, db), (label, "member", k, "search over", offsets, "voxels differs")
        m.set_search_offsets(1)
        print("%-36s member %2d n=%7d voxels=%6d largest=%5d" % (label, k, cloud.size(), m.size(), a[3].max() if len(a[3]) else 0))
        got.append(a)
    print("%-36s plan %s" % (label, plan))
    return got


# ---- the cases of the shared chain -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    sizes = [1, 63, 64, 65, 255, 256, 257, 2049]
    clouds = [cloud_of(scan(n, 10 + n)) for n in sizes]
    one_voxel = cloud_of(np.random.default_rng(5).uniform(0.05, 0.45, (300, 3)).astype(F32))  # one voxel at every leaf of the test
    g = np.arange(6, dtype=F32)
    own = cloud_of(np.stack(np.meshgrid(10 * g + 0.3, 10 * g + 0.3, 10 * g + 0.3), -1).reshape(-1, 3))  # 216 points, each in a voxel of its own
    return sizes, clouds, one_voxel, own


@pytest.mark.parametrize("leaf", [0.5, 2.0, 8.0])
def test_sizes_around_the_launch_blocks(sized, leaf):
    sizes, clouds, one_voxel, own = sized
    members = clouds + [one_voxel, own]
    got = check_batch("sizes, leaf %g" % leaf, members, leaf, {"forest": 10, "lone": 0, "empty": 0, "member_bits": 4, "end_bit": 53, "points": sum(sizes) + 300 + 216})
    assert len(got[8][3]) == 1 and got[8][3][0] == 300  # every point in one voxel
    assert len(got[9][3]) == 216 and got[9][3].max() == 1  # every point in a voxel of its own
    voxels = [len(g[3]) for g in got]
    if leaf == 0.5:
        assert voxels[7] > 1024 and voxels[4] > 128 and voxels[6] > 128 and voxels[0] == 1  # several finalize blocks, members on both sides of one block
    if leaf == 8.0:
        assert max(voxels[:8]) < 128  # members that share one finalize block with nobody: every block ends inside its member
    # every member alone and the members turned round give the same maps
    turned = check_batch("sizes turned, leaf %g" % leaf, members[::-1], leaf, {"forest": 10})
    for a, b in zip(got, turned[::-1]):
        assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(a, b))
    alone = check_batch("2049 alone, leaf %g" % leaf, [clouds[7]], leaf, {"forest": 1, "member_bits": 0, "end_bit": 49})
    assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(alone[0], got[7]))


def test_member_boundaries():
    """Two members that occupy the same voxel coordinates must not merge; the same cloud twice; a member whose last points are dropped
    beside a member whose first voxel — (0, 0, 0), the rest of it at non-negative coordinates — has the numerically next key."""
    a = scan(1500, 1)
    b = (a + np.random.default_rng(2).uniform(-0.01, 0.01, a.shape)).astype(F32)  # other points, (almost) the same voxels
    tail = scan(700, 3)
    tail[-150:] = [3e6, 1.0, 1.0]  # the last 150 points are out of the grid at a 1 m leaf
    octant = scan(900, 4, lo=(0, 0, 0), hi=(12, 12, 3))
    octant[0] = [0.5, 0.5, 0.5]
    ca, cb, ct, co = cloud_of(a), cloud_of(b), cloud_of(tail), cloud_of(octant)
    got = check_batch("member boundaries", [ca, cb, ca, ct, co, ct, ca], 1.0, {"forest": 7, "lone": 0, "member_bits": 3})
    assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(got[0], got[2])) and all(np.array_equal(raw(x), raw(y)) for x, y in zip(got[0], got[6]))
    assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(got[3], got[5]))
    assert got[3][3].sum() == 550 and got[4][3].sum() == 900 and (got[4][0] == 0).all(axis=1).any()
    assert got[0][3].sum() == 1500 and got[1][3].sum() == 1500


def test_dropped_points():
    some = scan(2000, 6)
    some[::7] = [3e6, -3e6, 0.0]  # beyond 2^20 voxels at a 1 m leaf
    gone = np.full((500, 3), 3e6, F32) + np.arange(500, dtype=F32)[:, None]
    empty = cloud_of(np.zeros((0, 3), F32))
    clouds = [cloud_of(some), cloud_of(gone), empty, cloud_of(scan(300, 7)), empty]
    got = check_batch("dropped points", clouds, 1.0, {"forest": 3, "lone": 0, "empty": 2})
    assert got[0][3].sum() == 2000 - len(some[::7]) and [len(g[3]) for g in got[1:3]] == [0, 0] and len(got[4][3]) == 0 and len(got[3][3]) > 0
    maps = sga.build_gaussian_voxelmaps([empty, empty], 1.0)  # nothing but empty members: no chain, two 16-slot tables
    assert [m.size() for m in maps] == [0, 0]
    assert api._voxelmap_batch_plan([empty, empty], 1.0) == {"forest": 0, "lone": 0, "empty": 2, "member_bits": 0, "end_bit": 0, "points": 0}
    idx, _ = maps[0].batch_knn_search(FAR, 1)
    assert (np.asarray(idx) < 0).all()


def test_negative_coordinates_and_frames():
    """A cloud straddling the origin (fast_floor on negative values, points on voxel faces included), and a geo-referenced cloud beside its
    twin at the origin: equal counts, coordinates that differ by the shift in voxels."""
    pts = scan(2500, 8, lo=(-20, -20, -6), hi=(20, 20, 6)).astype(np.float64)
    pts[:400] = np.round(pts[:400])  # on the faces of voxels (every second one at a 2 m leaf), negative ones included
    twin = cloud_of(pts.astype(F32))
    c6 = np.empty((len(pts), 6), F32)
    sga.api.check(sga.load().sga_cloud_download(twin.ctx.h, twin.h, None, None, sga.api._fp(c6)))
    geo = sga.PointCloud(pts + SHIFT, covs=c6)
    assert np.abs(geo.origin() - SHIFT).max() < 128.0 and np.abs(geo.origin()).max() > 9e5
    for leaf in (2.0, 4.0):  # (SHIFT's -2 000 000 m is inside the grid of +-2^20 voxels from a 2 m leaf on)
        got = check_batch("frames, leaf %g" % leaf, [geo, twin], leaf, {"forest": 2})
        assert (got[1][0] < 0).any() and (got[1][0] > 0).any()
        assert np.array_equal(got[0][3], got[1][3])
        assert np.array_equal(got[0][0].astype(np.int64), got[1][0] + np.round(SHIFT / leaf).astype(np.int64))


def test_key_overflow_and_fallbacks():
    """A member spanning 65536 or more voxels along an axis is within the lone key's range and beyond the batch key's: the device reports
    it, the host rebuilds it by the lone routine.  Two clusters exactly 65536 voxels apart would share every key of the batch; 70 km apart
    they would not, and are rebuilt all the same.  Members above the point cap and past the concatenation cap: the plan sends them lone."""
    cluster = scan(800, 9, lo=(0, 0, 0), hi=(30, 30, 3))
    for gap in (65536.0, 70000.0, -65536.0):
        far = cluster.copy()
        far[400:, 1] += gap
        wide = cloud_of(far)
        below = cluster.copy()
        below[400:, 0] += 65000.0  # spans fewer than 65536 voxels: stays in the chain
        got = check_batch("two clusters %g m apart" % gap, [cloud_of(scan(500, 11)), wide, cloud_of(below), wide], 1.0, {"forest": 4, "lone": 0})
        assert got[1][3].sum() == 800 and got[2][3].sum() == 800
    big = cloud_of(scan(262145, 12, lo=(-60, -60, -3), hi=(60, 60, 3)))
    most = big.slice(0, 262144)
    check_batch("above the point cap", [cloud_of(scan(400, 13)), big, cloud_of(scan(300, 14))], 1.0, {"forest": 2, "lone": 1, "points": 700})
    assert api._voxelmap_batch_plan([most], 1.0)["forest"] == 1
    plan = api._voxelmap_batch_plan([most] * 65, 1.0)  # 2^24 points fill the chain: the 65th member goes lone
    assert plan["forest"] == 64 and plan["lone"] == 1 and plan["points"] == 1 << 24 and plan["end_bit"] == 49 + 6, plan


def test_interleaving_on_one_context_and_a_member_of_another():
    """Batched and lone builds, a batched voxel grid and a batched kd-tree build (which share the box block) alternating on one context,
    blocking and stream-ordered; one member made by another context of the device."""
    ctx, other = sga.Context(0), sga.Context(0)
    raws = [sga.PointCloud(scan(6000 + 500 * k, 20 + k), ctx=ctx) for k in range(3)]
    for ordered in (False, True):
        prev = ctx.set_stream_ordered(ordered)
        prev_other = other.set_stream_ordered(ordered)
        try:
            down = sga.voxelgrid_sampling_batch(raws, 0.5)
            trees = sga.build_kdtrees(down)
            sga.estimate_covariances_batch(down, trees, 10)
            maps = sga.build_gaussian_voxelmaps(down, 1.0)
            lone = sga.GaussianVoxelMap.from_cloud(down[1], 1.0)
            down2 = sga.voxelgrid_sampling_batch(raws, 1.0)
            maps2 = sga.build_gaussian_voxelmaps(down[::-1], 2.0)
            trees2 = sga.build_kdtrees(down2)
            foreign = sga.PointCloud(scan(3000, 30), ctx=other)
            sga.estimate_covariances(foreign, None, 10)  # in flight on the other context's stream when the call below takes it
            hs = (C.c_void_p * 3)(down[0].h.value, foreign.h.value, down[2].h.value)
            out = (C.c_void_p * 3)()
            sga.api.check(sga.load().sga_index_build_gaussian_voxelmap_batch(ctx.h, hs, 3, 1.0, out))
            mixed = [sga.GaussianVoxelMap._adopt(1.0, ctx, C.c_void_p(out[k])) for k in range(3)]
            check_batch("interleaved, ordered=%s" % ordered, down, 1.0, maps=maps)
            check_batch("interleaved 2, ordered=%s" % ordered, down[::-1], 2.0, maps=maps2)
            for k, (c, m) in enumerate(zip([down[0], foreign, down[2]], mixed)):
                ref = sga.GaussianVoxelMap.from_cloud(c, 1.0)
                assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(m.download(), ref.download())), (ordered, k)
            assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(lone.download(), maps[1].download()))
            assert [t.size() for t in trees2] == [d.size() for d in down2]
            del mixed, maps, maps2, lone
        finally:
            ctx.set_stream_ordered(prev)
            other.set_stream_ordered(prev_other)
        ctx.synchronize()
        other.synchronize()


def test_launch_count_does_not_grow_with_the_batch():
    clouds = [cloud_of(scan(1500 + 100 * k, 40 + k)) for k in range(8)]
    n0 = sga.voxelmap_batch_launches()
    one = sga.build_gaussian_voxelmaps(clouds[:1], 1.0)
    n1 = sga.voxelmap_batch_launches()
    eight = sga.build_gaussian_voxelmaps(clouds, 1.0)
    n8 = sga.voxelmap_batch_launches()
    sga.GaussianVoxelMap.from_cloud(clouds[0], 1.0)
    assert sga.voxelmap_batch_launches() == n8  # the lone build counts nothing
    assert n1 - n0 == n8 - n1 and 0 < n1 - n0 <= 12, (n0, n1, n8)
    assert one[0].size() == eight[0].size() > 0


def test_argument_errors_on_a_live_device():
    lib = sga.load()
    good = cloud_of(scan(500, 50))
    bare = sga.PointCloud(scan(400, 51))  # no covariances
    ctx = good.ctx
    hs = (C.c_void_p * 3)(good.h.value, good.h.value, bare.h.value)
    before = sga.voxelmap_batch_launches()
    out = (C.c_void_p * 3)(1, 2, 3)
    assert lib.sga_index_build_gaussian_voxelmap_batch(ctx.h, hs, 3, 1.0, out) == INVALID
    assert "needs point covariances" in lib.sga_last_error().decode() and "cloud 2" in lib.sga_last_error().decode()
    assert [out[k] for k in range(3)] == [None] * 3
    for leaf in (0.0, -2.0):
        out = (C.c_void_p * 3)(1, 2, 3)
        assert lib.sga_index_build_gaussian_voxelmap_batch(ctx.h, hs, 2, leaf, out) == INVALID and "leaf size must be positive" in lib.sga_last_error().decode()
        assert [out[k] for k in range(3)] == [None, None, 3]
    with pytest.raises(sga.SgaError):
        sga.build_gaussian_voxelmaps([good, bare], 1.0)
    assert sga.voxelmap_batch_launches() == before  # refused before any device work
    check_batch("after the refusals", [good, good], 1.0, {"forest": 2})  # the context is still usable
    m = sga.build_gaussian_voxelmaps([good], 1.0)[0]
    with pytest.raises(sga.SgaError):  # a search target only
        m.insert(good)
    clone = C.c_void_p()
    sga.api.check(lib.sga_index_clone(ctx.h, m.h, C.byref(clone)))
    copy = sga.GaussianVoxelMap._adopt(1.0, ctx, clone)
    assert all(np.array_equal(raw(x), raw(y)) for x, y in zip(m.download(), copy.download()))


# ---- as targets ------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error"))


def test_align_batch_against_batch_built_maps_equals_lone_built_maps():
    tgt, src, T = sga.synthetic.registration_pair(12_000)
    targets = [cloud_of(tgt[: max(n, 2000)]) for n in SIZES]
    sources = [cloud_of(src[:n]) for n in SIZES]
    st = sga.make_setting("GICP")
    for offsets in (1, 7):
        batch_maps = sga.build_gaussian_voxelmaps(targets, 1.0)
        lone_maps = [sga.GaussianVoxelMap.from_cloud(c, 1.0) for c in targets]
        for m in batch_maps + lone_maps:
            m.set_search_offsets(offsets)
        a = sga.align_batch(batch_maps, sources, [T] * len(SIZES), st)
        b = sga.align_batch(lone_maps, sources, [T] * len(SIZES), st)
        for k in range(len(SIZES)):
            assert _same(a[k], b[k]), (offsets, k, a[k], b[k])
        assert a[-1].num_inliers > 0


def test_a_batch_built_map_matches_the_oracle(orc):
    """equal ids, coordinates and counts; means and covariances within the tolerances of
    test_gpu_parity.py::test_incremental_voxelmap_matches_oracle (fp32 export of fp64 sums over identical fp32 inputs)"""
    clouds = [cloud_of(scan(4000, 60)), cloud_of(scan(2500, 61, lo=(-9, -9, -2), hi=(9, 9, 2)))]
    maps = sga.build_gaussian_voxelmaps(clouds, 1.0)
    for cloud, m in zip(clouds, maps):
        oc_cloud = orc.Cloud(cloud.xyz().astype(np.float64), None, cloud.covs()[:, :3, :3], tree=False)
        ov = orc.VoxelMap(oc_cloud, 1.0)
        gc, gm, g6, gn = m.download()
        oc, om, ocv, on = ov.get()
        assert m.size() == len(ov) and (gc == oc).all() and (gn == on).all()
        scale = max(1.0, float(np.abs(om).max()))
        assert np.abs(gm - om).max() <= 2e-7 * scale
        assert np.abs(sga.api.mats_from_sym6(g6.astype(np.float64)) - ocv).max() <= 2e-7


# ---- the odometry driver ---------------------------------------------------------------------------------------------------------------
def test_odometry_vgicp_with_batched_and_lone_maps():
    from small_gicp_amd import odometry

    on = odometry.run_synthetic_batched(num_frames=6, batch=4, registration_type="VGICP", batched_voxelmaps=True)
    off = odometry.run_synthetic_batched(num_frames=6, batch=4, registration_type="VGICP", batched_voxelmaps=False)
    assert len(on["relative_poses"]) == 5 and on["iterations"] == off["iterations"]
    for a, b in zip(on["relative_poses"], off["relative_poses"]):
        assert np.array_equal(a, b)
    seq = odometry.run_synthetic(6)  # OnlineOdometry, kd-tree targets
    for i in range(1, 6):
        rel = np.linalg.inv(seq["estimated"][i - 1]) @ seq["estimated"][i]
        gt = np.linalg.inv(seq["ground_truth"][i - 1]) @ seq["ground_truth"][i]
        dt, dr = pose_error(on["relative_poses"][i - 1], rel)
        print("pair %d: VGICP vs the sequential GICP driver dt %.2e m dr %.2e rad; vs ground truth %.2e m" % (i, dt, dr, pose_error(on["relative_poses"][i - 1], gt)[0]))
    # the default call is the kd-tree form, unchanged: against OnlineOdometry as tests/test_batch_gpu.py compares it
    got = odometry.run_synthetic_batched(6, batch=4)
    for i in range(1, 6):
        rel = np.linalg.inv(seq["estimated"][i - 1]) @ seq["estimated"][i]
        dt, dr = pose_error(got["relative_poses"][i - 1], rel)
        assert dt < POSE_TOL_T and dr < POSE_TOL_R, (i, dt, dr)
    assert got["mean_iterations"] == seq["mean_iterations"]
    # the VGICP trajectory: every pair within the same tolerance of the registration of that pair alone against the lone-built map
    ctx = sga.Context(0)
    st = sga.make_setting("VGICP", max_correspondence_distance=1.0)
    frames = []
    for f in range(6):
        pts, _ = sga.synthetic.kitti_like_scan(f)
        cloud = sga.voxelgrid_sampling(sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=F32), ctx=ctx), 0.25)
        sga.estimate_covariances(cloud, sga.KdTree(cloud), 20)
        frames.append(cloud)
    for i in range(1, 6):
        lone = sga.Problem(sga.GaussianVoxelMap.from_cloud(frames[i - 1], 1.0), frames[i], np.eye(4), ctx=ctx).align(st, np.eye(4))
        dt, dr = pose_error(on["relative_poses"][i - 1], lone.T_target_source)
        assert dt < POSE_TOL_T and dr < POSE_TOL_R, (i, dt, dr)


# ---- the C++ header ---------------------------------------------------------------------------------------------------------------------
def test_cpp_create_gaussian_voxelmaps(tmp_path):
    """include/small_gicp_amd.hpp: create_gaussian_voxelmaps against create_gaussian_voxelmap and the lone C call, per member
    (tests/cpp/test_cpp_voxelmaps_batch.cpp, compiled with g++ as test_gpu_parity.py::test_cpp_header_layer compiles its program)."""
    exe = tmp_path / "test_cpp_voxelmaps_batch"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_voxelmaps_batch.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd", "-Wl,-rpath," + libdir,
           "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = sga.synthetic.kitti_like_scan(0)
    (tmp_path / "p.f32").write_bytes(np.ascontiguousarray(pts[:30000, :3], dtype=F32).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("MEMBER")]
    assert len(rows) == 4, p.stdout
    for tok in rows:
        print(" ".join(tok))
        assert int(tok[3]) == int(tok[4]) == int(tok[5]) > 0, tok  # voxels: batch, helper, lone
        assert tok[7] == "1" and tok[9] == "1" and tok[15] == "1", tok  # bit-equal to the lone build; coordinates and counts as the helper's; the search agrees
        assert float(tok[11]) <= 2e-7 and float(tok[13]) <= 2e-7, tok  # test_incremental_voxelmap_matches_oracle's tolerances

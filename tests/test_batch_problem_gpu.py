"""Batched problem creation (csrc/problem.hip: sga_problem_create_batch): the problems of B (target, source, pose)
triples made by one table copy, one keys launch, one stable sort, one gather / state / bounding-box launch and one host wait.

Every comparison is BIT EQUALITY against a twin made by Problem(target, source, T) on the same inputs — the engine's source order
(sorted_points, index column included), linearizations at two poses and a full align — no tolerance anywhere:
  * members at the block and tile edges, alone and eight to a call, first and last of a call;
  * kd-tree, one-shot and incremental Gaussian, flat maps with and without covariances, leaf sizes 0.5 and 2.0, in one call;
  * ties (duplicated points, a cloud inside one key cell): the order is the sort's stability;
  * a pose per member, init_T None, a geo-referenced pair;
  * shared targets, a cloud three times, inputs of a stream-ordered second context;
  * the plan, the lone fallbacks inside the call (projective target, a member over the point cap), an empty source;
  * a non-finite member; the launch count; the two odometry drivers; the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import api, odometry

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1
SIZES = [1, 63, 64, 65, 255, 256, 257, 2049, 11_003]  # one point; around a wave; around the 256-point workgroup; past the sort's 2048-item block; a C5-sized scan
SHIFT = np.array([1_000_064.0, -2_000_000.0, 128.0])  # tests/test_batch_gpu.py's: multiples of 128 m, the geo-referenced pair's origin
FIELDS = ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error")


def step(T, d):
    """T moved by a small rigid motion of size d"""
    c, s = np.cos(0.3 * d), np.sin(0.3 * d)
    D = np.eye(4)
    D[:2, :2] = [[c, -s], [s, c]]
    D[:3, 3] = [d, -0.5 * d, 0.25 * d]
    return D @ T


def conj(T, s):
    """the rigid motion T between frames both shifted by s"""
    S, Si = np.eye(4), np.eye(4)
    S[:3, 3], Si[:3, 3] = s, -s
    return S @ T @ Si


def cloud_with_covs(points, k=10, ctx=None):
    c = sga.PointCloud(points, ctx=ctx)
    sga.estimate_covariances(c, None, k)
    return c


@pytest.fixture(scope="module")
def world():
    ta, sa, T = sga.synthetic.registration_pair(20_000)
    w = type("World", (), {})()
    w.T, w.ta, w.sa = T, ta, sa
    w.tcloud = sga.PointCloud(ta)
    sga.estimate_normals_covariances(w.tcloud, None, 10)
    w.tree = sga.KdTree(w.tcloud)
    w.gauss = sga.GaussianVoxelMap.from_cloud(w.tcloud, 1.0)
    w.src = {n: cloud_with_covs(sa[:n]) for n in SIZES}
    return w


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_result(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


def assert_twin(label, pb, twin, kind, T):
    """the created problem against its lone twin: the engine's order, two linearizations, an align — the same calls on both, bit for bit"""
    a, b = pb.sorted_points(), twin.sorted_points()
    assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), (label, "order")
    st = sga.make_setting(kind)
    for pose in (T, step(T, 0.02)):
        ra, rb = pb.linearize(st.factor, pose), twin.linearize(st.factor, pose)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(ra, rb)), (label, "linearize", ra[2:], rb[2:])
    assert same_result(pb.align(st, T), twin.align(st, T)), (label, "align")


def check_call(label, targets, sources, Ts, kinds, ctx=None):
    pbs = sga.create_problems(targets, sources, Ts, ctx=ctx)
    assert len(pbs) == len(targets)
    for k, pb in enumerate(pbs):
        T = np.eye(4) if Ts is None else Ts[k]
        assert_twin("%s member %d" % (label, k), pb, sga.Problem(targets[k], sources[k], T, ctx=ctx), kinds[k], T)
    return pbs


def target_of(w, k):
    return (w.tree, "GICP") if k % 2 == 0 else (w.gauss, "GICP")


@pytest.mark.parametrize("B", [1, 8])
def test_block_and_tile_edges(world, B):
    w = world
    if B == 1:
        groups = [[n] for n in SIZES]
    else:
        groups = [SIZES[:8], SIZES[1:]]  # eight members a call; the second holds the C5-sized one
    for g in groups:
        tk = [target_of(w, SIZES.index(n)) for n in g]
        Ts = [step(w.T, 0.01 * j) for j in range(len(g))]
        plan = api._problem_batch_plan([t for t, _ in tk], [w.src[n] for n in g])
        assert plan == {"forest": len(g), "lone": 0, "empty": 0, "points": sum(g)}
        check_call("B=%d %s" % (B, g), [t for t, _ in tk], [w.src[n] for n in g], Ts, [k for _, k in tk])


def test_first_and_last_of_a_call_give_the_same_bits(world):
    w = world
    others = [257, 64, 2049, 1, 255]
    for tgt in (w.tree, w.gauss):
        orders = []
        for pos in (0, len(others)):
            ns = list(others)
            ns.insert(pos, 11_003)
            Ts = [step(w.T, 0.03) if n == 11_003 else w.T for n in ns]
            pbs = sga.create_problems([tgt] * len(ns), [w.src[n] for n in ns], Ts)
            orders.append(pbs[pos].sorted_points())
            assert_twin("pos %d" % pos, pbs[pos], sga.Problem(tgt, w.src[11_003], step(w.T, 0.03)), "GICP", step(w.T, 0.03))
        assert np.array_equal(bits(orders[0]), bits(orders[1]))


def test_kinds_in_one_call_and_batches_over_them(world):
    w = world
    inc = sga.GaussianVoxelMap(1.0)
    inc.insert(w.tcloud)
    flat, flat_cov = sga.IncrementalVoxelMap(0.5), sga.IncrementalVoxelMapCov(2.0)
    flat.insert(w.tcloud)
    flat_cov.insert(w.tcloud)
    members = [  # (target, factor downstream, family for the batch)
        (w.tree, "ICP", "kd"), (w.tree, "PLANE_ICP", "kd"), (w.tree, "GICP", "kd"),
        (w.gauss, "GICP", "gauss"), (inc, "GICP", "gauss"), (sga.GaussianVoxelMap.from_cloud(w.tcloud, 0.5), "GICP", "gauss"), (sga.GaussianVoxelMap.from_cloud(w.tcloud, 2.0), "GICP", "gauss"),
        (flat, "ICP", "flat"), (flat_cov, "GICP", "flatcov"),
    ]
    sizes = [2049, 257, 11_003, 2049, 255, 65, 11_003, 2049, 256]
    Ts = [step(w.T, 0.005 * k) for k in range(len(members))]
    targets, sources, kinds = [m[0] for m in members], [w.src[n] for n in sizes], [m[1] for m in members]
    check_call("kinds", targets, sources, Ts, kinds)
    # per kind: a BatchProblem over created problems against a BatchProblem over lone twins
    made = sga.create_problems(targets, sources, Ts)
    lone = [sga.Problem(t, s, T) for t, s, T in zip(targets, sources, Ts)]
    for family, kind in (("kd", "GICP"), ("gauss", "GICP"), ("flat", "ICP"), ("flatcov", "GICP")):
        idx = [k for k, m in enumerate(members) if m[2] == family]
        st = sga.make_setting(kind)
        out = []
        for pbs in (made, lone):
            bp = sga.BatchProblem([pbs[k] for k in idx])
            lin = bp.linearize(st.factor, [Ts[k] for k in idx])
            res = bp.align(st, [Ts[k] for k in idx])
            del bp
            out.append((lin, res))
        assert all(np.array_equal(x, y) for x, y in zip(out[0][0], out[1][0])), family
        assert all(same_result(a, b) for a, b in zip(out[0][1], out[1][1])), family
    with pytest.raises(sga.SgaError):  # a mix of kinds is fine for the creation; the batch still refuses it
        sga.BatchProblem([made[0], made[3]])


def test_ties_keep_the_input_order(world):
    w = world
    dup = sga.PointCloud(np.repeat(w.sa[:700], 4, axis=0), covs=np.repeat(w.src[2049].covs()[:700], 4, axis=0))  # every point four times: equal keys in every member
    wide = sga.GaussianVoxelMap.from_cloud(w.tcloud, 50.0)
    rng = np.random.default_rng(7)
    cell = cloud_with_covs(rng.uniform(1.0, 5.0, (1500, 3)).astype(np.float32))  # inside one 12.5 m key cell of the 50 m map
    pbs = check_call("ties", [w.tree, w.gauss, wide, wide], [dup, dup, cell, w.src[257]], [w.T, w.T, np.eye(4), w.T], ["GICP"] * 4)
    order = bits(pbs[2].sorted_points())[:, 3]
    assert np.array_equal(order, np.arange(1500, dtype=np.uint32))  # all keys equal: the engine's order is the input order
    for pb in pbs[:2]:  # the four copies of a point stay together in input order (their keys are equal, the sort is stable)
        idx = bits(pb.sorted_points())[:, 3].astype(np.int64).reshape(-1, 4)
        assert np.array_equal(idx[:, 0] % 4, np.zeros(len(idx), np.int64)) and np.array_equal(idx, idx[:, :1] + np.arange(4))


def test_poses_and_frames(world):
    w = world
    far = np.eye(4)
    far[:2, :2] = [[0.0, -1.0], [1.0, 0.0]]
    far[:3, 3] = [3.0, -2.0, 0.5]
    src = w.src[2049]
    for tgt in (w.tree, w.gauss):
        pbs = check_call("poses", [tgt, tgt], [src, src], [w.T, far @ w.T], ["GICP", "GICP"])
        assert not np.array_equal(bits(pbs[0].sorted_points()), bits(pbs[1].sorted_points()))  # the keys depend on the pose
        none = sga.create_problems([tgt, tgt], [src, w.src[257]])
        eye = sga.create_problems([tgt, tgt], [src, w.src[257]], [np.eye(4), np.eye(4)])
        for a, b in zip(none, eye):
            assert np.array_equal(bits(a.sorted_points()), bits(b.sorted_points()))
        check_call("identity", [tgt, tgt], [src, w.src[257]], None, ["GICP", "GICP"])
    # a geo-referenced pair beside its twin at the origin: each equals its own lone twin (the pose enters between ITS two device frames)
    n = 2049
    gt = sga.PointCloud(w.ta.astype(np.float64) + SHIFT)
    sga.estimate_normals_covariances(gt, None, 10)
    assert np.abs(gt.origin()).max() > 9e5
    gs = cloud_with_covs(w.sa[:n].astype(np.float64) + SHIFT)
    TG = conj(w.T, SHIFT)
    for far_t, near_t in ((sga.KdTree(gt), w.tree), (sga.GaussianVoxelMap.from_cloud(gt, 1.0), w.gauss)):
        pbs = check_call("geo", [far_t, near_t], [gs, w.src[n]], [TG, w.T], ["GICP", "GICP"])
        assert np.array_equal(bits(pbs[0].sorted_points())[:, 3], bits(pbs[1].sorted_points())[:, 3])  # the same records: the same order


def test_sharing(world):
    w = world
    c = w.src[2049]
    check_call("one target", [w.gauss] * 4, [w.src[63], c, w.src[256], w.src[11_003]], [w.T] * 4, ["GICP"] * 4)
    check_call("one cloud", [w.tree, w.gauss, w.tree], [c, c, c], [w.T, step(w.T, 0.05), step(w.T, 0.1)], ["GICP"] * 3)
    # inputs made on a second, stream-ordered context; the problems run on the default one
    other = sga.Context(0)
    other.set_stream_ordered(True)
    tc = sga.PointCloud(w.ta[:12_000], ctx=other)
    sga.estimate_normals_covariances(tc, None, 10)
    tree = sga.KdTree(tc)
    srcs = [cloud_with_covs(w.sa[:n], ctx=other) for n in (2049, 257)]
    check_call("second context", [tree, tree], srcs, [w.T, w.T], ["GICP", "GICP"], ctx=sga.default_context())
    other.synchronize()


def test_plan_and_fallbacks(world):
    w = world
    ring = sga.PointCloud(w.ta[:4000])
    proj = sga.ProjectiveSearch(ring, 64, 32)
    ramp = np.zeros((262_145, 3), np.float32)
    ramp[:, 0] = np.tile(np.linspace(0.0, 2.0, 5, dtype=np.float32), 52_429)
    big = sga.PointCloud(ramp)  # one point over the cap of a chain member
    empty = sga.PointCloud(np.zeros((0, 3), np.float32))
    targets = [w.tree, proj, w.tree, w.gauss, w.tree]
    sources = [w.src[257], w.src[2049], big, empty, empty]
    assert api._problem_batch_plan(targets, sources) == {"forest": 1, "lone": 2, "empty": 2, "points": 257}
    before = sga.problem_batch_launches()
    pbs = sga.create_problems(targets, sources, [w.T] * 5)
    chain = sga.problem_batch_launches() - before
    assert chain > 0
    assert_twin("chain", pbs[0], sga.Problem(w.tree, sources[0], w.T), "GICP", w.T)
    assert_twin("projective", pbs[1], sga.Problem(proj, sources[1], w.T), "ICP", w.T)
    a, b = pbs[2].sorted_points(), sga.Problem(w.tree, big, w.T).sorted_points()
    assert np.array_equal(bits(a), bits(b))
    for k in (3, 4):  # an empty source linearizes to zeros like the lone one
        st = sga.make_setting("GICP")
        H, bb, e, n = pbs[k].linearize(st.factor, w.T)
        Hl, bl, el, nl = sga.Problem(targets[k], empty, w.T).linearize(st.factor, w.T)
        assert not H.any() and not bb.any() and e == 0 and n == 0 and not Hl.any() and not bl.any() and el == 0 and nl == 0
    # only lone members: no chain at all
    before = sga.problem_batch_launches()
    sga.create_problems([proj, w.tree], [w.src[65], empty])
    assert sga.problem_batch_launches() == before


def test_non_finite_member_fails_the_whole_call(world):
    w = world
    lib = sga.load()
    bad = w.sa[:300].copy()
    bad[17, 1] = np.nan
    sources = [w.src[257], w.src[63], w.src[2049], sga.PointCloud(bad), w.src[64]]
    targets = [w.tree, w.gauss, w.tree, w.gauss, w.tree]
    ctx = sga.default_context()
    ts = (C.c_void_p * 5)(*[t.h.value for t in targets])
    ss = (C.c_void_p * 5)(*[s.h.value for s in sources])
    out = (C.c_void_p * 5)(*([7] * 5))
    assert lib.sga_problem_create_batch(ctx.h, ts, ss, None, 5, out) == INVALID
    msg = lib.sga_last_error().decode()
    assert "source cloud contains non-finite coordinates" in msg and "(problem 3)" in msg, msg
    assert list(out) == [None] * 5
    with pytest.raises(sga.SgaError, match="problem 3"):
        sga.create_problems(targets, sources)
    good = [0, 1, 2, 4]  # a following good call on the same context works
    check_call("after a refusal", [targets[k] for k in good], [sources[k] for k in good], [w.T] * 4, ["GICP"] * 4)


def test_launch_count_does_not_depend_on_the_members(world):
    w = world
    counts = []
    for ns in ([2049], [2049, 63, 257, 11_003, 1, 256, 255, 65]):
        before = sga.problem_batch_launches()
        pbs = sga.create_problems([target_of(w, k)[0] for k in range(len(ns))], [w.src[n] for n in ns], [w.T] * len(ns))
        counts.append(sga.problem_batch_launches() - before)
        del pbs
    print("chain launches for 1 and 8 members:", counts)
    assert counts[0] == counts[1] == 4  # the table copy, the keys launch, the sort, the finish launch
    before = sga.problem_batch_launches()
    sga.Problem(w.tree, w.src[2049], w.T)
    assert sga.problem_batch_launches() == before


def test_drivers_do_not_notice_the_flag():
    for run, args, kw in ((odometry.run_synthetic_batched, (9,), {"batch": 4, "registration_type": "VGICP"}), (odometry.run_synthetic_model_batched, (8,), {"streams": 4})):
        before = sga.problem_batch_launches()
        on = run(*args, batched_problems=True, **kw)
        assert sga.problem_batch_launches() > before  # the flag took the batched route
        before = sga.problem_batch_launches()
        off = run(*args, batched_problems=False, **kw)
        assert sga.problem_batch_launches() == before
        if "poses" in on:
            for a, b in zip(on["poses"], off["poses"]):
                assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
        else:
            assert len(on["relative_poses"]) == len(off["relative_poses"]) == 8
            assert all(np.array_equal(x, y) for x, y in zip(on["relative_poses"], off["relative_poses"]))
        assert on["iterations"] == off["iterations"]


def test_align_batch_goes_through_the_batched_creation(world):
    w = world
    before = sga.problem_batch_launches()
    res = sga.align_batch([w.gauss] * 3, [w.src[2049], w.src[257], w.src[11_003]], [w.T] * 3)
    assert sga.problem_batch_launches() - before == 4
    st = sga.make_setting("GICP")
    for r, n in zip(res, (2049, 257, 11_003)):
        assert same_result(r, sga.Problem(w.gauss, w.src[n], w.T).align(st, w.T))


def test_cpp_create_problems(tmp_path):
    """include/small_gicp_amd.hpp: create_problems over the C++ mirror against sga_problem_create (tests/cpp/test_cpp_problem_batch.cpp,
    compiled with g++ as test_batch_voxelmap_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_problem_batch"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_problem_batch.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = sga.synthetic.kitti_like_scan(0)
    (tmp_path / "p.f32").write_bytes(np.ascontiguousarray(pts[:30000, :3], dtype=np.float32).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("MEMBER")]
    assert len(rows) == 4, p.stdout
    for tok in rows:
        print(" ".join(tok))
        assert int(tok[3]) > 0 and tok[5] == "1", tok

"""Device-resident clouds, queries and results (csrc/cloud_io.hip, problem.hip, device_io.hip): torch tensors and device pointers in and out.

Every comparison is BIT EQUALITY with the host entry point fed the same values — no tolerance anywhere: the device path computes
fl32(double(x) - o), double(record) + o and plain casts, the host path the same expressions on the same values, and a bounding box is
a min / max (order independent).
  * clouds: n on both sides of the 256-point workgroup; float32 rows of stride 3, 4 and 8, float64 rows of stride 4; normals; covariances
    as 6, 9 and 16 columns in both dtypes; a geo-referenced cloud (origin not zero); NaN / inf rows; all-NaN rows; origin given;
    relative; n = 0.  Equal are the raw bytes of sga_cloud_download, origin() and _voxelgrid_plan(0.5) (so the record box is equal);
  * export: to_torch against xyz() / xyz64() / normals() / covs(), an `out` view of row stride 4 whose fourth column stays;
  * kNN against a kd-tree, a Gaussian and a flat map (1 / 7 / 27 offsets), a shifted and an empty index; a projective index is refused;
  * factors; a full align downstream of from_torch; the C++ mirror;
  * the ordering contract: inputs produced on a side stream without a host wait, outputs consumed on it straight away, in a blocking, a
    stream-ordered and a same-stream context.  That is COVERAGE of the contract, not a race detector: a missing wait would most likely
    pass it too;
  * refusals: error 1 with its message and no device work.  No test hands the library a pointer it would launch a kernel on and fault."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 255, 256, 257, 1000]  # on both sides of the 256-point workgroup; several workgroups
SHIFT = np.array([5e5, -3e5, 120.0])
FIELDS = ("T_target_source", "converged", "iterations", "num_inliers", "H", "b", "error")
DEV = "cuda:0"


def points(n, seed=0, shift=None, dtype=np.float32):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-20.0, 20.0, (n, 3))
    if shift is not None:
        p = p + shift
    return p.astype(dtype)


def strided(a, stride):
    """the rows of `a` as a view of a wider device tensor whose other columns hold a value that must never show up"""
    wide = torch.full((a.shape[0], stride), 7777.0, dtype=torch.from_numpy(a).dtype, device=DEV)
    wide[:, : a.shape[1]] = torch.from_numpy(a).to(DEV)
    return wide[:, : a.shape[1]]


def raw(cloud):
    """the bytes of sga_cloud_download (points, normals, cov6), the origin and the voxel-grid plan"""
    n = cloud.size()
    hn, hc = cloud._has()
    xyz, nr, c6 = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32)
    api.check(sga.load().sga_cloud_download(cloud.ctx.h, cloud.h, api._fp(xyz), api._fp(nr) if hn else None, api._fp(c6) if hc else None))
    return dict(n=n, has=(hn, hc), xyz=xyz.tobytes(), nrm=nr.tobytes(), cov=c6.tobytes(), origin=cloud.origin().tobytes(), plan=cloud._voxelgrid_plan(0.5))


def same_cloud(a, b):
    ra, rb = raw(a), raw(b)
    for key in ra:
        assert ra[key] == rb[key], key
    return True


def launch_counters():
    return (sga.forest_launches(), sga.problem_batch_launches(), sga.voxelgrid_batch_launches(), sga.voxelmap_batch_launches(), sga.voxelmap_insert_batch_launches())


def host_f64_origin(p64, origin, normals=None):
    """sga_cloud_create_f64_origin: the reference's layout (n x 4 doubles), recentred about a given origin"""
    n = len(p64)
    xyzw = np.ones((n, 4))
    xyzw[:, :3] = p64
    n4 = None
    if normals is not None:
        n4 = np.zeros((n, 4))
        n4[:, :3] = normals
    h = C.c_void_p()
    ctx = api.default_context()
    o = np.ascontiguousarray(origin, dtype=np.float64)
    api.check(sga.load().sga_cloud_create_f64_origin(ctx.h, api._dp(xyzw), api._dp(n4), None, n, api._dp(o), C.byref(h)))
    return sga.PointCloud(ctx=ctx, _handle=h)


# ---- clouds: the same bits as the host path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, stride", [(np.float32, 3), (np.float32, 4), (np.float32, 8), (np.float64, 4)])
@pytest.mark.parametrize("with_normals", [False, True])
def test_cloud_equals_the_host_upload(dtype, stride, with_normals):
    for n in SIZES:
        p = points(n, seed=n, dtype=dtype)
        nrm = points(n, seed=n + 1, dtype=dtype) / 20 if with_normals else None
        dev = sga.PointCloud.from_torch(strided(p, stride), None if nrm is None else strided(nrm, stride))
        assert same_cloud(dev, sga.PointCloud(p.copy(), None if nrm is None else nrm.copy())), n


@pytest.mark.parametrize("cols", [6, 9, 16])
@pytest.mark.parametrize("pdtype, cdtype", [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float64), (np.float64, np.float32)])
def test_covariance_layouts_equal_the_host_upload(cols, pdtype, cdtype):
    for n in SIZES:
        p = points(n, seed=3 * n, dtype=pdtype)
        rng = np.random.default_rng(n)
        m = rng.uniform(-1.0, 1.0, (n, cols)).astype(cdtype)  # NOT symmetric: which six entries are taken shows
        if cols == 6:
            host, t = m.copy(), strided(m, 7)
        else:
            d = 3 if cols == 9 else 4
            host = m.reshape(n, d, d).copy()
            t = torch.from_numpy(m).to(DEV).reshape(n, d, d)
            if cols == 16:  # the Python host path reads [0,0] [0,1] [0,2] [1,1] [1,2] [2,2]: entries 0, 1, 2, 5, 6, 10 of the 4x4
                assert np.array_equal(api.sym6_from_mats(host), m[:, [0, 1, 2, 5, 6, 10]])
        dev = sga.PointCloud.from_torch(torch.from_numpy(p).to(DEV), covs=t)
        assert same_cloud(dev, sga.PointCloud(p.copy(), covs=host)), n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_geo_referenced_cloud(dtype):
    for n in SIZES:
        p = points(n, seed=n, shift=SHIFT, dtype=dtype)
        dev = sga.PointCloud.from_torch(strided(p, 4))
        assert dev.origin().any()
        assert same_cloud(dev, sga.PointCloud(p.copy())), n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shift", [None, SHIFT])
def test_non_finite_rows(dtype, shift):
    for n in (257, 1000):
        p = points(n, seed=n, shift=shift, dtype=dtype)
        p[5] = np.nan
        p[256, 1] = np.inf
        p[100, 2] = -np.inf
        p[n - 1, 0] = np.nan
        dev = sga.PointCloud.from_torch(torch.from_numpy(p).to(DEV))
        assert same_cloud(dev, sga.PointCloud(p.copy())), n
        assert raw(dev)["plan"]["box"]  # the box of the finite coordinates
    allnan = np.full((300, 3), np.nan, dtype)
    dev = sga.PointCloud.from_torch(torch.from_numpy(allnan).to(DEV))
    assert not dev.origin().any() and not raw(dev)["plan"]["box"]
    assert same_cloud(dev, sga.PointCloud(allnan.copy()))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_origin_given(dtype):
    """absolute coordinates recentred about the caller's origin: sga_cloud_create_f64_origin on the same values"""
    origin = np.array([499_968.0, -300_032.0, 128.0])
    for n in SIZES:
        p = points(n, seed=n, shift=SHIFT, dtype=dtype)
        nrm = points(n, seed=n + 1, dtype=dtype) / 20
        dev = sga.PointCloud.from_torch(strided(p, 4), strided(nrm, 5), origin=origin)
        assert np.array_equal(dev.origin(), origin)
        assert same_cloud(dev, host_f64_origin(p.astype(np.float64), origin, nrm.astype(np.float64))), n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_relative(dtype):
    """the records as they are, about the caller's origin: sga_cloud_create_f32_origin"""
    origin = np.array([499_968.0, -300_032.0, 128.0])
    ctx = api.default_context()
    for n in SIZES:
        rel = points(n, seed=n, dtype=dtype)
        dev = sga.PointCloud.from_torch(strided(rel, 4), origin=origin, relative=True)
        h = C.c_void_p()
        rel32 = np.ascontiguousarray(rel, dtype=np.float32)
        api.check(sga.load().sga_cloud_create_f32_origin(ctx.h, api._fp(rel32), None, None, n, api._dp(origin), C.byref(h)))
        assert same_cloud(dev, sga.PointCloud(ctx=ctx, _handle=h)), n
    with pytest.raises(ValueError):
        sga.PointCloud.from_torch(strided(rel, 4), relative=True)


def test_an_empty_tensor_gives_an_empty_cloud():
    dev = sga.PointCloud.from_torch(torch.zeros((0, 3), device=DEV))
    assert dev.size() == 0 and dev.empty() and dev.to_torch().shape == (0, 3)


def test_from_device_pointer():
    p = points(1000, seed=9, shift=SHIFT, dtype=np.float64)
    xyzw = np.ones((1000, 4))
    xyzw[:, :3] = p
    t = torch.from_numpy(xyzw).to(DEV)
    torch.cuda.synchronize()
    dev = sga.PointCloud.from_device_pointer(t.data_ptr(), 1000, dtype=np.float64, stride=4)
    assert same_cloud(dev, sga.PointCloud(p.copy()))


# ---- export ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [None, SHIFT])
def test_to_torch_equals_the_downloads(shift):
    for n in (1, 257, 1000):
        p = points(n, seed=n, shift=shift, dtype=np.float64)
        cloud = sga.PointCloud(p, normals=points(n, seed=1) / 20, covs=np.random.default_rng(n).uniform(-1, 1, (n, 6)).astype(np.float32))
        x32, n32, c32 = cloud.to_torch(True, True, True)
        assert x32.cpu().numpy().tobytes() == cloud.xyz().tobytes()
        assert n32.cpu().numpy().astype(np.float64).tobytes() == cloud.normals()[:, :3].copy().tobytes()
        assert api.mats_from_sym6(c32.cpu().numpy().astype(np.float64)).tobytes() == cloud.covs()[:, :3, :3].copy().tobytes()
        x64, n64, c64 = cloud.to_torch(True, True, True, dtype=torch.float64)
        assert x64.cpu().numpy().tobytes() == cloud.xyz64().tobytes()
        assert n64.cpu().numpy().tobytes() == cloud.normals()[:, :3].copy().tobytes()
        assert api.mats_from_sym6(c64.cpu().numpy()).tobytes() == cloud.covs()[:, :3, :3].copy().tobytes()
        wide = torch.full((n, 4), 7777.0, device=DEV)
        assert cloud.to_torch(out=wide[:, :3]) is not None
        w = wide.cpu().numpy()
        assert w[:, :3].copy().tobytes() == cloud.xyz().tobytes() and (w[:, 3] == 7777.0).all()


def test_export_matrix_layouts():
    """covariance rows as 3x3 and 4x4 through the C call: the symmetric matrix, the fourth row and column zero"""
    n = 300
    c6 = np.random.default_rng(4).uniform(-1, 1, (n, 6)).astype(np.float32)
    cloud = sga.PointCloud(points(n), covs=c6)
    full = api.mats_from_sym6(c6)
    for cols in (9, 16):
        t = torch.full((n, cols + 1), 7777.0, device=DEV)
        a = api._device_array(t.data_ptr(), _lib.F32, cols, cols + 1)
        api.check(sga.load().sga_cloud_export_device(cloud.ctx.h, cloud.h, None, None, C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream), 0))
        got = t.cpu().numpy()
        assert (got[:, cols] == 7777.0).all()
        d = 3 if cols == 9 else 4
        want = np.zeros((n, d, d), np.float32)
        want[:, :3, :3] = full
        assert got[:, :cols].copy().tobytes() == want.tobytes()


# ---- kNN ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def indices():
    w = type("W", (), {})()
    w.p = points(1000, seed=11)
    cloud = sga.PointCloud(w.p)
    sga.estimate_covariances(cloud, None, 10)
    w.tree = sga.KdTree(cloud)
    w.gauss = sga.GaussianVoxelMap(2.0)
    w.gauss.insert(cloud)
    w.flat = api.IncrementalVoxelMapCov(2.0)
    w.flat.insert(cloud)
    w.ps = points(1000, seed=11, shift=SHIFT, dtype=np.float64)
    far = sga.PointCloud(w.ps)
    sga.estimate_covariances(far, None, 10)
    w.tree_far = sga.KdTree(far)
    w.gauss_far = sga.GaussianVoxelMap(2.0)
    w.gauss_far.insert(far)
    w.keep = [cloud, far]
    return w


def host_knn(index, q32, k, max_sq=-1.0):
    """sga_index_knn on host float queries: the float32 distances the device form must reproduce bit for bit"""
    q32 = np.ascontiguousarray(q32, dtype=np.float32)
    idx = np.empty((len(q32), k), np.int64)
    d2 = np.empty((len(q32), k), np.float32)
    api.check(sga.load().sga_index_knn(index.ctx.h, index.h, api._fp(q32), len(q32), k, float(max_sq), idx.ctypes.data_as(C.POINTER(C.c_int64)), api._fp(d2)))
    return idx, d2


def check_knn(index, q32, k, dtype, stride, max_sq=-1.0):
    """q32: float32 values; handed to the device as `dtype` (a float32 value widened to double is the same number, so both sides search
    the same fl32(double(q) - origin))"""
    t = strided(q32.astype(dtype), stride)
    idx, d2 = index.batch_knn_search_torch(t, k, max_sq)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.shape == d2.shape == (len(q32), k)
    hi, hd = host_knn(index, q32, k, max_sq)
    assert idx.cpu().numpy().tobytes() == hi.tobytes()
    assert d2.cpu().numpy().tobytes() == hd.tobytes()
    bi, bd = index.batch_knn_search(q32.astype(np.float64), k, max_sq)
    assert np.array_equal(idx.cpu().numpy(), bi)
    return idx


@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("dtype, stride", [(np.float32, 3), (np.float32, 4), (np.float64, 3), (np.float64, 4)])
def test_knn_kdtree(indices, k, dtype, stride):
    for m in (1, 255, 256, 257):
        q = points(m, seed=100 + m)
        idx = check_knn(indices.tree, q, k, dtype, stride)
        assert (idx >= 0).all()
    check_knn(indices.tree, points(257, seed=5), k, dtype, stride, max_sq=4.0)


@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("offsets", [1, 7, 27])
def test_knn_voxel_maps(indices, k, offsets):
    for vm in (indices.gauss, indices.flat):
        vm.set_search_offsets(offsets)
        for m, dtype, stride in ((1, np.float32, 3), (255, np.float64, 4), (256, np.float32, 4), (257, np.float64, 3)):
            check_knn(vm, points(m, seed=200 + m), k, dtype, stride)
        vm.set_search_offsets(1)


@pytest.mark.parametrize("dtype, stride", [(np.float32, 4), (np.float64, 3)])
def test_knn_shifted_index(indices, dtype, stride):
    for m in (1, 257):
        q = points(m, seed=300 + m, shift=SHIFT)  # float32 values near 5e5: they resolve 0.03 m, both sides search the same roundings
        check_knn(indices.tree_far, q, 5, dtype, stride)
        check_knn(indices.gauss_far, q, 5, dtype, stride)
    # double queries that float32 cannot hold: the device subtracts the origin in double, as sga_index_knn_f64 does on the host
    q64 = points(257, seed=7, shift=SHIFT, dtype=np.float64)
    idx, _ = indices.tree_far.batch_knn_search_torch(torch.from_numpy(q64).to(DEV), 5)
    assert np.array_equal(idx.cpu().numpy(), indices.tree_far.batch_knn_search(q64, 5)[0])


def test_knn_empty_index():
    q = torch.from_numpy(points(257, seed=1)).to(DEV)
    for index in (sga.KdTree(sga.PointCloud(np.zeros((0, 3), np.float32))), sga.GaussianVoxelMap(1.0), api.IncrementalVoxelMap(1.0)):
        idx, d2 = index.batch_knn_search_torch(q, 5)
        assert (idx.cpu().numpy() == -1).all() and np.isposinf(d2.cpu().numpy()).all()
        hi, hd = host_knn(index, q.cpu().numpy(), 5)
        assert idx.cpu().numpy().tobytes() == hi.tobytes() and d2.cpu().numpy().tobytes() == hd.tobytes()


def test_knn_refusals(indices):
    q = torch.from_numpy(points(64, seed=1)).to(DEV)
    before = launch_counters()
    proj = sga.ProjectiveSearch(sga.PointCloud(points(500, seed=2)), 64, 32)
    a, _ = api._torch_rows(q, "queries", proj.ctx, (3,))
    out_i, out_d = torch.empty((64, 1), dtype=torch.int64, device=DEV), torch.empty((64, 1), device=DEV)
    rc = sga.load().sga_index_knn_device(proj.ctx.h, proj.h, C.byref(a), 64, 1, -1.0, C.c_void_p(out_i.data_ptr()), C.c_void_p(out_d.data_ptr()), None, 0)
    assert rc == 4 and "projective" in sga.load().sga_last_error().decode()
    with pytest.raises(sga.SgaError, match="error 1: k must be <= 116"):
        indices.tree.batch_knn_search_torch(q, 117)
    with pytest.raises(sga.SgaError, match=r"error 1: k must be in \[1,128\]"):
        indices.gauss.batch_knn_search_torch(q, 129)
    # queries claimed to be 2^28 rows: past any allocation
    rc = sga.load().sga_index_knn_device(indices.tree.ctx.h, indices.tree.h, C.byref(a), 1 << 28, 1, -1.0, C.c_void_p(out_i.data_ptr()), C.c_void_p(out_d.data_ptr()), None, 0)
    assert rc == 1 and "past its allocation" in sga.load().sga_last_error().decode()
    assert launch_counters() == before


# ---- factors, downstream --------------------------------------------------------------------------------------------------------------
def test_factors_torch():
    ta, sa, T = sga.synthetic.registration_pair(1000)
    tgt, tree = sga.preprocess_points(ta, 0.25, 10)
    src, _ = sga.preprocess_points(sa, 0.25, 10)
    pb = sga.Problem(tree, src, T)
    pb.linearize(sga.make_setting("GICP").factor, T)
    ti, m6 = pb.factors_torch()
    hi, hm = pb.factors()
    assert (hi >= 0).any() and np.abs(hm).max() > 0
    assert ti.cpu().numpy().tobytes() == hi.tobytes() and m6.cpu().numpy().tobytes() == hm.tobytes()


def test_align_downstream_of_from_torch(c1_f32):
    def run(make):
        tgt, src = make(c1_f32["tp"]), make(c1_f32["sp"])
        tree = sga.KdTree(tgt)
        sga.estimate_normals_covariances(tgt, tree, 10)
        sga.estimate_covariances(src, None, 10)
        return sga.align(tgt, src, tree), tgt, src

    rd, td, sd = run(lambda a: sga.PointCloud.from_torch(torch.from_numpy(a).to(DEV)))
    rh, th, sh = run(lambda a: sga.PointCloud(a.copy()))
    assert same_cloud(td, th) and same_cloud(sd, sh)
    for f in FIELDS:
        assert np.asarray(getattr(rd, f)).tobytes() == np.asarray(getattr(rh, f)).tobytes(), f
    assert rd.converged and rd.num_inliers > 0


# ---- the ordering contract ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["blocking", "stream_ordered", "same_stream"])
def test_ordering_with_a_side_stream(mode):
    """coverage of the contract (see the module docstring): the values are right when producer and consumer never wait on the host"""
    side = torch.cuda.Stream(device=DEV)
    ctx = sga.Context(0, stream=side.cuda_stream) if mode == "same_stream" else sga.Context(0)
    if mode == "stream_ordered":
        ctx.set_stream_ordered(True)
    base = points(100_000, seed=21, shift=SHIFT)
    dbase = torch.from_numpy(base).to(DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        t = dbase
        for _ in range(8):  # exact in float32 whatever the device fuses: x * 2 - x is x
            t = t * 2.0 - dbase
        t = t * 0.5 + 16.0
        cloud = sga.PointCloud.from_torch(t, ctx=ctx, stream=side.cuda_stream)
        del t  # the block goes back to torch's allocator, which may hand it out again on this stream
        back = cloud.to_torch(stream=side.cuda_stream)
        used = back * 2.0
    side.synchronize()
    want = base * np.float32(0.5) + np.float32(16.0)
    host = sga.PointCloud(want, ctx=ctx)
    assert same_cloud(cloud, host)
    assert back.cpu().numpy().tobytes() == host.xyz().tobytes()
    assert used.cpu().numpy().tobytes() == (host.xyz() * np.float32(2.0)).tobytes()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_do_no_device_work(c1_raw):
    lib = sga.load()
    ctx = api.default_context()
    before = launch_counters()
    host = points(64)
    with pytest.raises(sga.SgaError, match="error 1: .*sga_cloud_create_f32"):
        sga.PointCloud.from_device_pointer(host.ctypes.data, 64)  # a numpy array's pointer
    pinned = api.pinned_copy(host)
    with pytest.raises(sga.SgaError, match="error 1: .*host memory.*sga_cloud_create_f32"):
        sga.PointCloud.from_device_pointer(pinned.ctypes.data, 64)  # sga_host_alloc memory
    with pytest.raises(sga.SgaError, match="error 1: .*sga_cloud_create_f64"):
        sga.PointCloud.from_device_pointer(host.ctypes.data, 16, dtype=np.float64, stride=4)
    t = torch.from_numpy(host).to(DEV)
    torch.cuda.synchronize()
    with pytest.raises(sga.SgaError, match="error 1: .*past its allocation"):
        sga.PointCloud.from_device_pointer(t.data_ptr(), 1 << 28)  # 64 rows claimed as 2^28
    with pytest.raises(sga.SgaError, match="error 1: .*stride 2 < cols 3"):
        sga.PointCloud.from_device_pointer(t.data_ptr(), 64, stride=2)
    cloud = sga.PointCloud(host)
    with pytest.raises(sga.SgaError, match="error 1: cloud has no covariances"):
        cloud.to_torch(covs=True)
    with pytest.raises(sga.SgaError, match="error 1: cloud has no normals"):
        cloud.to_torch(normals=True)
    h = C.c_void_p()
    rc = lib.sga_cloud_create_f32(ctx.h, C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_float)), None, None, 64, C.byref(h))
    assert rc == 1 and "sga_cloud_create_device" in lib.sga_last_error().decode() and not h.value
    assert launch_counters() == before
    # the context is as good as before: C1 registers
    tgt, src, T_gt = c1_raw
    res = sga.align(tgt, src)
    E = np.linalg.inv(res.T_target_source) @ T_gt
    assert res.converged and np.linalg.norm(E[:3, 3]) < 0.05


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------------
def test_cpp_device_io(tmp_path):
    """include/small_gicp_amd.hpp: PointCloud::from_device / export_device / knn_device over hipMalloc'd memory
    (tests/cpp/test_cpp_device_io.cpp, compiled as tests/test_batch_problem_gpu.py compiles its program, plus the ROCm paths)."""
    exe = tmp_path / "test_cpp_device_io"
    libdir = os.path.dirname(sga.LIB_PATH)
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = ["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_device_io.cpp"), "-o", str(exe),
           "-L" + libdir, "-lsmall_gicp_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath," + os.path.join(rocm, "lib")]
    subprocess.check_call(cmd)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("EQUAL")]
    assert len(rows) == 5, p.stdout
    assert all(tok[2] == "1" for tok in rows), p.stdout

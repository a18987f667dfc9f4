"""Every way of making and reading a cloud (csrc/cloud_io.hip; slices: csrc/cloud_crop.hip) against a NumPy fp64 restatement written here.

The host and the device entry points share one pack and one unpack kernel, so "device equals host" (tests/test_device_io_gpu.py) compares
a kernel with itself; this file says what the bytes must BE.  Every step is one correctly rounded IEEE operation (a widening, one
subtraction or addition in double, one rounding to float), so every comparison is of bytes, with no tolerance:
  origin     per axis 128 * rint(0.5 * (lo + hi) / 128) over the finite input coordinates widened to double, 0 for an axis without one;
             the given origin when one is passed
  records    fl32(double(x) - origin); fl32(x) for origin 0 and for relative input
  normals    fl32(v);  covariances: fl32 of entries (0,1,2,3,4,5) / (0,1,2,4,5,8) / (0,1,2,5,6,10) of 6 / 9 / 16 columns (inputs NOT symmetric)
  downloads  sga_cloud_download: the records for origin 0, else fl32(double(record) + origin); sga_cloud_download_f64: double(record) + origin;
             to_torch / sga_cloud_export_device: the same rules, covariances as 6, 9 and 16 columns, the padding of wider rows untouched
Inputs: n on both sides of the 256-point workgroup and several workgroups; uniform points in +-20 m; the same shifted by (5e5, -3e5, 120)
(a non-zero origin: the second pass of the uploads that learn their origin from the kernel); NaN / +-inf rows.
Forms: pageable and pinned fp32 arrays, sga_cloud_create_f32_origin, sga_cloud_create_f64, sga_cloud_create_f64_origin, from_torch of float
and double rows at strides 3, 4, 9 (the LDS tile of load_rows holds fewer than 256 rows: its staging loop runs more than once) and 2049
(wider than the tile: rows are read in place), normals at stride 9, covariances of 6 columns at stride 2049."""
import ctypes as C

import numpy as np
import pytest
import torch

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

pytestmark = pytest.mark.gpu

SIZES = [1, 255, 256, 257, 1000]
SHIFT = np.array([5e5, -3e5, 120.0])
DEV = "cuda:0"
COV_SEL = {6: [0, 1, 2, 3, 4, 5], 9: [0, 1, 2, 4, 5, 8], 16: [0, 1, 2, 5, 6, 10]}
SENTINEL = 7777.0


def inputs(n, dtype):
    """(name, points) of n points: uniform, shifted, and for n > 256 the shifted ones with non-finite rows"""
    rng = np.random.default_rng(n)
    base = rng.uniform(-20.0, 20.0, (n, 3))
    out = [("uniform", base.astype(dtype)), ("shifted", (base + SHIFT).astype(dtype))]
    if n > 256:
        p = (base + SHIFT).astype(dtype)
        p[5] = np.nan
        p[256, 1] = np.inf
        p[100, 2] = -np.inf
        p[n - 1, 0] = np.nan
        out.append(("non-finite", p))
    return out


def attributes(n, dtype, cols=6):
    rng = np.random.default_rng(7 * n + cols)
    return (rng.uniform(-1.0, 1.0, (n, 3))).astype(dtype), rng.uniform(-1.0, 1.0, (n, cols)).astype(dtype)


def strided(a, stride):
    """the rows of `a` as a view of a wider device tensor whose other columns hold a value that must never show up"""
    wide = torch.full((a.shape[0], stride), SENTINEL, dtype=torch.from_numpy(a).dtype, device=DEV)
    wide[:, : a.shape[1]] = torch.from_numpy(a).to(DEV)
    return wide[:, : a.shape[1]]


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def want_origin(x):
    x = x.astype(np.float64)
    o = np.zeros(3)
    for k in range(3):
        fin = x[np.isfinite(x[:, k]), k]
        if fin.size:
            o[k] = 128.0 * np.rint(0.5 * (fin.min() + fin.max()) / 128.0)
    return o


def want_records(x, origin, relative=False):
    if relative or not origin.any():
        return x.astype(np.float32)
    with np.errstate(invalid="ignore"):
        return (x.astype(np.float64) - origin).astype(np.float32)


def check_cloud(cloud, x, what, origin=None, relative=False, normals=None, covs=None):
    """cloud was made from points x (and normals, covariance rows): its origin, and every download and export, byte for byte"""
    n = len(x)
    o = want_origin(x) if origin is None else np.asarray(origin, np.float64)
    rec = want_records(x, o, relative)
    assert cloud.size() == n, what
    assert np.array_equal(cloud.origin(), o), (what, cloud.origin(), o)
    assert cloud._has() == (normals is not None, covs is not None), what
    with np.errstate(invalid="ignore"):
        x64 = rec.astype(np.float64) + o
    x32 = x64.astype(np.float32) if o.any() else rec
    lib = sga.load()
    g32, gn, gc = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 6), np.float32)
    api.check(lib.sga_cloud_download(cloud.ctx.h, cloud.h, api._fp(g32), api._fp(gn) if normals is not None else None, api._fp(gc) if covs is not None else None))
    assert g32.tobytes() == x32.tobytes(), (what, "sga_cloud_download")
    assert cloud.xyz64().tobytes() == x64.tobytes(), (what, "sga_cloud_download_f64")
    t32 = cloud.to_torch()
    t64 = cloud.to_torch(dtype=torch.float64)
    assert t32.cpu().numpy().tobytes() == x32.tobytes(), (what, "to_torch float32")
    assert t64.cpu().numpy().tobytes() == x64.tobytes(), (what, "to_torch float64")
    if normals is not None:
        wn = normals.astype(np.float32)
        assert gn.tobytes() == wn.tobytes(), (what, "normals")
        assert cloud.to_torch(False, True).cpu().numpy().tobytes() == wn.tobytes(), (what, "to_torch normals")
        assert cloud.to_torch(False, True, dtype=torch.float64).cpu().numpy().tobytes() == wn.astype(np.float64).tobytes(), (what, "to_torch normals float64")
    if covs is not None:
        wc = np.ascontiguousarray(covs[:, COV_SEL[covs.shape[1]]]).astype(np.float32)
        assert gc.tobytes() == wc.tobytes(), (what, "covariances")
        assert cloud.to_torch(False, False, True).cpu().numpy().tobytes() == wc.tobytes(), (what, "to_torch covs")
        assert cloud.to_torch(False, False, True, dtype=torch.float64).cpu().numpy().tobytes() == wc.astype(np.float64).tobytes(), (what, "to_torch covs float64")


# ---- host arrays ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("memory", ["pageable", "pinned"])
@pytest.mark.parametrize("attrs", [False, True])
def test_host_fp32(memory, attrs):
    place = api.pinned_copy if memory == "pinned" else (lambda a: a.copy())
    for n in SIZES:
        nrm, cov = attributes(n, np.float32) if attrs else (None, None)
        for name, x in inputs(n, np.float32):
            cloud = sga.PointCloud(place(x), None if nrm is None else place(nrm), None if cov is None else place(cov))
            check_cloud(cloud, x, (memory, n, name), normals=nrm, covs=cov)


def test_host_fp32_relative_to_an_origin():
    """sga_cloud_create_f32_origin: the records are the input as it is"""
    origin = np.array([499_968.0, -300_032.0, 128.0])
    ctx = api.default_context()
    for n in SIZES:
        nrm, cov = attributes(n, np.float32)
        for place in (lambda a: a.copy(), api.pinned_copy):
            x = place(inputs(n, np.float32)[0][1])
            pn, pc = place(nrm), place(cov)
            h = C.c_void_p()
            api.check(sga.load().sga_cloud_create_f32_origin(ctx.h, api._fp(x), api._fp(pn), api._fp(pc), n, api._dp(origin), C.byref(h)))
            check_cloud(sga.PointCloud(ctx=ctx, _handle=h), x, ("f32_origin", n), origin=origin, relative=True, normals=nrm, covs=cov)


@pytest.mark.parametrize("given", [False, True])
def test_host_fp64(given):
    """sga_cloud_create_f64 / sga_cloud_create_f64_origin: the reference's layout, n x 4 doubles, normals n x 4, covariances 4 x 4"""
    origin = np.array([499_968.0, -300_032.0, 128.0]) if given else None
    ctx = api.default_context()
    lib = sga.load()
    for n in SIZES:
        nrm, cov = attributes(n, np.float64, 16)
        n4 = np.full((n, 4), SENTINEL)
        n4[:, :3] = nrm
        for name, x in inputs(n, np.float64):
            xyzw = np.full((n, 4), SENTINEL)
            xyzw[:, :3] = x
            h = C.c_void_p()
            if given:
                api.check(lib.sga_cloud_create_f64_origin(ctx.h, api._dp(xyzw), api._dp(n4), api._dp(cov), n, api._dp(origin), C.byref(h)))
            else:
                api.check(lib.sga_cloud_create_f64(ctx.h, api._dp(xyzw), api._dp(n4), api._dp(cov), n, C.byref(h)))
            check_cloud(sga.PointCloud(ctx=ctx, _handle=h), x, ("f64", given, n, name), origin=origin, normals=nrm, covs=cov)


# ---- device tensors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("stride", [3, 4, 9, 2049])
def test_from_torch(dtype, stride):
    for n in SIZES:
        for name, x in inputs(n, dtype):
            check_cloud(sga.PointCloud.from_torch(strided(x, stride)), x, ("from_torch", n, name))


@pytest.mark.parametrize("pdtype, adtype", [(np.float32, np.float32), (np.float64, np.float64), (np.float32, np.float64), (np.float64, np.float32)])
def test_from_torch_wide_attributes(pdtype, adtype):
    """normals at stride 9, covariances of 6 columns at stride 2049; the origin chosen, given, and the input relative to it"""
    origin = np.array([499_968.0, -300_032.0, 128.0])
    for n in SIZES:
        nrm, cov = attributes(n, adtype)
        tn, tc = strided(nrm, 9), strided(cov, 2049)
        for name, x in inputs(n, pdtype):
            check_cloud(sga.PointCloud.from_torch(strided(x, 9), tn, tc), x, ("chosen", n, name), normals=nrm, covs=cov)
        x = inputs(n, pdtype)[1][1]
        check_cloud(sga.PointCloud.from_torch(strided(x, 9), tn, tc, origin=origin), x, ("given", n), origin=origin, normals=nrm, covs=cov)
        x = inputs(n, pdtype)[0][1]
        check_cloud(sga.PointCloud.from_torch(strided(x, 4), tn, tc, origin=origin, relative=True), x, ("relative", n), origin=origin, relative=True, normals=nrm, covs=cov)


@pytest.mark.parametrize("cols", [9, 16])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_from_torch_matrix_covariances(cols, dtype):
    for n in SIZES:
        _, cov = attributes(n, dtype, cols)
        x = inputs(n, np.float32)[0][1]
        check_cloud(sga.PointCloud.from_torch(torch.from_numpy(x).to(DEV), covs=strided(cov, cols + 1)), x, ("covs", cols, n), covs=cov)


# ---- exports into wider rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdtype, code", [(torch.float32, _lib.F32), (torch.float64, _lib.F64)])
def test_export_layouts(tdtype, code):
    """points and normals into rows of stride 4, covariances as 6, 9 and 16 columns into rows one element wider: what lies beyond the columns stays"""
    lib = sga.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    npdt = np.float32 if tdtype == torch.float32 else np.float64
    for n in (1, 257, 1000):
        nrm, cov = attributes(n, np.float32)
        for name, x in inputs(n, np.float32)[:2]:
            cloud = sga.PointCloud(x.copy(), nrm, cov)
            o = want_origin(x)
            x64 = want_records(x, o).astype(np.float64) + o
            want_x = x64.astype(npdt) if (o.any() or npdt == np.float64) else x
            tp, tn = torch.full((n, 4), SENTINEL, dtype=tdtype, device=DEV), torch.full((n, 4), SENTINEL, dtype=tdtype, device=DEV)
            ap, an = api._device_array(tp.data_ptr(), code, 3, 4), api._device_array(tn.data_ptr(), code, 3, 4)
            api.check(lib.sga_cloud_export_device(cloud.ctx.h, cloud.h, C.byref(ap), C.byref(an), None, stream, 0))
            gp, gn = tp.cpu().numpy(), tn.cpu().numpy()
            assert gp[:, :3].copy().tobytes() == want_x.tobytes() and (gp[:, 3] == SENTINEL).all(), (n, name)
            assert gn[:, :3].copy().tobytes() == nrm.astype(npdt).tobytes() and (gn[:, 3] == SENTINEL).all(), (n, name)
            xx, xy, xz, yy, yz, zz = (cov[:, k].astype(npdt) for k in range(6))
            zero = np.zeros(n, npdt)
            rows = {6: [xx, xy, xz, yy, yz, zz], 9: [xx, xy, xz, xy, yy, yz, xz, yz, zz], 16: [xx, xy, xz, zero, xy, yy, yz, zero, xz, yz, zz, zero, zero, zero, zero, zero]}
            for cols in (6, 9, 16):
                tc = torch.full((n, cols + 1), SENTINEL, dtype=tdtype, device=DEV)
                ac = api._device_array(tc.data_ptr(), code, cols, cols + 1)
                api.check(lib.sga_cloud_export_device(cloud.ctx.h, cloud.h, None, None, C.byref(ac), stream, 0))
                got = tc.cpu().numpy()
                assert got[:, :cols].copy().tobytes() == np.stack(rows[cols], axis=1).tobytes() and (got[:, cols] == SENTINEL).all(), (n, name, cols)

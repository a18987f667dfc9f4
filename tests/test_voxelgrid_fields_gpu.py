"""sga_voxelgrid_sampling_fields (csrc/preprocess.hip: ds_fields_kernel) against its restatement in float64
(tests/voxel_fields_ref.py).  Every call goes through run(): the output cloud must be sga_voxelgrid_sampling's on the same input, bit for
bit; counts and voxel_of must equal the restatement's and each other (bincount); MEAN columns must meet

    |out - mean| <= ulp32(max(|out|, |mean|)) / 2 + 2 (N + 2) 2^-53 max|v_i|

MIN / MAX must be equal under ==, FIRST and NEAREST bit for bit — NEAREST restated from the fp32 centroids the device itself wrote.  A
voxel whose two best squared distances differ by less than 1e-12 relative without the records being bit-identical FAILS the call's check
(check_fields); nothing is skipped.  The clouds and seeds are chosen so that none occurs — voxel_fields_ref.grouped_cloud says how and
why — and test_no_near_tie_on_the_cpu checks that without a device, with the restatement's rounded mean as the centroid.

Seeds: regimes SEEDS below (one per size); single voxels 1000 + N; edges and forms 7, 8, 9, 21, 22.

WORST_MEAN_RATIO_OBSERVED = 1.000 to three digits on an MI355X (a quotient exactly between two floats: the error is the half ulp itself)
"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api
from voxel_fields_ref import FIRST, MAX, MEAN, MIN, NEAREST, check_fields, grouped_cloud, partition_ref, reduce_ref

gpu = pytest.mark.gpu
F32 = np.float32
LEAF = 0.5
NAMES = {MEAN: "mean", MIN: "min", MAX: "max", FIRST: "first", NEAREST: "nearest"}
SEEDS = {1500: 31, 5000: 32, 200_001: 33, 262_145: 34}
FAR = np.array([256_000.0, -128_000.0, 0.0])  # 256 km away: a multiple of the 128 m quantum of the device frames
REGIMES = [(n, made, far) for n in SEEDS for made, far in ((False, False), (True, False))] + [(5000, False, True)]
OPS_A = [NEAREST, MEAN, FIRST]  # a time follows one real return, the intensity is averaged, the label is the first member's
OPS_B = [MIN, MAX, NEAREST]


def records_of(cloud):
    x = cloud.xyz64() - cloud.origin()
    r = x.astype(F32)
    assert np.array_equal(r.astype(np.float64), x, equal_nan=True), "xyz64 - origin is not the fp32 record"
    return r


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def run(label, cloud, fields, ops, leaf=LEAF, part=None):
    """One call checked against the restatement; returns (the partition, the restated columns, the outputs as numpy arrays)."""
    plain = sga.voxelgrid_sampling(cloud, leaf)
    out, red_f, counts, voxel_of = sga.voxelgrid_sampling_fields(cloud, fields, leaf, reduce=None if fields is None else [NAMES[o] for o in ops], return_counts=True, return_voxel_of=True)
    ro, rp = records_of(out), records_of(plain)
    assert ro.shape == rp.shape and np.array_equal(bits(ro), bits(rp)), (label, "the cloud differs from sga_voxelgrid_sampling's", ro.shape, rp.shape)
    assert np.array_equal(out.origin(), plain.origin()) and np.array_equal(out.origin(), cloud.origin()), label
    rec = records_of(cloud)
    if part is None:
        part = partition_ref(rec, cloud.origin(), leaf)
    assert len(part.counts) == out.size(), (label, "voxels", out.size(), "expected", len(part.counts))
    if fields is None:
        assert red_f is None
        check_fields(part, None, [], None, counts, voxel_of, label)
        return part, None, (ro, None, counts, voxel_of)
    got = red_f.numpy()
    assert red_f.dim == len(ops) and red_f.size() == out.size()
    f = fields.numpy() if isinstance(fields, sga.Features) else np.asarray(fields, dtype=F32).reshape(len(rec), -1)
    red = reduce_ref(part, f, ops, rec, ro)
    worst = check_fields(part, red, ops, got, counts, voxel_of, label)
    print("%-40s n=%7d voxels=%6d dropped=%5d largest=%4d ops=%s  MEAN error / bound %.3f" % (label, len(rec), len(part.counts), int((part.voxel_of < 0).sum()), int(part.counts.max()) if len(part.counts) else 0,
                                                                                           "".join(NAMES[o][0] if o != MEAN else "M" for o in ops), worst))
    return part, red, (ro, got, counts, voxel_of)


# ---- 2. single voxels --------------------------------------------------------------------------------------------------------------------
SINGLE_N = [1, 2, 7, 8, 9, 24, 25, 31, 32, 33, 40, 257]  # the edges of the 8-lane split and of the four-in-flight loop


def single_voxel(N, dim):
    """N points in one voxel, every record present twice (the second half of the indices repeats the first: every NEAREST is a real
    tie, which goes to the lowest index; N odd: one more record of its own), dim columns of which column 1 is all NaN and column 2
    holds one NaN."""
    rng = np.random.default_rng(1000 + N)
    half = (N + 1) // 2
    p = ((np.array([3.0, -2.0, 1.0]) + rng.uniform(0.05, 0.95, (half, 3))) * LEAF).astype(F32)
    p = np.r_[p, p[: N - half]]
    f = rng.uniform(-5.0, 5.0, (N, dim)).astype(F32)
    f[:, dim - 1] = rng.integers(0, 4, N)
    if dim >= 3:
        f[:, 1] = np.nan
        f[rng.integers(0, N), 2] = np.nan
    return p, f


@gpu
@pytest.mark.parametrize("N", SINGLE_N)
def test_single_voxel(N):
    for dim in (1, 3, 5, 32):
        p, f = single_voxel(N, dim)
        cloud = sga.PointCloud(p)
        feats = sga.Features.from_array(f, cloud.ctx)
        part = None
        for shift in range(5):  # every op on every column
            ops = [(c + shift) % 5 for c in range(dim)]
            part, red, (ro, got, counts, voxel_of) = run("single voxel N=%d dim=%d shift=%d" % (N, dim, shift), cloud, feats, ops, part=part)
            assert list(counts) == [N] and (voxel_of == 0).all()
            half = (N + 1) // 2
            for c, op in enumerate(ops):
                if op == NEAREST:  # the winner is of the first half; where it has a twin in the second, the tie was real
                    w = int(red.winner[0])
                    assert w < half and (w + half >= N or np.array_equal(bits(p[w]), bits(p[w + half])))
                if dim >= 3 and c == 1:
                    assert np.isnan(got[0, 1])  # all NaN, under every op
                if dim >= 3 and c == 2 and op in (MIN, MAX):
                    assert not np.isnan(got[0, 2]) or N == 1


# ---- 3. the regimes of the chain ---------------------------------------------------------------------------------------------------------
def regime_cloud(n, far):
    return grouped_cloud(n, SEEDS[n], LEAF, base=FAR if far else (0.0, 0.0, 0.0))


def label_of(n, made, far):
    return "n=%d %s%s" % (n, "made on the device" if made else "uploaded", ", 256 km away" if far else "")


@pytest.mark.parametrize("n, made, far", REGIMES, ids=[label_of(*r) for r in REGIMES])
def test_no_near_tie_on_the_cpu(n, made, far):
    """(no device) the seeds give no NEAREST voxel that hangs on the last bits, with the restatement's rounded mean as the centroid"""
    p, f = regime_cloud(n, far)
    rec = (p - (FAR if far else 0.0)).astype(F32)
    part = partition_ref(rec, FAR if far else np.zeros(3), LEAF)
    red = reduce_ref(part, f, OPS_A, rec, part.grid.means.astype(F32))
    assert not red.near_tie.any(), int(red.near_tie.sum())
    assert 2 not in part.counts and part.counts.max() == 300 and 4.0 < (part.counts.sum() - 300) / (len(part.counts) - 1) < 6.5
    assert (part.voxel_of < 0).sum() == n // 100


@gpu
@pytest.mark.parametrize("n, made, far", REGIMES, ids=[label_of(*r) for r in REGIMES])
def test_regime(n, made, far):
    p, f = regime_cloud(n, far)
    want = {"sort": 0 if n <= 2048 else 1 if n <= 200_000 else 2, "speculative": n <= 262_144}
    if made:  # a cloud made on the device by a stream-ordered context: no box, the reference's 63-bit keys
        ctx = sga.Context(0)
        ctx.set_stream_ordered(True)
        cloud = sga.PointCloud(p, ctx=ctx).deskewed(np.zeros(n, F32), np.zeros(6))
        want["box"] = False
    else:
        cloud = sga.PointCloud(p)
        want["box"] = True
    plan = cloud._voxelgrid_plan(LEAF)
    for key, v in want.items():
        assert plan[key] == v, (key, plan)
    if far:
        assert np.array_equal(cloud.origin(), FAR), cloud.origin()
    label = label_of(n, made, far)
    part, _, _ = run(label + " A", cloud, f, OPS_A)
    run(label + " B", cloud, f, OPS_B, part=part)
    assert part.counts.max() == 300 and (part.voxel_of < 0).sum() == n // 100
    if made:
        ctx.set_stream_ordered(False)


# ---- 4. edge inputs ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_edge_inputs():
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    out, red, counts, voxel_of = sga.voxelgrid_sampling_fields(empty, np.zeros((0, 2), F32), LEAF, reduce=["min", "nearest"], return_counts=True, return_voxel_of=True)
    assert out.size() == 0 and red.size() == 0 and red.dim == 2 and counts.shape == (0,) and voxel_of.shape == (0,)
    one = sga.PointCloud(np.array([[1.0, 2.0, 3.0]], F32))
    part, _, (ro, got, counts, voxel_of) = run("n = 1", one, np.array([[7.5, -1.0]], F32), [NEAREST, MEAN])
    assert got.tolist() == [[7.5, -1.0]] and list(counts) == [1] and list(voxel_of) == [0]
    for n in (5000, 300_000):  # below and above the speculative limit
        dropped = sga.PointCloud(np.full((n, 3), np.nan, F32))
        out, red, counts, voxel_of = sga.voxelgrid_sampling_fields(dropped, np.ones((n, 3), F32), LEAF, return_counts=True, return_voxel_of=True)
        assert out.size() == 0 and red.size() == 0 and red.dim == 3 and red.numpy().shape == (0, 3) and counts.shape == (0,)
        assert voxel_of.shape == (n,) and (voxel_of == -1).all()
    p, _ = grouped_cloud(3000, 7, LEAF)
    run("membership only", sga.PointCloud(p), None, [])
    out, red = sga.voxelgrid_sampling_fields(sga.PointCloud(p), None, LEAF)
    assert red is None and out.size() > 0


# ---- 5. the device form ------------------------------------------------------------------------------------------------------------------
@gpu
def test_device_form():
    import torch

    n = 6000
    p, f = grouped_cloud(n, 8, LEAF)
    scan = torch.from_numpy(np.c_[p.astype(F32), f[:, 1]].astype(F32)).cuda()  # N x 4: x y z intensity
    assert scan.stride(0) == 4
    cloud = sga.PointCloud.from_torch(scan[:, :3])
    host = sga.voxelgrid_sampling_fields(cloud, f[:, 1], LEAF, reduce="nearest", return_counts=True, return_voxel_of=True)
    dev = sga.voxelgrid_sampling_fields(cloud, scan[:, 3:4], LEAF, reduce="nearest", return_counts=True, return_voxel_of=True)
    assert np.array_equal(bits(records_of(dev[0])), bits(records_of(host[0])))
    assert np.array_equal(bits(dev[1].numpy()), bits(host[1].numpy())) and dev[1].numpy().shape == (host[0].size(), 1)
    assert dev[2].dtype == torch.int32 and dev[3].dtype == torch.int64 and dev[2].is_cuda and dev[3].is_cuda
    assert np.array_equal(dev[2].cpu().numpy(), host[2]) and np.array_equal(dev[3].cpu().numpy(), host[3])
    run("device form's input", cloud, f[:, 1], [NEAREST])
    # a double tensor: rounded to fp32 once on entry
    rng = np.random.default_rng(9)
    f64 = rng.random((n, 2)) * 1e3 + 1e-9
    assert not np.array_equal(f64, f64.astype(F32).astype(np.float64))
    host = sga.voxelgrid_sampling_fields(cloud, f64.astype(F32), LEAF, reduce=["mean", "max"], return_counts=True, return_voxel_of=True)
    dev = sga.voxelgrid_sampling_fields(cloud, torch.from_numpy(f64).cuda(), LEAF, reduce=["mean", "max"], return_counts=True, return_voxel_of=True)
    assert np.array_equal(bits(dev[1].numpy()), bits(host[1].numpy())) and np.array_equal(bits(records_of(dev[0])), bits(records_of(host[0])))
    assert np.array_equal(dev[2].cpu().numpy(), host[2]) and np.array_equal(dev[3].cpu().numpy(), host[3])
    # Features.from_torch / to_torch
    feats = sga.Features.from_torch(scan[:, 1:4])
    assert feats.size() == n and feats.dim == 3 and np.array_equal(bits(feats.numpy()), bits(scan[:, 1:4].cpu().numpy()))
    back = feats.to_torch()
    want = np.ascontiguousarray(scan[:, 1:4].cpu().numpy())  # (with the NaN coordinates of the dropped points: compared as bits)
    assert back.dtype == torch.float32 and back.is_cuda and back.shape == (n, 3) and np.array_equal(bits(back.cpu().numpy()), bits(want))
    back64 = feats.to_torch(dtype=torch.float64)
    assert back64.dtype == torch.float64 and np.array_equal(bits(back64.cpu().numpy()), bits(want.astype(np.float64)))
    f64t = torch.from_numpy(f64).cuda()
    assert np.array_equal(bits(sga.Features.from_torch(f64t).numpy()), bits(f64.astype(F32)))
    assert sga.Features.from_torch(scan[:, 3]).numpy().shape == (n, 1)


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------
@gpu
def test_two_calls_give_the_same_bytes():
    p, f = grouped_cloud(20_000, 21, LEAF)
    cloud = sga.PointCloud(p)
    f5 = np.c_[f, f[:, :2]].astype(F32)
    a = sga.voxelgrid_sampling_fields(cloud, f5, LEAF, reduce=["mean", "min", "max", "first", "nearest"], return_counts=True, return_voxel_of=True)
    b = sga.voxelgrid_sampling_fields(cloud, f5, LEAF, reduce=["mean", "min", "max", "first", "nearest"], return_counts=True, return_voxel_of=True)
    assert np.array_equal(bits(records_of(a[0])), bits(records_of(b[0]))) and np.array_equal(bits(a[1].numpy()), bits(b[1].numpy()))
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- 7. refusals with live handles -------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_with_live_handles():
    import torch

    n = 1000
    p, f = grouped_cloud(n, 22, LEAF)
    cloud = sga.PointCloud(p)
    before = sga.voxelgrid_fields_launches()
    with pytest.raises(sga.SgaError, match="fields have 999 rows, the cloud has 1000 points"):
        sga.voxelgrid_sampling_fields(cloud, sga.Features.from_array(f[:999], cloud.ctx), LEAF)
    with pytest.raises(sga.SgaError, match=r"dim must be in \[1,32\], got 33"):
        sga.voxelgrid_sampling_fields(cloud, np.zeros((n, 33), F32), LEAF)
    with pytest.raises(sga.SgaError, match="reduction 5 of column 1"):
        sga.voxelgrid_sampling_fields(cloud, f, LEAF, reduce=[0, 5, 0])
    lib = sga.load()
    out, out_f = C.c_void_p(), C.c_void_p()
    hostf = np.zeros(n, F32)
    arr = api._device_array(hostf.ctypes.data, _lib.F32, 1, 1)
    rc = lib.sga_voxelgrid_sampling_fields_device(cloud.ctx.h, cloud.h, C.byref(arr), None, LEAF, C.byref(out), C.byref(out_f), None, None, None, 0)
    assert rc == 1 and "fields" in lib.sga_last_error().decode() and "host" in lib.sga_last_error().decode() and not out.value and not out_f.value
    # Allocations that are too small.  The library checks a range against the allocation the runtime knows the pointer by, and torch
    # carves small tensors out of 2 MiB segments: a cloud of 600 000 points needs 4.8 MB of voxel_of and 2.4 MB of counts, which leave
    # the segment of an 8-byte tensor wherever it lies in it.
    n = 600_000
    big = sga.PointCloud(np.random.default_rng(23).uniform(-20.0, 20.0, (n, 3)).astype(F32))
    good = torch.zeros(n, dtype=torch.float32, device="cuda")
    arr = api._device_array(good.data_ptr(), _lib.F32, 1, 1)
    small = torch.empty(1, dtype=torch.int64, device="cuda")
    rc = lib.sga_voxelgrid_sampling_fields_device(big.ctx.h, big.h, C.byref(arr), None, LEAF, C.byref(out), C.byref(out_f), None, C.c_void_p(small.data_ptr()), None, 0)
    assert rc == 1 and "d_voxel_of" in lib.sga_last_error().decode() and "reaches past its allocation" in lib.sga_last_error().decode() and not out.value and not out_f.value
    small32 = torch.empty(2, dtype=torch.int32, device="cuda")
    rc = lib.sga_voxelgrid_sampling_fields_device(big.ctx.h, big.h, C.byref(arr), None, LEAF, C.byref(out), C.byref(out_f), C.c_void_p(small32.data_ptr()), None, None, 0)
    assert rc == 1 and "d_counts" in lib.sga_last_error().decode() and "reaches past its allocation" in lib.sga_last_error().decode() and not out.value
    short = api._device_array(small.data_ptr(), _lib.F64, 1, 1)  # fields of one row for 600 000 points
    rc = lib.sga_voxelgrid_sampling_fields_device(big.ctx.h, big.h, C.byref(short), None, LEAF, C.byref(out), C.byref(out_f), None, None, None, 0)
    assert rc == 1 and "fields" in lib.sga_last_error().decode() and "reaches past its allocation" in lib.sga_last_error().decode() and not out.value
    assert sga.voxelgrid_fields_launches() == before


# ---- 8. launches -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_launch_count():
    p, f = grouped_cloud(5000, 22, LEAF)
    cloud = sga.PointCloud(p)
    b0 = sga.voxelgrid_batch_launches()
    sga.voxelgrid_sampling_batch([cloud], LEAF)  # the plain chain, counted: keys, sort, runs, centroids
    plain = sga.voxelgrid_batch_launches() - b0
    assert plain >= 4
    f0 = sga.voxelgrid_fields_launches()
    sga.voxelgrid_sampling_fields(cloud, f, LEAF, reduce=["nearest", "mean", "max"], return_counts=True, return_voxel_of=True)
    mine = sga.voxelgrid_fields_launches() - f0
    assert 1 <= mine <= plain + 2, (mine, plain)
    assert mine == 4  # keys, sort, runs and ONE launch for centroids, columns, counts and voxel_of

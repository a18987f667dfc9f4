"""Sweeps deskewed on the device (csrc/cloud_pose.hip: sga_cloud_deskew / _batch / _device).

The reference is an fp64 restatement in this file, computed from the members' records, origins, times and twists, never the library.  For
a member with twist xi = (w, v), origin o, reference time s0 and a point with record r and time s:  a = float64(s) - s0, theta = |w|,
k = w / theta, K = skew(k), phi = a theta,
    D = sin(phi) K + 2 sin^2(phi / 2) K^2,   t = a v + (2 sin^2(phi / 2) (k x v) + (phi - sin phi) (k x (k x v))) / theta,
    ref = r + D (r + o) + t          (= R r + (R o + t - o) with R = I + D),
normals R n, covariances R C R^T.  The exponential is evaluated in np.longdouble where that has more than 64 bits (x86: 80) and rounded to
float64 at the end; elsewhere the same forms run in float64 — they are the stable ones (no difference of nearly equal numbers; phi - sin phi
by its series below 0.1), so the restatement keeps a few eps64 either way.  Bounds (section 3.18's with the exponential's slack):
    points       |float64(out) - ref| <= 0.5 spacing32(ref) + 256 eps64 (sum_j |R_kj| (|r_j| + |o_j|) + |t_k| + |o_k|)
    normals      the same without the offset terms: 256 eps64 (|R| |n|)_k
    covariances  0.5 spacing32(ref) + 256 eps64 (|R| |C| |R|^T)_kl
The members' records are known exactly (uploaded RELATIVE to a named origin); the output's records come back exactly through
sga_cloud_download when the origin is zero and through the kd-tree's debug view otherwise (tests/test_cloud_merge_gpu.py: records)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api
from test_cloud_merge_gpu import Member, attributes, raw, records, restate, spacing32, upload_relative
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32 = np.float32
LD = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64
EPS64 = float(np.finfo(np.float64).eps)
FAR = np.array([500e3, 4000e3, 0.0])  # a member's origin: (500 km, 4 000 km, 0)


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def exp_scaled(xi, a):
    """exp(a_i xi) for every a_i: (D = R - I (n,3,3), t (n,3)) in LD"""
    xi = np.asarray(xi, dtype=np.float64).astype(LD)
    a = np.asarray(a, dtype=np.float64).astype(LD)
    w, v = xi[:3], xi[3:]
    theta = np.sqrt(w @ w)
    k = w / theta if theta > 0 else np.zeros(3, LD)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=LD)
    KK = K @ K
    with np.errstate(invalid="ignore"):
        phi = a * theta
        s1, sh = np.sin(phi), np.sin(phi / 2)
        c2 = 2 * sh * sh
        q = phi * phi
        series = phi * q * (LD(1) / 6 - q * (LD(1) / 120 - q * (LD(1) / 5040 - q * (LD(1) / 362880 - q * (LD(1) / 39916800 - q / LD(6227020800))))))
        f3 = np.where(np.abs(phi) < 0.1, series, phi - s1)
        D = s1[:, None, None] * K + c2[:, None, None] * KK
        t = a[:, None] * v
        if theta > 0:
            t = t + (c2[:, None] * (K @ v) + f3[:, None] * (KK @ v)) / theta
    return D, t


def restate_member(m, times, xi, ref_time):
    """(ref points, their magnitudes, R) of member m in float64"""
    a = np.asarray(times, dtype=F32).astype(np.float64) - float(ref_time)
    D, t = exp_scaled(xi, a)
    r, o = m.rel.astype(LD), m.origin.astype(LD)
    with np.errstate(invalid="ignore"):
        ref = (r + np.einsum("nij,nj->ni", D, r + o) + t).astype(np.float64)
        R = (np.eye(3, dtype=LD) + D).astype(np.float64)
        mag = np.einsum("nij,nj->ni", np.abs(R), np.abs(m.rel.astype(np.float64)) + np.abs(m.origin)) + np.abs(t.astype(np.float64)) + np.abs(m.origin)
    return ref, mag, R


def within(out, ref, mag, what):
    with np.errstate(invalid="ignore"):
        err = np.abs(out.astype(np.float64) - ref)
        bound = 0.5 * spacing32(ref) + 256 * EPS64 * mag
    fin = np.isfinite(ref)
    print("%s: worst error / bound %.3f over %d values" % (what, float(np.max(err[fin] / bound[fin])) if fin.any() else 0.0, int(fin.sum())))
    assert np.all(err[fin] <= bound[fin]), what
    assert not np.isfinite(out[~fin]).any(), what  # a non-finite value stays non-finite


def check_member(out, m, times, xi, ref_time, what):
    """the deskewed cloud `out` against the restatement of member m; -> (records, normals, cov6)"""
    assert out.size() == m.n and np.array_equal(out.origin(), m.origin)  # the output keeps the input's origin
    if m.n == 0:
        assert out._has() == (False, False)  # an empty member: an empty cloud without attributes
        return np.zeros((0, 3), F32), None, None
    assert out._has() == (m.nrm is not None, m.cov6 is not None)  # an attribute the input lacks is absent
    rec, order = records(out)
    if order is None:
        assert np.array_equal(np.nan_to_num(out.points()[:, :3]), np.nan_to_num(rec.astype(np.float64)))  # points(): storage order = the input's order, w = the index
    nr, c6 = attributes(out)
    ref, mag, R = restate_member(m, times, xi, ref_time)
    within(rec, ref, mag, what + " points")
    with np.errstate(invalid="ignore"):
        if nr is not None:
            q = m.nrm.astype(np.float64)
            within(nr, np.einsum("nij,nj->ni", R, q), np.einsum("nij,nj->ni", np.abs(R), np.abs(q)), what + " normals")
        if c6 is not None:
            Cm = api.mats_from_sym6(m.cov6.astype(np.float64))
            cref = api.sym6_from_mats(R @ Cm @ R.transpose(0, 2, 1))
            cmag = api.sym6_from_mats(np.abs(R) @ np.abs(Cm) @ np.abs(R).transpose(0, 2, 1))
            within(c6, cref, cmag, what + " covariances")
    return rec, nr, c6


def twist(omega, v, seed):
    """|w| = omega about a seeded axis, |v| = v along another"""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=3), rng.normal(size=3)
    return np.concatenate([omega * a / np.linalg.norm(a), v * b / np.linalg.norm(b)])


def unit_times(n, seed, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, n).astype(F32)


def same_bits(a, b):
    """two clouds hold the same records, attributes and origin, bit for bit"""
    return raw(a) == raw(b)


@pytest.fixture(scope="module")
def eight():
    """B = 8 (read only): sizes 1, 255, 256, 257, 1000 and an empty member; every attribute combination; one cloud twice under two twists; a
    member made by a second context; a member whose origin is (500 km, 4 000 km, 0); one member's times in [-0.5, 1.5]; |w| from
    {0, 1e-9, 1e-5, 1e-3, 0.02, 1} and |v| up to 3 m; reference times 0, 0.5 and 1"""
    ctx2 = sga.Context(0)
    both = Member(255, 1)
    members = [Member(1, 2), both, Member(256, 3, covs=False), Member(0, 4), Member(257, 5, normals=False, origin=FAR), Member(1000, 6, ctx=ctx2), Member(300, 7, normals=False, covs=False), both]
    twists = [twist(1.0, 3.0, 10), twist(1e-9, 2.0, 11), twist(1e-5, 3.0, 12), twist(0.5, 1.0, 13), twist(1e-3, 1.5, 14), twist(0.02, 1.0, 15), twist(0.0, 2.5, 16), twist(1.0, 0.5, 17)]
    times = [unit_times(m.n, 20 + j) for j, m in enumerate(members)]
    times[5] = unit_times(1000, 25, -0.5, 1.5)
    refs = [1.0, 0.5, 0.0, 1.0, 0.5, 1.0, 0.0, 0.5]
    return members, times, twists, refs


# ---- against the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 8])
def test_deskew_matches_the_restatement(eight, B):
    members, times, twists, refs = eight
    pick = {1: [5], 2: [2, 4], 8: list(range(8))}[B]
    ms, ts, xs, rs = [members[j] for j in pick], [times[j] for j in pick], [twists[j] for j in pick], [refs[j] for j in pick]
    outs = sga.deskew_clouds([m.cloud for m in ms], ts, xs, rs)
    assert len(outs) == B
    recs = [check_member(o, m, t, x, r, "B=%d member %d" % (B, j))[0] for j, (o, m, t, x, r) in enumerate(zip(outs, ms, ts, xs, rs))]
    if B == 8:  # one cloud under two twists: two different results
        assert not np.array_equal(recs[1], recs[7])
        for o in outs:  # a blocking context keeps the box of the records with every member that has points
            if o.size():
                rec, _ = records(o)
                lo, hi = o._box()
                assert np.array_equal(lo, rec.min(axis=0)) and np.array_equal(hi, rec.max(axis=0))
            else:
                assert o._box() is None


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("ref_time", [0.0, 0.5, 1.0])
def test_deskewed_of_one_cloud(n, ref_time):
    """PointCloud.deskewed (sga_cloud_deskew) at every size around the workgroup's 256 and every reference time; default ref_time = 1"""
    m = Member(n, 30 + n)
    t, xi = unit_times(n, n), twist(0.02, 1.0, n)
    out = m.cloud.deskewed(t, xi, ref_time) if ref_time != 1.0 else m.cloud.deskewed(t, xi)
    check_member(out, m, t, xi, ref_time, "n=%d ref=%.1f" % (n, ref_time))


# ---- exact cases, bit for bit -------------------------------------------------------------------------------------------------------------
def test_zero_twist_and_times_at_the_reference_return_the_input(eight):
    """R = I and t = 0 exactly: records, normals and covariances of the input (whose values hold no -0)"""
    for m in (Member(257, 40), Member(255, 41, origin=FAR), Member(1000, 42, origin=(128.0, -256.0, 0.0))):
        assert not np.signbit(m.rel[m.rel == 0]).any() and not np.signbit(m.nrm[m.nrm == 0]).any() and not np.signbit(m.cov6[m.cov6 == 0]).any()
        t = unit_times(m.n, 43, -0.5, 1.5)
        for out in (m.cloud.deskewed(t, np.zeros(6), 1.0), m.cloud.deskewed(np.full(m.n, 0.5, F32), twist(1.0, 3.0, 44), 0.5), m.cloud.deskewed(np.full(m.n, 0.25, F32), twist(1e-5, 3.0, 45), 0.25)):
            rec, _ = records(out)
            nr, c6 = attributes(out)
            assert np.array_equal(rec, m.rel) and np.array_equal(nr, m.nrm) and np.array_equal(c6, m.cov6)
            assert np.array_equal(out.origin(), m.origin)


def test_batch_members_equal_their_lone_calls(eight):
    members, times, twists, refs = eight
    single = sga.deskew_clouds([members[5].cloud], [times[5]], [twists[5]], [refs[5]])[0]
    assert same_bits(single, members[5].cloud.deskewed(times[5], twists[5], refs[5]))  # a single-member batch against sga_cloud_deskew
    outs = sga.deskew_clouds([m.cloud for m in members], times, twists, refs)
    for j, (o, m) in enumerate(zip(outs, members)):
        lone = sga.deskew_clouds([m.cloud], [times[j]], [twists[j]], [refs[j]])[0]
        assert same_bits(o, lone), j
        if m.n:
            for a, b in zip(o._box(), lone._box()):
                assert np.array_equal(a, b), j
    assert same_bits(sga.deskew_clouds([members[0].cloud], [times[0]], [twists[0]])[0], members[0].cloud.deskewed(times[0], twists[0], 1.0))  # ref_times None: 1.0 each


def test_device_times_equal_host_times():
    """(the first test of a run that puts a tensor on the device also pays torch's start-up there, about ten seconds)"""
    import torch

    m = Member(1000, 50)
    t, xi = unit_times(1000, 51), twist(0.02, 2.0, 52)
    host = m.cloud.deskewed(t, xi, 0.5)
    flat = torch.from_numpy(t).to("cuda:0")
    wide = torch.zeros((1000, 2), dtype=torch.float32, device="cuda:0")
    wide[:, 1] = flat  # a column of an N x 2 tensor: stride 2
    assert wide[:, 1].stride(0) == 2
    for what, dev in (("float, stride 1", flat), ("float, stride 2", wide[:, 1]), ("double", flat.double()), ("(N, 1)", flat.reshape(-1, 1))):
        assert same_bits(m.cloud.deskewed(dev, xi, 0.5), host), what
    before = sga.cloud_deskew_launches()
    m.cloud.deskewed(flat, xi, 0.5, stream=torch.cuda.current_stream())
    assert sga.cloud_deskew_launches() - before == 2
    with pytest.raises(ValueError):
        m.cloud.deskewed(flat[:999], xi)
    with pytest.raises(ValueError):
        m.cloud.deskewed(torch.from_numpy(t), xi)  # a CPU tensor
    with pytest.raises(ValueError):
        m.cloud.deskewed(flat.half(), xi)
    with pytest.raises(ValueError):
        m.cloud.deskewed(t[:999], xi)


# ---- against the rigid path ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (1280.0, -2560.0, 0.0)])
def test_all_times_one_is_the_rigid_transform(origin):
    """times all 1, ref_time 0: every point gets exp(xi) — the restatement of sga_cloud_transform(cloud, se3_exp(xi), origin = the cloud's)
    (tests/test_cloud_merge_gpu.py: restate), within this file's bound.  Not bit for bit: the host's and the device's sine differ."""
    m = Member(1000, 60, origin=origin)
    for xi in (twist(0.02, 1.0, 61), twist(1.0, 3.0, 62), twist(1e-5, 2.0, 63)):
        T = sga.se3_exp(xi)
        out = m.cloud.deskewed(np.ones(m.n, F32), xi, 0.0)
        rec, _ = records(out)
        ref, _ = restate(m, T, m.origin)
        R, r = np.abs(T[:3, :3]), np.abs(m.rel.astype(np.float64))
        mag = (r + np.abs(m.origin)) @ R.T + np.abs(T[:3, 3]) + np.abs(m.origin)
        within(rec, ref, mag, "rigid points")
        nr, c6 = attributes(out)
        within(nr, m.nrm.astype(np.float64) @ T[:3, :3].T, np.abs(m.nrm.astype(np.float64)) @ R.T, "rigid normals")
        Cm = api.mats_from_sym6(m.cov6.astype(np.float64))
        within(c6, api.sym6_from_mats(T[:3, :3] @ Cm @ T[:3, :3].T), api.sym6_from_mats(R @ np.abs(Cm) @ R.T), "rigid covariances")
        moved = m.cloud.transformed(T, origin=m.origin)  # and the library's own rigid path: a few fp32 spacings apart at most
        assert np.abs(records(moved)[0].astype(np.float64) - rec).max() <= 2 * spacing32(np.abs(ref).max())


# ---- non-finite values ----------------------------------------------------------------------------------------------------------------------
def test_a_nan_time_and_a_nan_point_stay_out_of_the_box():
    m = Member(300, 70)
    m.rel[100] = (np.nan, 1.0, 2.0)
    m.cloud = upload_relative(m.rel, m.nrm, m.cov6, m.origin)
    t = unit_times(300, 71)
    t[7] = np.nan
    t[299] = np.inf
    xi = twist(0.02, 1.0, 72)
    out = m.cloud.deskewed(t, xi, 1.0)
    rec, _, _ = check_member(out, m, t, xi, 1.0, "non-finite")
    bad = ~np.isfinite(rec).all(axis=1)
    assert list(np.flatnonzero(bad)) == [7, 100, 299] and not np.isfinite(rec[[7, 299]]).any()  # exactly those
    lo, hi = out._box()
    assert np.array_equal(lo, rec[~bad].min(axis=0)) and np.array_equal(hi, rec[~bad].max(axis=0))
    zero = m.cloud.deskewed(t, np.zeros(6), 1.0)  # a zero twist too: a non-finite time never yields a finite point
    assert list(np.flatnonzero(~np.isfinite(records(zero)[0]).all(axis=1))) == [7, 100, 299]


# ---- context modes and launch counts ------------------------------------------------------------------------------------------------------
def test_stream_ordered_waits_for_nothing_and_one_chain_whatever_the_count(eight):
    members, times, twists, refs = eight
    blocking = sga.deskew_clouds([m.cloud for m in members], times, twists, refs)
    ctx = sga.Context(0)
    ctx.set_stream_ordered(True)
    counts = []
    for pick in ([5], list(range(8))):
        before = sga.cloud_deskew_launches()
        outs = sga.deskew_clouds([members[j].cloud for j in pick], [times[j] for j in pick], [twists[j] for j in pick], [refs[j] for j in pick], ctx=ctx)
        counts.append(sga.cloud_deskew_launches() - before)
        for j, o in zip(pick, outs):
            assert o._box() is None  # nothing waited: no box
            assert same_bits(o, blocking[j]), j
    assert counts == [2, 2], counts  # one table copy and one kernel, B = 1 and B = 8 alike
    ctx.set_stream_ordered(False)
    before = sga.cloud_deskew_launches()
    outs = sga.deskew_clouds([members[j].cloud for j in (1, 2)], [times[1], times[2]], [twists[1], twists[2]], ctx=ctx)
    assert sga.cloud_deskew_launches() - before == 2 and all(o._box() is not None for o in outs)  # a blocking context: boxes
    before = sga.cloud_deskew_launches()
    empty = sga.deskew_clouds([members[3].cloud], [times[3]], [twists[3]])
    assert sga.cloud_deskew_launches() == before and empty[0].size() == 0  # an empty member takes no workgroups: no device work
    members[1].cloud.slice(3, 100)
    assert sga.cloud_deskew_launches() == before


# ---- downstream: a deskewed cloud is an ordinary cloud ------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (1024.0, -640.0, 0.0)])
def test_downstream_results_equal_a_twin_uploaded_from_the_deskewed_records(origin):
    """voxelgrid_sampling, KdTree, estimate_covariances and a GICP align on a deskewed cloud against the same calls on a twin made by
    sga_cloud_create_f32_origin from the deskewed cloud's own records and origin: the same records in, the same results out, bit for bit"""
    o = np.array(origin)
    m = Member(3000, 80, origin=o, spread=6.0)
    out = m.cloud.deskewed(unit_times(m.n, 81), twist(0.02, 1.0, 82), 1.0)
    rec, _ = records(out)
    nr, c6 = attributes(out)
    twin = upload_relative(rec, nr, c6, o)
    assert raw(out) == raw(twin)
    for a, b in zip(out._box(), twin._box()):
        assert np.array_equal(a, b)
    assert out._voxelgrid_plan(0.5) == twin._voxelgrid_plan(0.5) and out._voxelgrid_plan(0.5)["box"]
    assert raw(sga.voxelgrid_sampling(out, 0.5)) == raw(sga.voxelgrid_sampling(twin, 0.5))
    ta, tb = sga.KdTree(out), sga.KdTree(twin)
    (da, tha, axa, pa, oa), (db, thb, axb, pb, ob) = ta._tree(), tb._tree()
    assert da == db and np.array_equal(tha[1:], thb[1:]) and np.array_equal(axa[1:], axb[1:]) and np.array_equal(pa, pb) and np.array_equal(oa, ob)  # (entry 0 of the nodes is never written)
    src = Member(900, 83, spread=6.0)
    init = np.eye(4)
    init[:3, 3] = o + (0.2, 0.1, 0.0)
    ra = sga.align(out, src.cloud, ta, init, max_iterations=5)
    rb = sga.align(twin, src.cloud, tb, init, max_iterations=5)
    assert ra.T_target_source.tobytes() == rb.T_target_source.tobytes() and ra.iterations == rb.iterations and ra.num_inliers == rb.num_inliers and ra.error == rb.error
    sga.estimate_covariances(out, ta, 10)  # last: the estimation overwrites the covariances of both
    sga.estimate_covariances(twin, tb, 10)
    assert raw(out) == raw(twin)


# ---- refusals on a live device --------------------------------------------------------------------------------------------------------------
def test_a_cloud_of_another_device_is_refused():
    if sga.load().sga_device_count() < 2:
        pytest.skip("ONE DEVICE ONLY: the refusal of a cloud that lives on another device was NOT exercised")
    here, there = Member(64, 90), Member(64, 91, ctx=sga.Context(1))
    t = unit_times(64, 92)
    before = sga.cloud_deskew_launches()
    with pytest.raises(sga.SgaError, match="cloud 1 lives on another device"):
        sga.deskew_clouds([here.cloud, there.cloud], [t, t], np.zeros((2, 6)))
    assert sga.cloud_deskew_launches() == before


def test_refusals_that_need_live_pointers():
    import torch

    lib = sga.load()
    m = Member(3000, 93)
    ctx = m.cloud.ctx
    t = unit_times(m.n, 94)
    xi = np.ascontiguousarray(twist(0.02, 1.0, 95))
    dev = torch.from_numpy(t).to("cuda:0")
    torch.cuda.synchronize()
    before = sga.cloud_deskew_launches()
    out = C.c_void_p(1)

    def refused(rc, *texts):
        msg = lib.sga_last_error().decode()
        assert rc == 1 and all(x in msg for x in texts), (rc, msg)
        assert out.value is None
        out.value = 1

    # a host pointer handed to the device variant names the host entry point, pageable or pinned
    for host in (t, api.pinned_copy(t)):
        refused(lib.sga_cloud_deskew_device(ctx.h, m.cloud.h, C.byref(api._device_array(host.ctypes.data, _lib.F32, 1, 1)), api._dp(xi), 1.0, None, 0, C.byref(out)), "times", "go through sga_cloud_deskew")
    # a device pointer handed to the host variant names the device entry point
    refused(lib.sga_cloud_deskew(ctx.h, m.cloud.h, C.cast(C.c_void_p(dev.data_ptr()), C.POINTER(C.c_float)), api._dp(xi), 1.0, C.byref(out)), "times[0] is device memory", "sga_cloud_deskew_device")
    # times shorter than the cloud.  The library checks a caller's range against the allocation the runtime reports for it, so what it can
    # refuse is a range that leaves that allocation: 64 times for 3000 points is refused by the Python layer from the shapes; at the C
    # boundary a times array whose rows, at the stride claimed, end 50 GB behind its start is refused whatever block the tensor was carved from
    with pytest.raises(ValueError):
        m.cloud.deskewed(dev[:64], xi)
    refused(lib.sga_cloud_deskew_device(ctx.h, m.cloud.h, C.byref(api._device_array(dev.data_ptr(), _lib.F32, 1, 1 << 22)), api._dp(xi), 1.0, None, 0, C.byref(out)), "times", "past its allocation")  # a stride that leaves it
    refused(lib.sga_cloud_deskew_device(ctx.h, m.cloud.h, C.byref(api._device_array(dev.data_ptr() + 2, _lib.F32, 1, 1)), api._dp(xi), 1.0, None, 0, C.byref(out)), "times", "not aligned")
    assert sga.cloud_deskew_launches() == before  # a refusal enqueues nothing
    check_member(m.cloud.deskewed(dev, xi), m, t, xi, 1.0, "after the refusals")  # and the context is as good as before


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_deskew_clouds(tmp_path):
    """include/small_gicp_amd.hpp: deskew_clouds, PointCloud::deskewed and se3_log against a host loop in (long) double
    (tests/cpp/test_cpp_cloud_deskew.cpp, compiled with g++ as test_cloud_merge_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_deskew"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_deskew.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = sga.synthetic.kitti_like_scan(0)
    (tmp_path / "p.f32").write_bytes(np.ascontiguousarray(pts[:20000, :3], dtype=F32).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines()]
    print(p.stdout)
    assert sum(r[0] == "DESKEW" for r in rows) == 4 and sum(r[0] == "LONE" for r in rows) == 4 and sum(r[0] == "SAME" for r in rows) == 4 and sum(r[0] == "LOG" for r in rows) == 1
    for r in rows:
        if r[0] == "DESKEW":
            assert int(r[3]) > 0 and r[5] == "1", r
        elif r[0] in ("LONE", "SAME"):
            assert r[3] == "1", r
        elif r[0] == "LOG":
            assert r[2] == "200" and r[4] == "1", r


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def test_deskewed_sweeps_track_better_than_raw_sweeps():
    """run_synthetic(8) three ways: (a) raw sweeps registered as if they were snapshots, (b) the sweeps with their times — deskewed on the
    device under constant velocity, from the third frame on (the first has no motion before it, the second no estimate of one when it is
    registered) —, (c) the
    unskewed scans.  From the third frame on every relative pose of (b) is closer to the ground truth than (a)'s, in translation; (c)
    is what run_synthetic(8) without the new arguments gives, bit for bit."""
    from small_gicp_amd import odometry

    a = odometry.run_synthetic(8, sweeps=True, times=False)
    b = odometry.run_synthetic(8, sweeps=True)
    c = odometry.run_synthetic(8, sweeps=False)
    plain = odometry.run_synthetic(8)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(c["estimated"], plain["estimated"])) and len(c["estimated"]) == 8
    assert a["sweeps"] and b["sweeps"] and not c["sweeps"]
    print("relative translation error per frame pair  (a) raw sweeps: %s" % " ".join("%.4f" % e for e in a["rpe_trans_m"]))
    print("                                           (b) deskewed:   %s" % " ".join("%.4f" % e for e in b["rpe_trans_m"]))
    print("                                           (c) snapshots:  %s" % " ".join("%.4f" % e for e in c["rpe_trans_m"]))
    print("ate_trans_m_max: (a) %.4f (b) %.4f (c) %.4f" % (a["ate_trans_m_max"], b["ate_trans_m_max"], c["ate_trans_m_max"]))
    # the first two frames are the same in (a) and (b): nothing to deskew with yet (the second is deskewed only as the third's target)
    assert a["estimated"][1].tobytes() == b["estimated"][1].tobytes()
    for f in range(2, 8):  # frame pair (f - 1, f): entry f - 1 of the relative errors
        assert b["rpe_trans_m"][f - 1] < a["rpe_trans_m"][f - 1], (f, a["rpe_trans_m"], b["rpe_trans_m"])

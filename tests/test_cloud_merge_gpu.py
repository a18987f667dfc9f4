"""Posed clouds merged on the device (csrc/cloud_pose.hip: sga_cloud_merge / sga_cloud_transform).

The reference is an fp64 restatement in this file, computed from the members' records and origins, never the library: for member m with
pose (R, t) and origin o_m, and the output's origin o,
    c = ((R0 o0 + R1 o1) + R2 o2) + t per row (the order the header states),   ref = R r + (c - o)   in numpy float64.
Bounds (not tuned: one fp32 rounding, and 64 eps64 of the magnitudes for a three-term double dot product plus one add in any order, with
or without contraction — the true factor is about 4):
    points       |float64(out) - ref| <= 0.5 spacing32(ref) + 64 eps64 (sum_j |R_kj r_j| + |c_k - o_k|)
    normals      the same without the offset term
    covariances  0.5 spacing32(ref) + 64 eps64 (|R| |C| |R|^T)_kl
spacing32(x) is the spacing of fp32 in the binade of x.  Where the double arithmetic is exact (identity poses, quarter turns with integer
translations) the outputs are compared bit for bit.

The members' records are known exactly: they are uploaded RELATIVE to a named origin (sga_cloud_create_f32_origin takes the records as
they are).  The output's records come back exactly through sga_cloud_download when its origin is zero and through the kd-tree's debug
view (device frame, with the index words) otherwise."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import api
from test_gpu_parity import POSE_TOL_R, POSE_TOL_T
from conftest import ROOT, pose_error

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS64 = float(np.finfo(np.float64).eps)
FAR = np.array([500e3, 4000e3, 0.0])  # a member's origin: (500 km, 4 000 km, 0)


# ---- members with known records ---------------------------------------------------------------------------------------------------------
class Member:
    def __init__(self, n, seed, normals=True, covs=True, origin=(0.0, 0.0, 0.0), ctx=None, spread=20.0):
        rng = np.random.default_rng(seed)
        self.rel = rng.uniform(-spread, spread, (n, 3)).astype(F32)
        v = rng.normal(size=(n, 3))
        self.nrm = (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)).astype(F32) if normals else None
        a = rng.normal(size=(n, 3, 3)) * 0.05
        self.cov6 = api.sym6_from_mats(a @ a.transpose(0, 2, 1) + 1e-4 * np.eye(3)).astype(F32) if covs else None
        self.origin = np.array(origin, dtype=np.float64)
        self.cloud = upload_relative(self.rel, self.nrm, self.cov6, self.origin, ctx)

    @property
    def n(self):
        return len(self.rel)


def upload_relative(rel, nrm, cov6, origin, ctx=None):
    """sga_cloud_create_f32_origin: the records go to the device as they are"""
    ctx = ctx or sga.default_context()
    h = C.c_void_p()
    rel = np.ascontiguousarray(rel, dtype=F32)
    nrm = None if nrm is None else np.ascontiguousarray(nrm, dtype=F32)
    cov6 = None if cov6 is None else np.ascontiguousarray(cov6, dtype=F32)
    o = np.ascontiguousarray(origin, dtype=np.float64)
    api.check(sga.load().sga_cloud_create_f32_origin(ctx.h, api._fp(rel), api._fp(nrm), api._fp(cov6), len(rel), api._dp(o), C.byref(h)))
    return sga.PointCloud(ctx=ctx, _handle=h)


def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    T = np.eye(4)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = t
    return T


QUARTER = [  # axis permutations with integer translations: the double arithmetic is exact
    np.array([[0, -1, 0, 3], [1, 0, 0, -2], [0, 0, 1, 1], [0, 0, 0, 1]], dtype=np.float64),
    np.array([[0, 0, 1, -4], [0, 1, 0, 0], [-1, 0, 0, 6], [0, 0, 0, 1]], dtype=np.float64),
    np.array([[-1, 0, 0, 0], [0, 0, 1, 5], [0, 1, 0, -7], [0, 0, 0, 1]], dtype=np.float64),
]


def general_poses(count, seed=1):
    rng = np.random.default_rng(seed)
    return [pose(*rng.uniform(-1.0, 1.0, 3), t=rng.uniform(-8.0, 8.0, 3)) for _ in range(count)]


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def spacing32(x):
    """spacing of fp32 in the binade of x (the denormal spacing below 2^-126)"""
    _, e = np.frexp(np.abs(np.asarray(x, dtype=np.float64)))
    return np.ldexp(1.0, np.maximum(e - 24, -149))


def member_offset(T, o_m):
    """c = R o_m + t per row as the header states it: ((R0 o0 + R1 o1) + R2 o2) + t, every operation rounded on its own"""
    return np.array([((T[k, 0] * o_m[0] + T[k, 1] * o_m[1]) + T[k, 2] * o_m[2]) + T[k, 3] for k in range(3)])


def restate(member, T, o):
    """(ref points, their bound's magnitude) of one member in the output's device frame, float64"""
    R, r = T[:3, :3], member.rel.astype(np.float64)
    d = member_offset(T, member.origin) - np.asarray(o, dtype=np.float64)
    ref = (R[:, 0] * r[:, 0:1] + R[:, 1] * r[:, 1:2]) + R[:, 2] * r[:, 2:3] + d
    mag = np.abs(R[:, 0] * r[:, 0:1]) + np.abs(R[:, 1] * r[:, 1:2]) + np.abs(R[:, 2] * r[:, 2:3]) + np.abs(d)
    return ref, mag


def within(out, ref, mag, what):
    err = np.abs(out.astype(np.float64) - ref)
    bound = 0.5 * spacing32(ref) + 64 * EPS64 * mag
    fin = np.isfinite(ref)
    print("%s: worst error / bound %.3f over %d values" % (what, float(np.max(err[fin] / bound[fin])) if fin.any() else 0.0, int(fin.sum())))
    assert np.all(err[fin] <= bound[fin]), what
    assert not np.isfinite(out[~fin]).any(), what  # a non-finite point stays non-finite


def records(cloud):
    """(device-frame records (n, 3) float32, exactly; the index words or None)"""
    n = cloud.size()
    if not cloud.origin().any():
        return cloud.xyz(), None  # origin zero: the download is the records as they are
    _, _, _, pts, order = sga.KdTree(cloud)._tree()
    assert np.array_equal(np.sort(order), np.arange(n))  # the index words are a permutation of 0 .. n - 1
    rec = np.empty((n, 3), F32)
    rec[order] = pts
    return rec, order


def attributes(cloud):
    n = cloud.size()
    hn, hc = cloud._has()
    nr, c6 = np.zeros((n, 3), F32), np.zeros((n, 6), F32)
    api.check(sga.load().sga_cloud_download(cloud.ctx.h, cloud.h, None, api._fp(nr) if hn else None, api._fp(c6) if hc else None))
    return (nr if hn else None), (c6 if hc else None)


def check_merge(out, members, Ts, o, normals=None, covs=None, exact=False):
    """the merged cloud `out` against the restatement of every member"""
    total = sum(m.n for m in members)
    assert out.size() == total
    assert np.array_equal(out.origin(), np.asarray(o, dtype=np.float64))
    nonempty = [m for m in members if m.n > 0]
    want_n = all(m.nrm is not None for m in nonempty) and bool(nonempty) if normals is None else normals
    want_c = all(m.cov6 is not None for m in nonempty) and bool(nonempty) if covs is None else covs
    assert out._has() == (want_n, want_c)
    rec, _ = records(out)
    nr, c6 = attributes(out)
    if total:
        assert np.array_equal(out.points()[:, :3], rec.astype(np.float64) + out.origin(), equal_nan=True)  # points(): the records in storage order — the merged order
    off = 0
    for k, (m, T) in enumerate(zip(members, Ts)):
        if m.n == 0:
            continue
        R = T[:3, :3]
        ref, mag = restate(m, T, o)
        within(rec[off : off + m.n], ref, mag, "member %d points" % k)
        if exact:
            assert np.array_equal(rec[off : off + m.n], ref.astype(F32)), k
        if want_n:
            q = m.nrm.astype(np.float64)
            nref = (R[:, 0] * q[:, 0:1] + R[:, 1] * q[:, 1:2]) + R[:, 2] * q[:, 2:3]
            within(nr[off : off + m.n], nref, np.abs(q) @ np.abs(R).T, "member %d normals" % k)
            if exact:
                assert np.array_equal(nr[off : off + m.n], nref.astype(F32)), k
        if want_c:
            Cm = api.mats_from_sym6(m.cov6.astype(np.float64))
            cref = api.sym6_from_mats(R @ Cm @ R.T)
            cmag = api.sym6_from_mats(np.abs(R) @ np.abs(Cm) @ np.abs(R).T)
            within(c6[off : off + m.n], cref, cmag, "member %d covariances" % k)
            if exact:
                assert np.array_equal(c6[off : off + m.n], cref.astype(F32)), k
        off += m.n
    return rec, nr, c6


@pytest.fixture(scope="module")
def trio():
    """members of 255, 256 and 257 points with both attributes (read only)"""
    return [Member(n, seed) for seed, n in enumerate((255, 256, 257))]


def eight(trio, ctx2=None):
    """B = 8: one member first and last of its call (under two poses), an empty member in the middle, one on a second context"""
    return [trio[0], trio[1], Member(1, 41), Member(0, 42), trio[2], Member(1000, 43, ctx=ctx2), Member(300, 40), trio[0]]


# ---- points, normals, covariances under general poses ---------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 2, 8])
def test_merge_matches_the_restatement(trio, B):
    ctx2 = sga.Context(0)
    members = trio[:B] if B < 8 else eight(trio, ctx2)
    Ts = general_poses(B, seed=B)
    o = np.zeros(3)
    out = sga.merge_clouds([m.cloud for m in members], Ts, origin=o)
    check_merge(out, members, Ts, o)
    if B == 8:  # one cloud under two poses: two different stretches
        rec, _ = records(out)
        assert not np.array_equal(rec[: trio[0].n], rec[-trio[0].n :])


def test_a_member_that_came_from_torch(trio):
    """(the first test of a run that puts a tensor on the device also pays torch's start-up there, about ten seconds; the merge itself is milliseconds)"""
    import torch

    tm = Member(300, 44)
    tm.cloud = sga.PointCloud.from_torch(torch.from_numpy(tm.rel).to("cuda:0"), torch.from_numpy(tm.nrm).to("cuda:0"), torch.from_numpy(tm.cov6).to("cuda:0"))
    assert not tm.cloud.origin().any()  # near zero: the records are the tensor's values
    members, Ts, o = [trio[0], tm, trio[1]], general_poses(3, seed=12), np.zeros(3)
    check_merge(sga.merge_clouds([m.cloud for m in members], Ts, origin=o), members, Ts, o)


@pytest.mark.parametrize("n", [255, 256, 257])
def test_transformed_is_the_merge_of_one(n):
    m = Member(n, 7 + n)
    T = general_poses(1, seed=n)[0]
    o = np.array([128.0, 0.0, -128.0])
    one = m.cloud.transformed(T, origin=o)
    check_merge(one, [m], [T], o)
    merged = sga.merge_clouds([m.cloud], [T], origin=o)
    assert np.array_equal(records(one)[0], records(merged)[0])
    for a, b in zip(attributes(one), attributes(merged)):
        assert np.array_equal(a, b)


# ---- exact cases ------------------------------------------------------------------------------------------------------------------------
def test_identity_poses_concatenate_and_return_the_input(trio):
    origin = np.array([256.0, -384.0, 128.0])
    members = [Member(n, 20 + n, origin=origin) for n in (255, 257)]
    for Ts in (None, [np.eye(4)] * 2):
        out = sga.merge_clouds([m.cloud for m in members], Ts, origin=origin)
        rec, nr, c6 = check_merge(out, members, [np.eye(4)] * 2, origin, exact=True)
        assert np.array_equal(rec, np.concatenate([m.rel for m in members]))
        assert np.array_equal(nr, np.concatenate([m.nrm for m in members])) and np.array_equal(c6, np.concatenate([m.cov6 for m in members]))
        _, order = records(out)
        assert order is not None  # (origin not zero: the kd view showed the index words to be 0 .. n - 1, each once)
    same = members[0].cloud.transformed(np.eye(4), origin=origin)
    assert np.array_equal(records(same)[0], members[0].rel) and np.array_equal(same.origin(), origin)
    assert np.array_equal(same.points(), members[0].cloud.points()) and np.array_equal(same.normals(), members[0].cloud.normals()) and np.array_equal(same.covs(), members[0].cloud.covs())


def test_quarter_turns_with_integer_translations_are_exact(trio):
    out = sga.merge_clouds([m.cloud for m in trio], QUARTER, origin=np.zeros(3))
    check_merge(out, trio, QUARTER, np.zeros(3), exact=True)
    far = [Member(256, 30, origin=(1280.0, -2560.0, 0.0)), Member(255, 31, origin=(1408.0, -2560.0, 128.0))]
    o = np.array([2560.0, 1280.0, 0.0])  # (near where the first member's origin lands)
    out = sga.merge_clouds([m.cloud for m in far], QUARTER[:2], origin=o)
    check_merge(out, far, QUARTER[:2], o, exact=True)


# ---- the attribute rule ---------------------------------------------------------------------------------------------------------------
def test_an_attribute_is_kept_only_if_every_nonempty_member_has_it(trio):
    Ts = general_poses(3, seed=9)
    o = np.zeros(3)
    full = sga.merge_clouds([m.cloud for m in trio], Ts, origin=o)
    assert full._has() == (True, True)  # both attributes
    full_rec = records(full)[0]
    bare = Member(256, 50, covs=False)  # one member without covariances: the output has none, its points are unchanged
    mixed = [trio[0], bare, trio[2]]
    out = sga.merge_clouds([m.cloud for m in mixed], Ts, origin=o)
    rec, nr, c6 = check_merge(out, mixed, Ts, o, normals=True, covs=False)
    assert c6 is None and nr is not None
    assert np.array_equal(rec[: trio[0].n], full_rec[: trio[0].n]) and np.array_equal(rec[-trio[2].n :], full_rec[-trio[2].n :])
    only_normals = [Member(255, 51, covs=False), Member(257, 52, covs=False)]  # normals only
    check_merge(sga.merge_clouds([m.cloud for m in only_normals], Ts[:2], origin=o), only_normals, Ts[:2], o, normals=True, covs=False)
    only_covs = [Member(255, 53, normals=False), trio[1]]  # all members with covariances, one without normals
    check_merge(sga.merge_clouds([m.cloud for m in only_covs], Ts[:2], origin=o), only_covs, Ts[:2], o, normals=False, covs=True)
    with_empty = [trio[0], Member(0, 54, normals=False, covs=False), trio[1]]  # an empty member has no say
    check_merge(sga.merge_clouds([m.cloud for m in with_empty], Ts, origin=o), with_empty, Ts, o, normals=True, covs=True)
    nothing = sga.merge_clouds([Member(0, 55).cloud, Member(0, 56).cloud], origin=[128.0, 0.0, 0.0])  # empty members only
    assert nothing.size() == 0 and nothing._has() == (False, False) and np.array_equal(nothing.origin(), [128.0, 0.0, 0.0])
    assert sga.merge_clouds([]).size() == 0


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
def test_a_far_member_and_a_near_member_land_together():
    """origin (500 km, 4 000 km, 0) and a member near zero, posed so that both land within metres of the output's origin: c - o is metres,
    and the bound holds with it — the kilometres cancel once, on the host, in double"""
    a, b = Member(257, 60, origin=FAR), Member(255, 61)
    Ta = pose(0.3, 0.02, -0.01)
    Ta[:3, 3] = -(Ta[:3, :3] @ FAR) + np.array([3.0, 4.0, 0.5])
    Tb = pose(-0.2, 0.0, 0.03, t=(1.0, -2.0, 0.25))
    o = np.zeros(3)
    d = member_offset(Ta, FAR) - o
    assert np.all(np.abs(d) < 10.0), d
    out = sga.merge_clouds([a.cloud, b.cloud], [Ta, Tb], origin=o)
    check_merge(out, [a, b], [Ta, Tb], o)
    # the other way round: the output lives far away too
    Ta2 = pose(0.3, 0.0, 0.0, t=(12.0, -7.0, 1.0))
    Tb2 = np.eye(4)
    Tb2[:3, 3] = Ta2[:3, :3] @ FAR + np.array([5.0, 5.0, 0.0])
    o2 = 128.0 * np.round((Ta2[:3, :3] @ FAR + Ta2[:3, 3]) / 128.0)
    assert np.all(np.abs(o2[:2]) > 1e5) and np.all(o2 % 128.0 == 0.0)
    out = sga.merge_clouds([a.cloud, b.cloud], [Ta2, Tb2], origin=o2)
    check_merge(out, [a, b], [Ta2, Tb2], o2)


def reference_box(members, Ts):
    """the box of the finite posed points in the caller's frame, from the restatement at origin zero"""
    q = np.concatenate([restate(m, T, np.zeros(3))[0] for m, T in zip(members, Ts) if m.n])
    q = q[np.isfinite(q).all(axis=1)]
    return q.min(axis=0), q.max(axis=0)


def chosen(lo, hi):
    o = np.zeros(3)
    sga.load().sga_choose_origin(api._dp(np.ascontiguousarray(lo)), api._dp(np.ascontiguousarray(hi)), api._dp(o))
    return o


@pytest.mark.parametrize("where", ["near", "far", "very_far"])
def test_origin_none_is_the_rule_applied_to_the_box_of_the_posed_points(where):
    members = [Member(257, 70), Member(255, 71), Member(256, 72, origin=(128.0, 0.0, 0.0))]
    if where == "very_far":
        members = [Member(257, 70, origin=FAR), Member(255, 71, origin=FAR + np.array([128.0, -128.0, 0.0]))]
    Ts = general_poses(len(members), seed=3)
    centre = {"near": np.array([10.0, -20.0, 3.0]), "far": np.array([1000.0, -680.0, 5.0]), "very_far": np.zeros(3)}[where]
    for T, m in zip(Ts, members):
        T[:3, 3] = centre + T[:3, 3] - T[:3, :3] @ m.origin  # (every member lands around `centre`)
    if where == "very_far":
        Ts = [pose(0.0, 0.0, 0.0, t=(1.0, 2.0, 3.0)), pose(0.0, 0.0, 0.0, t=(-4.0, 5.0, 0.0))]  # the members stay where their origins are
    lo, hi = reference_box(members, Ts)
    o = chosen(lo, hi)
    mid = 0.5 * (lo + hi) / 128.0
    assert np.all(np.abs(mid - np.floor(mid) - 0.5) * 128.0 >= 1.0)  # the box centre is a metre or more from a rounding boundary of the 128 m rule
    assert o.any() == (where != "near") and np.all(o % 128.0 == 0.0)
    launches = sga.cloud_merge_launches()
    out = sga.merge_clouds([m.cloud for m in members], Ts)
    assert sga.cloud_merge_launches() - launches == (2 if where == "near" else 4)  # a second pass only when the origin is not zero
    assert np.array_equal(out.origin(), o)
    rec, _, _ = check_merge(out, members, Ts, o)
    blo, bhi = out._box()
    assert np.array_equal(blo, rec.min(axis=0)) and np.array_equal(bhi, rec.max(axis=0))  # the box of the records, exactly


def test_origin_given_the_records_follow_it(trio):
    Ts = general_poses(3, seed=5)
    for o in (np.array([128.0, -256.0, 0.0]), np.array([1.5, 0.25, -3.0]), np.array([-4096.0, 8192.0, 128.0])):
        check_merge(sga.merge_clouds([m.cloud for m in trio], Ts, origin=o), trio, Ts, o)


def test_nonfinite_points_pass_through_and_stay_out_of_the_box():
    a, b = Member(300, 80), Member(257, 81)
    a.rel[5] = (np.nan, 1.0, 2.0)
    a.rel[299] = (3.0, np.inf, -1.0)
    b.rel[0] = (-np.inf, 0.0, 0.0)
    a.cloud, b.cloud = upload_relative(a.rel, a.nrm, a.cov6, a.origin), upload_relative(b.rel, b.nrm, b.cov6, b.origin)
    Ts = general_poses(2, seed=6)
    with np.errstate(invalid="ignore"):
        for origin in (np.zeros(3), None):
            out = sga.merge_clouds([a.cloud, b.cloud], Ts, origin=origin)
            rec, _, _ = check_merge(out, [a, b], Ts, np.zeros(3))
            bad = ~np.isfinite(rec).all(axis=1)
            assert list(np.flatnonzero(bad)) == [5, 299, 300] and not np.isfinite(rec[bad]).any()
            blo, bhi = out._box()
            assert np.array_equal(blo, rec[~bad].min(axis=0)) and np.array_equal(bhi, rec[~bad].max(axis=0))


def test_the_box_bounds_the_records_and_is_absent_when_nothing_waited(trio):
    Ts = general_poses(3, seed=8)
    o = np.array([128.0, 0.0, 0.0])
    out = sga.merge_clouds([m.cloud for m in trio], Ts, origin=o)  # a blocking context keeps the box
    rec, _ = records(out)
    blo, bhi = out._box()
    assert np.array_equal(blo, rec.min(axis=0)) and np.array_equal(bhi, rec.max(axis=0))
    ctx = sga.Context(0)
    ctx.set_stream_ordered(True)
    ordered = sga.merge_clouds([m.cloud for m in trio], Ts, origin=o, ctx=ctx)  # stream-ordered, origin given: waits for nothing, no box
    assert ordered._box() is None
    assert np.array_equal(records(ordered)[0], rec)
    chosen_there = sga.merge_clouds([m.cloud for m in trio], Ts, ctx=ctx)  # origin None: the box was reduced, so it is kept
    assert chosen_there._box() is not None and not chosen_there.origin().any()
    ctx.set_stream_ordered(False)


# ---- launches ---------------------------------------------------------------------------------------------------------------------------
def test_one_chain_whatever_the_count(trio):
    o = np.zeros(3)
    counts = []
    for B in (1, 8):
        members = trio[:1] if B == 1 else eight(trio)
        Ts = general_poses(B, seed=11)
        before = sga.cloud_merge_launches()
        sga.merge_clouds([m.cloud for m in members], Ts, origin=o)
        counts.append(sga.cloud_merge_launches() - before)
    assert counts[0] == counts[1] == 2, counts  # one table copy and one kernel
    before = sga.cloud_merge_launches()
    trio[1].cloud.slice(3, 100)
    Member(64, 90)
    assert sga.cloud_merge_launches() == before  # a lone slice or an upload counts nothing


def test_refusals_that_need_live_clouds(trio):
    lib = sga.load()
    if lib.sga_device_count() >= 2:
        other = Member(64, 91, ctx=sga.Context(1))
        with pytest.raises(sga.SgaError, match="cloud 1 lives on another device"):
            sga.merge_clouds([trio[0].cloud, other.cloud])
    with pytest.raises(ValueError):
        sga.merge_clouds([trio[0].cloud], [np.eye(4), np.eye(4)])
    bad = np.eye(4)
    bad[1, 2] = np.nan
    before = sga.cloud_merge_launches()
    with pytest.raises(sga.SgaError, match="pose 1 has a non-finite entry"):
        sga.merge_clouds([trio[0].cloud, trio[1].cloud], [np.eye(4), bad])
    with pytest.raises(sga.SgaError, match="origin has a non-finite entry"):
        trio[0].cloud.transformed(np.eye(4), origin=[0.0, np.inf, 0.0])
    assert sga.cloud_merge_launches() == before


# ---- downstream: a merged cloud is an ordinary cloud ------------------------------------------------------------------------------------
def raw(cloud):
    n = cloud.size()
    hn, hc = cloud._has()
    xyz, nr, c6 = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros((n, 6), F32)
    api.check(sga.load().sga_cloud_download(cloud.ctx.h, cloud.h, api._fp(xyz), api._fp(nr) if hn else None, api._fp(c6) if hc else None))
    return (n, hn, hc, xyz.tobytes(), nr.tobytes(), c6.tobytes(), cloud.origin().tobytes())


@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (1024.0, -640.0, 0.0)])
def test_downstream_results_equal_a_twin_uploaded_from_the_merged_records(origin):
    """voxelgrid_sampling, KdTree, estimate_covariances and a GICP align on a merged cloud against the same calls on a twin made by
    sga_cloud_create_f32_origin from the merged cloud's own records and origin: the same records in, the same results out, bit for bit"""
    o = np.array(origin)
    members = [Member(1500, 100, spread=6.0), Member(1200, 101, spread=6.0), Member(257, 102, spread=6.0)]
    Ts = [pose(0.1 * k, 0.01, -0.02, t=o + (0.5 * k, -0.3 * k, 0.1)) for k in range(3)]
    merged = sga.merge_clouds([m.cloud for m in members], Ts, origin=o)
    rec, _ = records(merged)
    nr, c6 = attributes(merged)
    twin = upload_relative(rec, nr, c6, o)
    assert raw(merged) == raw(twin)
    for a, b in zip(merged._box(), twin._box()):
        assert np.array_equal(a, b)
    assert merged._voxelgrid_plan(0.5) == twin._voxelgrid_plan(0.5) and merged._voxelgrid_plan(0.5)["box"]
    assert raw(sga.voxelgrid_sampling(merged, 0.5)) == raw(sga.voxelgrid_sampling(twin, 0.5))
    tm, tt = sga.KdTree(merged), sga.KdTree(twin)
    (da, tha, axa, pa, oa), (db, thb, axb, pb, ob) = tm._tree(), tt._tree()
    assert da == db and np.array_equal(tha[1:], thb[1:]) and np.array_equal(axa[1:], axb[1:]) and np.array_equal(pa, pb) and np.array_equal(oa, ob)  # (entry 0 of the nodes is never written)
    # a GICP align against the two trees (the rotated covariances ride along), from the same pose
    src = Member(900, 103, spread=6.0)
    init = pose(0.05, 0.0, 0.0, t=o + (0.2, 0.1, 0.0))
    ra = sga.align(merged, src.cloud, tm, init, max_iterations=5)
    rb = sga.align(twin, src.cloud, tt, init, max_iterations=5)
    assert ra.T_target_source.tobytes() == rb.T_target_source.tobytes() and ra.iterations == rb.iterations and ra.num_inliers == rb.num_inliers and ra.error == rb.error
    # last: the estimation overwrites the covariances of both
    sga.estimate_covariances(merged, tm, 10)
    sga.estimate_covariances(twin, tt, 10)
    assert raw(merged) == raw(twin)


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def test_scan_to_submap_odometry_matches_oracle(orc):
    """run_synthetic_submap(6, window=3): per frame the oracle is given the GPU's own merged points and covariances and the GPU's scan and
    registers from the previous pose — the comparison (a) of test_scan_to_scan_odometry_matches_oracle, with its tolerances and the same
    iteration count; each relative motion is the simulated 1 m."""
    from small_gicp_amd import odometry

    out = odometry.run_synthetic_submap(6, window=3, record=True)
    assert len(out["records"]) == 5 and len(out["estimated"]) == 6 and out["frames"] == 6
    for key in ("registration_ms_per_scan", "total_ms_per_scan", "total_ms_per_scan_median", "mean_iterations", "ate_trans_m_max", "estimated", "ground_truth"):
        assert key in out, key
    sizes = []
    for f, (submap, scan, init, T, iterations) in enumerate(out["records"], start=1):
        sizes.append(submap.size())
        assert submap._has() == (False, True) and submap._box() is None  # covariances rode along; the stream-ordered driver named its origin
        target = orc.Cloud(submap.points()[:, :3], None, submap.covs()[:, :3, :3], tree=True)
        source = orc.Cloud(scan.xyz().astype(np.float64), None, scan.covs()[:, :3, :3], tree=False)
        ref = orc.align(target, source, orc.default_setting(factor_kind=orc.GICP, num_threads=8), init)
        dt, dr = pose_error(T, ref.T_target_source)
        print("frame %d: submap %d points, dt %.2e dr %.2e, iterations %d / %d" % (f, submap.size(), dt, dr, iterations, ref.iterations + 1))
        assert dt < POSE_TOL_T and dr < POSE_TOL_R and iterations == ref.iterations + 1, (f, dt, dr, iterations, ref.iterations)
        rel = np.linalg.inv(out["estimated"][f - 1]) @ out["estimated"][f]
        assert abs(np.linalg.norm(rel[:3, 3]) - 1.0) < 0.02
    assert sizes[0] < sizes[1] < sizes[2]  # the window fills: 1, 2, 3 scans


# ---- the C++ header -------------------------------------------------------------------------------------------------------------------------
def test_cpp_merge_clouds(tmp_path):
    """include/small_gicp_amd.hpp: merge_clouds and PointCloud::transformed against the host loop (tests/cpp/test_cpp_cloud_merge.cpp,
    compiled with g++ as test_batch_voxelmap_insert_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_merge"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_merge.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = sga.synthetic.kitti_like_scan(0)
    (tmp_path / "p.f32").write_bytes(np.ascontiguousarray(pts[:20000, :3], dtype=F32).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = [ln.split() for ln in p.stdout.splitlines()]
    print(p.stdout)
    assert sum(r[0] == "EXACT" for r in rows) == 4 and sum(r[0] == "POSED" for r in rows) == 4 and sum(r[0] == "LONE" for r in rows) == 4
    for r in rows:
        if r[0] in ("EXACT", "POSED"):
            assert int(r[3]) > 0 and r[5] == "1", r
        elif r[0] == "LONE":
            assert r[3] == "1", r
        elif r[0] == "SHAPE":
            assert r[2] == r[3] and r[5] == "1" and r[7] == "1", r
    assert any(r[0] == "SHAPE" for r in rows)

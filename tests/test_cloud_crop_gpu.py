"""Clouds cropped and gathered on the device (csrc/cloud_crop.hip: sga_cloud_crop / _batch / _device, sga_cloud_select).

The reference is an fp64 restatement in this file, computed from the members' records, origin and crop, never the library: with r the fp32
record, o the cloud's origin and c the crop's center,
    x = double(r) + (o - c)  (the bracket first),  d2 = x0 x0 + x1 x1 + x2 x2,  keep iff finite(r) and min^2 <= d2 <= max^2
    y = double(r) + o,  inside iff lo <= y <= hi on every axis;  box mode 1 keeps inside, 2 keeps not inside.
The comparison is exact: kept equals the restatement's index list, and output record j is input record kept[j] bit for bit.  So that no
rounding decides membership (the device may contract d2 into fused multiply-adds), every test with random points first asserts, on the
restatement, that no point's d2 lies within 64 eps64 d2 of a bound (margin()); the lattice tests need no margin: their arithmetic is exact.

The members' records are known exactly: they are uploaded RELATIVE to a named origin (tests/test_cloud_merge_gpu.py: Member,
upload_relative), and come back exactly through records() / attributes() of that file."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import api
from test_cloud_merge_gpu import Member, attributes, records, upload_relative
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS64 = float(np.finfo(np.float64).eps)
INF = float("inf")
FAR = np.array([500e3, 4000e3, 0.0])
TILE = 2048
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4097, 133121)  # around a load of 64 and a tile of 2048; 66 tiles: a second look-back window


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------
def restate(rel, origin, min_range=0.0, max_range=INF, center=None, box=None, box_mode="inside"):
    """(indices kept, d2 of every record) in float64"""
    r = np.asarray(rel, dtype=F32).astype(np.float64).reshape(-1, 3)
    o = np.asarray(origin, dtype=np.float64)
    d = o - (np.zeros(3) if center is None else np.asarray(center, dtype=np.float64))  # the bracket, formed first
    with np.errstate(invalid="ignore", over="ignore"):
        x = r + d
        d2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
        keep = np.isfinite(r).all(axis=1) & (min_range * min_range <= d2) & (d2 <= max_range * max_range)
        if box is not None:
            y = r + o
            inside = ((np.asarray(box[0], dtype=np.float64) <= y) & (y <= np.asarray(box[1], dtype=np.float64))).all(axis=1)
            keep &= inside if box_mode == "inside" else ~inside
    return np.flatnonzero(keep).astype(np.int64), d2


def margin(d2, min_range=0.0, max_range=INF, **_):
    """no finite d2 within 64 eps64 d2 of a bound (if this ever fails: another seed, never a looser comparison)"""
    fin = d2[np.isfinite(d2)]
    for b in (min_range * min_range, max_range * max_range):
        if 0.0 < b < INF and len(fin):
            assert np.abs(fin - b).min() > 64 * EPS64 * b, b


def check_crop(rel, nrm, cov6, origin, out, kept, crop, exact=False):
    """the cropped cloud `out` and its indices `kept` against the restatement of the input (rel, nrm, cov6 at origin) under `crop`"""
    want, d2 = restate(rel, origin, **crop)
    if not exact:
        margin(d2, **crop)
    assert kept.dtype == np.int64 and np.array_equal(kept, want)
    assert out.size() == len(want)
    assert np.array_equal(out.origin(), np.asarray(origin, dtype=np.float64))  # the origin is kept
    if len(want) == 0:
        assert out._has() == (False, False) and out._box() is None  # an empty cloud without attributes
        return want
    assert out._has() == (nrm is not None, cov6 is not None)
    rec, _ = records(out)
    assert rec.tobytes() == np.ascontiguousarray(rel[want]).tobytes()  # bit for bit, the sign of a zero included
    nr, c6 = attributes(out)
    if nrm is not None:
        assert nr.tobytes() == np.ascontiguousarray(nrm[want]).tobytes()
    if cov6 is not None:
        assert c6.tobytes() == np.ascontiguousarray(cov6[want]).tobytes()
    lo, hi = out._box()
    assert np.array_equal(lo, rel[want].min(axis=0)) and np.array_equal(hi, rel[want].max(axis=0))  # the box of its records
    return want


def crop_member(m, **crop):
    out, kept = m.cloud.cropped(return_kept=True, **crop)
    return out, kept, check_crop(m.rel, m.nrm, m.cov6, m.origin, out, kept, crop)


def raw(cloud):
    n = cloud.size()
    hn, hc = cloud._has()
    xyz, nr, c6 = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros((n, 6), F32)
    api.check(sga.load().sga_cloud_download(cloud.ctx.h, cloud.h, api._fp(xyz), api._fp(nr) if hn else None, api._fp(c6) if hc else None))
    box = cloud._box()
    return (n, hn, hc, xyz.tobytes(), nr.tobytes(), c6.tobytes(), cloud.origin().tobytes(), None if box is None else (box[0].tobytes(), box[1].tobytes()))


@pytest.fixture(scope="module")
def big():
    """143 365 points uniform in +-50 m with normals and covariances (read only): 71 tiles"""
    return Member(143365, 7, spread=50.0)


# ---- exact set and order ------------------------------------------------------------------------------------------------------------------
def test_kept_is_the_restatement_and_the_records_are_the_inputs(big):
    assert np.array_equal(big.rel, np.random.default_rng(7).uniform(-50.0, 50.0, (143365, 3)).astype(F32))
    out, kept, want = crop_member(big, min_range=10.0, max_range=45.0)
    assert 50000 < len(want) < 60000
    # w = 0 .. m - 1 in storage order: the kd-tree's view returns the points with their index words
    _, _, _, pts, order = sga.KdTree(out)._tree()
    assert np.array_equal(np.sort(order), np.arange(len(want)))
    back = np.empty((len(want), 3), F32)
    back[order] = pts
    assert back.tobytes() == np.ascontiguousarray(big.rel[want]).tobytes()  # index word j sits on record j
    # without kept: the same cloud
    assert raw(big.cloud.cropped(10.0, 45.0)) == raw(out)
    # ranges with a center and a box, inside and outside
    crop_member(big, min_range=5.0, max_range=30.0, center=(10.0, -20.0, 5.0))
    crop_member(big, max_range=60.0, box=((-20.0, -30.0, -5.0), (25.0, 10.0, 40.0)))
    crop_member(big, min_range=10.0, max_range=45.0, box=((-3.0, -2.0, -2.0), (3.0, 2.0, 2.0)), box_mode="outside")
    crop_member(big, box=((-INF, -INF, 0.0), (INF, 0.0, INF)))  # infinite bounds are fine


# ---- boundaries, where the arithmetic is exact -------------------------------------------------------------------------------------------
def lattice():
    g = np.arange(-8, 9, dtype=F32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def test_range_bounds_are_closed():
    rel = lattice()
    cloud = upload_relative(rel, None, None, np.zeros(3))
    crop = dict(min_range=3.0, max_range=5.0)
    out, kept = cloud.cropped(return_kept=True, **crop)
    want = check_crop(rel, None, None, np.zeros(3), out, kept, crop, exact=True)
    d2 = (rel.astype(np.float64) ** 2).sum(axis=1)
    got = np.zeros(len(rel), bool)
    got[kept] = True
    for value, inside in ((9.0, True), (25.0, True), (8.0, False), (26.0, False)):
        assert (d2 == value).sum() > 0 and np.all(got[d2 == value] == inside), value
    assert len(want) == ((d2 >= 9.0) & (d2 <= 25.0)).sum()
    # a center on the lattice: the same rule about it
    crop = dict(min_range=3.0, max_range=5.0, center=(2.0, -1.0, 3.0))
    out, kept = cloud.cropped(return_kept=True, **crop)
    check_crop(rel, None, None, np.zeros(3), out, kept, crop, exact=True)


def test_box_bounds_are_closed():
    rel = lattice()
    cloud = upload_relative(rel, None, None, np.zeros(3))
    lo, hi = np.array([-2.0, -3.0, 0.0]), np.array([4.0, 1.0, 5.0])
    r = rel.astype(np.float64)
    inside = ((lo <= r) & (r <= hi)).all(axis=1)
    on_face = inside & ((r == lo) | (r == hi)).any(axis=1)
    assert on_face.sum() > 100
    for mode, keeps_faces in (("inside", True), ("outside", False)):
        crop = dict(box=(lo, hi), box_mode=mode)
        out, kept = cloud.cropped(return_kept=True, **crop)
        check_crop(rel, None, None, np.zeros(3), out, kept, crop, exact=True)
        got = np.zeros(len(rel), bool)
        got[kept] = True
        assert np.all(got[on_face] == keeps_faces), mode
        assert kept.size == (inside.sum() if mode == "inside" else (~inside).sum())
    # a lattice away from the origin of its frame: y = r + o is still exact
    o = np.array([128.0, -256.0, 0.0])
    far = upload_relative(rel, None, None, o)
    crop = dict(min_range=3.0, max_range=5.0, center=o + (1.0, 0.0, -2.0), box=(o + lo, o + hi), box_mode="outside")
    out, kept = far.cropped(return_kept=True, **crop)
    check_crop(rel, None, None, o, out, kept, crop, exact=True)


# ---- sizes and keep patterns --------------------------------------------------------------------------------------------------------------
def placed(n, keep, seed):
    """n points whose membership under ranges (10, 45) is `keep`: kept ones at radius 15 .. 40, the others at 1 .. 8 or 50 .. 80"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)
    near = rng.random(n) < 0.5
    radius = np.where(keep, rng.uniform(15.0, 40.0, n), np.where(near, rng.uniform(1.0, 8.0, n), rng.uniform(50.0, 80.0, n)))
    return (v * radius[:, None]).astype(F32)


def patterns(n, seed):
    i = np.arange(n)
    yield "all", np.ones(n, bool)
    yield "none", np.zeros(n, bool)
    yield "first only", i == 0
    yield "last only", i == n - 1
    yield "every other", i % 2 == 0
    yield "random half", np.random.default_rng(seed).random(n) < 0.5
    if n > 3 * TILE:  # whole tiles dropped in the middle: zero aggregates are looked back over (66 tiles: across a whole window of 64)
        yield "middle tiles dropped", (i < TILE) | (i >= (n // TILE) * TILE)
        yield "one point per tile", i % TILE == 77 % min(n, TILE)


@pytest.mark.parametrize("n", SIZES)
def test_every_size_and_keep_pattern(n):
    crop = dict(min_range=10.0, max_range=45.0)
    for label, keep in patterns(n, 100 + n):
        rel = placed(n, keep, 200 + n)
        cloud = upload_relative(rel, None, None, np.zeros(3))
        out, kept = cloud.cropped(return_kept=True, **crop)
        want = check_crop(rel, None, None, np.zeros(3), out, kept, crop)
        assert np.array_equal(want, np.flatnonzero(keep)), label  # the points were placed as meant


# ---- attributes ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normals,covs", [(False, False), (True, False), (False, True), (True, True)])
def test_attributes_follow_their_points(normals, covs):
    m = Member(4097, 300 + 2 * normals + covs, normals=normals, covs=covs, spread=30.0)
    crop_member(m, min_range=12.0, max_range=35.0)
    crop_member(m, box=((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0)), box_mode="outside")


# ---- non-finite records --------------------------------------------------------------------------------------------------------------------
def test_non_finite_records_are_dropped_in_every_mode():
    m = Member(5000, 400, spread=30.0)
    rel, bad = m.rel.copy(), []
    rng = np.random.default_rng(401)
    for j, value in enumerate((np.nan, np.inf, -np.inf) * 40):
        i = int(rng.integers(0, len(rel)))
        rel[i, j % 3] = value
        bad.append(i)
    rel[0], rel[-1] = (np.nan, np.nan, np.nan), (np.inf, -np.inf, 1.0)
    rel[2048] = (0.0, np.inf, 0.0)  # an infinite d2, not a NaN: max_range = +inf must not keep it
    bad = np.unique(bad + [0, len(rel) - 1, 2048])
    cloud = upload_relative(rel, m.nrm, m.cov6, m.origin)
    good = np.setdiff1d(np.arange(len(rel)), bad)
    # the default crop: "remove the non-finite points" — everything else is kept bit for bit
    out, kept = cloud.cropped(return_kept=True)
    assert np.array_equal(check_crop(rel, m.nrm, m.cov6, m.origin, out, kept, {}), good)
    # box mode 2 keeps the finite points that are not inside: a NaN is not inside, and is dropped all the same
    crop = dict(box=((-5.0, -5.0, -5.0), (5.0, 5.0, 5.0)), box_mode="outside")
    out, kept = cloud.cropped(return_kept=True, **crop)
    want = check_crop(rel, m.nrm, m.cov6, m.origin, out, kept, crop)
    assert not np.intersect1d(want, bad).size and len(want) > 4000
    crop = dict(box=((-INF, -INF, -INF), (INF, INF, INF)))
    out, kept = cloud.cropped(return_kept=True, **crop)
    assert np.array_equal(check_crop(rel, m.nrm, m.cov6, m.origin, out, kept, crop), good)
    # a cloud of nothing but non-finite points
    none = upload_relative(np.full((70, 3), np.nan, F32), None, None, np.zeros(3))
    out, kept = none.cropped(return_kept=True)
    assert out.size() == 0 and kept.size == 0 and out._has() == (False, False)


# ---- a frame far from the origin -----------------------------------------------------------------------------------------------------------
def test_far_frame_forms_the_offset_first():
    m = Member(6000, 500, origin=FAR, spread=40.0)
    center = FAR + (2.0, 3.0, 6.0)  # 7 m from the origin of the frame
    crop_member(m, min_range=8.0, max_range=33.0, center=center)
    crop_member(m, max_range=50.0, center=center, box=(FAR + (-10.0, -20.0, -30.0), FAR + (30.0, 20.0, 10.0)))
    # ranges measured from the caller's origin: everything is 4 000 km away
    out, kept = m.cloud.cropped(max_range=1000.0, return_kept=True)
    assert out.size() == 0 and kept.size == 0
    out, kept = m.cloud.cropped(min_range=1000.0, return_kept=True)
    assert out.size() == m.n


# ---- the batch ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eight():
    """B = 8 (read only): sizes 1 .. 6000 and an empty member, every attribute combination, a member made by a second context, a member far
    from the origin, a member that loses everything, crops that differ"""
    ctx2 = sga.Context(0)
    members = [Member(1, 601, spread=30.0), Member(2049, 602, spread=30.0), Member(0, 603), Member(4097, 604, covs=False, spread=30.0), Member(300, 605, normals=False, origin=FAR, spread=30.0),
               Member(6000, 606, ctx=ctx2, spread=30.0), Member(2048, 607, normals=False, covs=False, spread=30.0), Member(65, 608, spread=30.0)]
    crops = [dict(), dict(min_range=10.0, max_range=30.0), dict(min_range=1.0), dict(box=((-10.0, -10.0, -10.0), (10.0, 10.0, 10.0)), box_mode="outside"), dict(max_range=25.0, center=FAR + (1.0, 2.0, 3.0)),
             dict(min_range=5.0, max_range=28.0, center=(3.0, -4.0, 1.0), box=((-20.0, -20.0, -20.0), (20.0, 25.0, 15.0))), dict(min_range=500.0), dict(max_range=35.0)]
    return members, crops


@pytest.mark.parametrize("B", [1, 2, 8])
def test_batch_members_equal_their_lone_calls(eight, B):
    members, crops = eight
    pick = {1: [5], 2: [2, 6], 8: list(range(8))}[B]
    before = sga.cloud_crop_launches()
    outs, kepts = sga.crop_clouds([members[j].cloud for j in pick], [crops[j] for j in pick], return_kept=True)
    launches = sga.cloud_crop_launches() - before
    assert launches == (2 if any(members[j].n for j in pick) else 0), launches  # one table copy and ONE kernel whatever B is (the single-pass form)
    for j, out, kept in zip(pick, outs, kepts):
        m = members[j]
        check_crop(m.rel, m.nrm, m.cov6, m.origin, out, kept, crops[j])
        lone, lone_kept = m.cloud.cropped(return_kept=True, **crops[j])
        assert raw(lone) == raw(out) and np.array_equal(lone_kept, kept), j
    assert outs[pick.index(6)].size() == 0 if 6 in pick else True  # the member that loses everything
    # without kept, and with one crop for all
    plain = sga.crop_clouds([members[j].cloud for j in pick], [crops[j] for j in pick])
    assert [raw(a) for a in plain] == [raw(b) for b in outs]
    if B == 8:
        near = [j for j in pick if not members[j].origin.any()]
        shared = sga.crop_clouds([members[j].cloud for j in near], dict(min_range=10.0, max_range=30.0))
        for j, out in zip(near, shared):
            assert raw(out) == raw(members[j].cloud.cropped(10.0, 30.0)), j


def test_launch_count_is_two_whatever_the_count_and_a_stream_ordered_context_waits_too(eight):
    members, crops = eight
    blocking = sga.crop_clouds([m.cloud for m in members], crops)
    ctx = sga.Context(0)
    ctx.set_stream_ordered(True)
    counts = []
    for pick in ([5], list(range(8))):
        before = sga.cloud_crop_launches()
        outs, kepts = sga.crop_clouds([members[j].cloud for j in pick], [crops[j] for j in pick], return_kept=True, ctx=ctx)
        counts.append(sga.cloud_crop_launches() - before)
        for j, o, k in zip(pick, outs, kepts):
            assert raw(o) == raw(blocking[j]), j  # the box included: the count has to reach the host, the box comes with it
            assert np.array_equal(k, restate(members[j].rel, members[j].origin, **crops[j])[0])
    assert counts == [2, 2], counts
    ctx.set_stream_ordered(False)
    before = sga.cloud_crop_launches()
    empty = sga.crop_clouds([members[2].cloud], [crops[2]])
    assert sga.cloud_crop_launches() == before and empty[0].size() == 0  # an empty member takes no workgroups: no device work
    members[1].cloud.selected([0, 1, 2])
    assert sga.cloud_crop_launches() == before  # a gather is not a crop


# ---- the device form -----------------------------------------------------------------------------------------------------------------------
def test_device_kept_equals_host_kept():
    """(the first test of a run that puts a tensor on the device also pays torch's start-up there, about ten seconds)"""
    import torch

    rng = np.random.default_rng(700)
    xyz = rng.uniform(-40.0, 40.0, (5000, 3)).astype(F32)
    cloud = sga.PointCloud.from_torch(torch.from_numpy(xyz).to("cuda:0"), origin=(0.0, 0.0, 0.0), relative=True)
    crop = dict(min_range=10.0, max_range=35.0, box=((-30.0, -30.0, -5.0), (30.0, 30.0, 30.0)))
    host, host_kept = cloud.cropped(return_kept=True, **crop)
    check_crop(xyz, None, None, np.zeros(3), host, host_kept, crop)
    before = sga.cloud_crop_launches()
    dev, dev_kept = cloud.cropped(return_kept=True, stream=torch.cuda.current_stream(), **crop)
    assert sga.cloud_crop_launches() - before == 2
    assert isinstance(dev_kept, torch.Tensor) and dev_kept.dtype == torch.int64 and dev_kept.is_cuda
    assert np.array_equal(dev_kept.cpu().numpy(), host_kept)
    assert raw(dev) == raw(host)
    assert raw(cloud.cropped(stream=torch.cuda.current_stream(), **crop)) == raw(host)  # without kept
    # the indices serve on the device: a side channel follows its points without touching the host
    side = torch.arange(5000, device="cuda:0", dtype=torch.float32) * 0.5
    assert np.array_equal(side[dev_kept].cpu().numpy(), 0.5 * host_kept.astype(F32))
    # host memory handed over as device memory is refused
    lib, h = sga.load(), C.c_void_p()
    pageable = np.empty(5000, np.int64)
    rc = lib.sga_cloud_crop_device(cloud.ctx.h, cloud.h, C.byref(api._crop(**crop)), C.c_void_p(pageable.ctypes.data), None, 0, C.byref(h))
    assert rc == 1 and "d_kept" in lib.sga_last_error().decode() and h.value is None


# ---- downstream: a cropped cloud is an ordinary cloud ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("origin", [(0.0, 0.0, 0.0), (1024.0, -640.0, 0.0)])
def test_voxelgrid_of_the_cropped_cloud_equals_that_of_a_twin(origin):
    """voxelgrid_sampling of the cropped cloud against that of a twin uploaded relative to the same origin from input[kept]: the same
    records and the same box in (the short keys come from it), the same voxels out, bit for bit — the spare room of the cropped cloud's
    arrays is nobody's business"""
    o = np.array(origin)
    m = Member(20000, 800, origin=o, spread=30.0)
    crop = dict(min_range=6.0, max_range=25.0, center=o)
    out, kept, want = crop_member(m, **crop)
    twin = upload_relative(m.rel[want], m.nrm[want], m.cov6[want], o)
    assert raw(out) == raw(twin)
    assert out._voxelgrid_plan(0.5) == twin._voxelgrid_plan(0.5) and out._voxelgrid_plan(0.5)["box"]
    a, b = sga.voxelgrid_sampling(out, 0.5), sga.voxelgrid_sampling(twin, 0.5)
    assert a.size() > 1000 and raw(a) == raw(b)
    ta, tb = sga.KdTree(out), sga.KdTree(twin)
    (da, tha, axa, pa, oa), (db, thb, axb, pb, ob) = ta._tree(), tb._tree()
    assert da == db and np.array_equal(tha[1:], thb[1:]) and np.array_equal(axa[1:], axb[1:]) and np.array_equal(pa, pb) and np.array_equal(oa, ob)
    # a cropped raw sweep can be deskewed: the times follow the points
    times = np.random.default_rng(801).uniform(0.0, 1.0, m.n).astype(F32)
    xi = np.array([0.0, 0.0, 0.02, 1.0, 0.1, 0.0])
    assert raw(out.deskewed(times[kept], xi)) == raw(twin.deskewed(times[want], xi))


# ---- select -----------------------------------------------------------------------------------------------------------------------------------
def check_select(m, idx):
    idx = np.asarray(idx, dtype=np.int64)
    out = m.cloud.selected(idx)
    assert out.size() == len(idx) and np.array_equal(out.origin(), m.origin)
    if len(idx) == 0:
        assert out._has() == (False, False)
        return out
    assert out._has() == (m.nrm is not None, m.cov6 is not None)
    rec, _ = records(out)
    assert rec.tobytes() == np.ascontiguousarray(m.rel[idx]).tobytes()
    nr, c6 = attributes(out)
    if m.nrm is not None:
        assert nr.tobytes() == np.ascontiguousarray(m.nrm[idx]).tobytes()
    if m.cov6 is not None:
        assert c6.tobytes() == np.ascontiguousarray(m.cov6[idx]).tobytes()
    return out


def test_select_gathers_in_the_order_given():
    rng = np.random.default_rng(900)
    for m in (Member(3000, 901), Member(1000, 902, normals=False), Member(257, 903, covs=False, origin=(128.0, -256.0, 0.0)), Member(64, 904, normals=False, covs=False)):
        check_select(m, rng.permutation(m.n))  # a permutation
        check_select(m, rng.integers(0, m.n, 2 * m.n + 3))  # repeats, more indices than points
        check_select(m, [m.n - 1] * 5 + [0])
        check_select(m, [])
    m = Member(3000, 901)
    out = check_select(m, np.arange(m.n)[::-1])
    _, _, _, pts, order = sga.KdTree(out)._tree()  # w is the new index
    back = np.empty((m.n, 3), F32)
    back[order] = pts
    assert np.array_equal(np.sort(order), np.arange(m.n)) and back.tobytes() == np.ascontiguousarray(m.rel[::-1]).tobytes()
    for bad, where in (([0, 1, 2, m.n], "indices[3]"), ([-1], "indices[0]"), ([5, 2**40], "indices[1]")):
        with pytest.raises(sga.SgaError, match=where.replace("[", r"\[").replace("]", r"\]")):
            m.cloud.selected(bad)


def test_random_sampling_returns_input_records_in_input_order():
    m = Member(5000, 910)
    for count, seed in ((1, 1), (500, 2), (4999, 3)):
        out = sga.random_sampling(m.cloud, count, seed)
        idx = sga.random_sampling_indices(m.n, count, seed)
        assert out.size() == count and len(np.unique(idx)) == count and np.all(np.diff(idx) > 0)
        rec, _ = records(out)
        assert rec.tobytes() == np.ascontiguousarray(m.rel[idx]).tobytes()
        assert raw(out) == raw(sga.random_sampling(m.cloud, count, seed))
    assert sga.random_sampling(m.cloud, 5000) is m.cloud and sga.random_sampling(m.cloud, 6000, 1) is m.cloud  # num_samples >= n: the cloud as it is
    assert sga.random_sampling(m.rel, 100, 4).size() == 100  # an array goes through PointCloud, as voxelgrid_sampling's does


# ---- the driver -------------------------------------------------------------------------------------------------------------------------------
def test_odometry_with_ranges_that_drop_nothing_is_the_odometry():
    from small_gicp_amd import odometry

    plain = odometry.run_synthetic(4)
    before = sga.cloud_crop_launches()
    again = odometry.run_synthetic(4)
    assert sga.cloud_crop_launches() == before  # both None: no new call is made
    cropped = odometry.run_synthetic(4, min_range=0.0, max_range=INF)
    assert sga.cloud_crop_launches() - before == 2 * 4
    for a, b, c in zip(plain["estimated"], again["estimated"], cropped["estimated"]):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_odometry_on_cropped_sweeps_completes():
    from small_gicp_amd import odometry, synthetic

    pts, times = synthetic.kitti_like_sweep(1)[:2]
    cloud = sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=F32))
    out, kept = cloud.cropped(4.0, 30.0, return_kept=True)
    want, d2 = restate(pts[:, :3], np.zeros(3), 4.0, 30.0)
    margin(d2, 4.0, 30.0)
    assert np.array_equal(kept, want) and 0 < len(want) < len(pts)
    print("frame 0: %d points, %d nearer than 4 m and %d farther than 30 m dropped" % (len(pts), (d2 < 16.0).sum(), (d2 > 900.0).sum()))
    res = odometry.run_synthetic(4, sweeps=True, min_range=4.0, max_range=30.0)
    assert all(np.isfinite(T).all() for T in res["estimated"]) and len(res["estimated"]) == 4
    print("run_synthetic(4, sweeps=True, min_range=4, max_range=30): ate_trans_m_max %.4f" % res["ate_trans_m_max"])


# ---- the C++ header ---------------------------------------------------------------------------------------------------------------------------
def test_cpp_crop_clouds(tmp_path):
    """include/small_gicp_amd.hpp: crop_clouds, PointCloud::cropped with kept and PointCloud::selected against a host loop
    (tests/cpp/test_cpp_cloud_crop.cpp, compiled with g++ as test_cloud_deskew_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_crop"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_crop.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = sga.synthetic.kitti_like_scan(0)
    (tmp_path / "p.f32").write_bytes(np.ascontiguousarray(pts[::6, :3], dtype=F32).tobytes())  # every sixth point: the whole scan, thinned
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    crop = [r for r in rows if r[0] == "CROP"]
    assert len(crop) == 4 and all(r[7] == "1" and r[9] == "0" for r in crop), crop
    assert all(0 < int(r[3]) < int(r[5]) for r in crop[:2]) and int(crop[3][3]) == 0  # members that keep part, one that keeps nothing
    for label in ("LONE", "SELECT"):
        got = [r for r in rows if r[0] == label]
        assert len(got) == 4 and all(r[3] == "1" for r in got), got
    assert ["REFUSE", "equal", "1"] in rows

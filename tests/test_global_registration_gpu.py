"""Global registration on the device (csrc/cloud_fpfh.hip, feature_match.hip, ransac.hip) against the float64
restatement of tests/global_ref.py, which never goes through the library.

The comparison rule.  Every restatement marks its band — what an ulp of double arithmetic can change (global_ref.py says how) — and
every test first asserts ON THE RESTATEMENT that the band holds at most 1 % of the points, rows or pairs (if it ever fails: another
seed, never a looser comparison).  Outside the band:
  FPFH      every value within 1 fp32 ulp of the restatement rounded to fp32 (the double arithmetic differs by about (k + 40) eps64
            relative, far below 2^-24: only a rounding tie can move a value); every sub-histogram of EVERY row sums to 100 within 33
            fp32 ulps or is zero; two calls give the same bytes.
  matching  the winners are the restatement's, dist within 64 D eps64 relative, the mutual result equal.
  RANSAC    best_hypothesis draws the restatement's triple and scores the restatement's count up to that hypothesis' band count; no
            hypothesis of the restatement scores above it; scored is equal up to the hypotheses with a test at its limit; the refit
            pose against numpy's Kabsch over the same inliers within REFIT_TOL (measured on the MI355X: see below).
Refit tolerance: the greatest deviation measured on the MI355X over the planted cases of this file was 1.52e-10 m (on the origin
256 km away: an ulp of such a coordinate is 3e-11 m; 2.4e-15 m near the origin) and 7.04e-16 rad; 100 x that
is allowed, and the bound must stay below 1e-6 m and 1e-6 rad."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import global_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import api, synthetic
from conftest import ROOT
from test_cloud_merge_gpu import attributes, records, upload_relative

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = np.zeros(3)
WAVE_DEFAULT = 81920
REFIT_TOL_M, REFIT_TOL_RAD = 100 * 1.52e-10, 100 * 7.04e-16
ULP100 = 7.62939453125e-06  # one fp32 ulp at 100


class Route:
    """every call inside takes the wave-per-query route (True) or the lane-per-query route (False)"""

    def __init__(self, wave):
        self.wave = wave

    def __enter__(self):
        sga.load().sga_set_knn_wave_max(C.c_longlong(1 << 40 if self.wave else 0))

    def __exit__(self, *exc):
        sga.load().sga_set_knn_wave_max(C.c_longlong(WAVE_DEFAULT))


def rigid(axis, angle, t):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


# ---- FPFH ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def terrain(n, seed=3):
    """n points of a 12 m x 12 m piece of the bumpy terrain with unit normals that lean away from +z and point up or down at random"""
    p = synthetic.bumpy_terrain(20 * max(n, 50), seed)
    p = p[(np.abs(p[:, 0]) < 6) & (np.abs(p[:, 1]) < 6)][:n]
    assert len(p) == n
    rng = np.random.default_rng(100 + seed)
    v = np.array([0.0, 0.0, 1.0]) + 0.6 * rng.normal(size=(n, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.choice([-1.0, 1.0], n)[:, None]
    p, v = np.ascontiguousarray(p, dtype=F32), np.ascontiguousarray(v, dtype=F32)
    p.setflags(write=False)
    v.setflags(write=False)
    return p, v


@functools.lru_cache(maxsize=None)
def fpfh_reference(n, k, viewpoint):
    p, v = terrain(n)
    return ref.fpfh(p, v, k, viewpoint)


def ulps(a, b):
    """distance in fp32 ulps between non-negative fp32 arrays"""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def check_fpfh(got, want, what):
    n = len(want["rows"])
    band = want["band"]
    assert band.sum() <= 0.01 * n, (what, "the restatement has %d of %d points in the band" % (band.sum(), n))
    assert got.shape == (n, 33) and got.dtype == F32, what
    assert np.isfinite(got).all() and (got >= 0).all(), what
    want32 = want["rows"].astype(F32)
    off = ulps(got[~band], want32[~band])
    sums = np.stack([got[:, o:o + 11].astype(np.float64).sum(axis=1) for o in (0, 11, 22)], axis=1)
    print("%s: n %d, band %d, greatest distance %d ulp, values off by one ulp %d of %d, sub-histogram sums within %.2e of 100" % (
        what, n, band.sum(), off.max() if off.size else 0, (off == 1).sum(), off.size, np.abs(sums[sums != 0] - 100).max() if (sums != 0).any() else 0.0))
    assert off.size == 0 or off.max() <= 1, (what, np.argwhere(ulps(got, want32) > 1)[:5])
    assert np.all((sums == 0) | (np.abs(sums - 100.0) <= 33 * ULP100)), what
    zero = want["rows"].reshape(n, 3, 11).sum(axis=2) == 0
    assert np.array_equal((sums == 0)[~band], zero[~band]), what


@pytest.mark.parametrize("wave", [True, False], ids=["wave", "lane"])
@pytest.mark.parametrize("n", [1, 2, 10, 11, 63, 64, 65, 2000])  # k and k + 1 with k = 10; a wave and its neighbours; many workgroups
def test_fpfh_sizes_on_both_routes(n, wave):
    p, v = terrain(n)
    cloud = upload_relative(p, v, None, ZERO)
    for viewpoint in ((0.0, 0.0, 50.0), None):
        with Route(wave):
            f = cloud.fpfh(None, 10, viewpoint)
        assert f.size() == n and f.dim == 33
        check_fpfh(f.numpy(), fpfh_reference(n, 10, viewpoint), "n %d, %s route, viewpoint %s" % (n, "wave" if wave else "lane", viewpoint))
    if n == 1:
        assert not f.numpy().any()  # a zero row


@pytest.mark.parametrize("k", [2, 20, 63])
def test_fpfh_neighbourhood_sizes(k):
    p, v = terrain(2000)
    cloud = upload_relative(p, v, None, ZERO)
    tree = sga.KdTree(cloud)
    got = {}
    for wave in (True, False):
        with Route(wave):
            got[wave] = cloud.fpfh(tree, k, (0.0, 0.0, 50.0)).numpy()
        check_fpfh(got[wave], fpfh_reference(2000, k, (0.0, 0.0, 50.0)), "k %d, %s route" % (k, "wave" if wave else "lane"))
    band = fpfh_reference(2000, k, (0.0, 0.0, 50.0))["band"]
    assert ulps(got[True][~band], got[False][~band]).max() <= 1  # the routes list the same neighbours in another order


def test_fpfh_on_a_far_origin_and_with_a_temporary_tree():
    # coordinates on a 2^-10 m lattice: about an origin 1280 m away the records are the near cloud's exactly, so the rows are the same bytes
    p, v = terrain(2000)
    near = (np.round(p.astype(np.float64) * 1024.0) / 1024.0).astype(F32)
    want = ref.fpfh(near, v, 20, (3.0, -2.0, 40.0))
    a = upload_relative(near, v, None, ZERO)
    origin = np.array([1280.0, -2560.0, 128.0])
    b = upload_relative(near, v, None, origin)
    rows_a = a.fpfh(sga.KdTree(a), 20, (3.0, -2.0, 40.0)).numpy()
    rows_b = b.fpfh(None, 20, origin + (3.0, -2.0, 40.0)).numpy()
    check_fpfh(rows_a, want, "near")
    assert rows_a.tobytes() == rows_b.tobytes()
    assert np.array_equal(attributes(a)[0], v)  # the viewpoint wrote nothing back


def test_fpfh_two_calls_give_the_same_bytes_and_the_launches_do_not_grow():
    p, v = terrain(2000)
    cloud = upload_relative(p, v, None, ZERO)
    tree = sga.KdTree(cloud)
    for wave in (True, False):
        with Route(wave):
            before = sga.cloud_fpfh_launches()
            a = cloud.fpfh(tree, 20).numpy()
            count = sga.cloud_fpfh_launches() - before
            b = cloud.fpfh(tree, 20).numpy()
        assert a.tobytes() == b.tobytes()
        assert count == 3
    small = upload_relative(p[:65], v[:65], None, ZERO)
    before = sga.cloud_fpfh_launches()
    small.fpfh(None, 20)
    assert sga.cloud_fpfh_launches() - before == 3  # whatever the size
    before = sga.cloud_fpfh_launches()
    empty = sga.PointCloud(np.zeros((0, 3), F32)).fpfh()
    assert empty.size() == 0 and empty.dim == 33 and empty.numpy().shape == (0, 33) and sga.cloud_fpfh_launches() == before


def test_fpfh_refusals():
    p, v = terrain(2000)
    cloud = upload_relative(p, v, None, ZERO)
    before = sga.cloud_fpfh_launches()
    with pytest.raises(sga.SgaError, match="needs a cloud with normals"):
        upload_relative(p, None, None, ZERO).fpfh()
    with pytest.raises(sga.SgaError, match="index was built over a cloud of 1999 points, got 2000"):
        cloud.fpfh(sga.KdTree(upload_relative(p[:1999], v[:1999], None, ZERO)))
    with pytest.raises(sga.SgaError, match="device frames differ"):
        cloud.fpfh(sga.KdTree(upload_relative(p, v, None, np.array([128.0, 0.0, 0.0]))))
    bad = p.copy()
    bad[17, 1] = np.nan
    with pytest.raises(sga.SgaError, match="contains non-finite coordinates"):
        upload_relative(bad, v, None, ZERO).fpfh()
    with pytest.raises(sga.SgaError, match=r"k must be in \[2,63\]"):
        cloud.fpfh(None, 64)
    assert sga.cloud_fpfh_launches() == before  # nothing was enqueued


# ---- matching -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows(n, D, seed):
    r = np.random.default_rng(seed).uniform(0, 100, (n, D)).astype(F32)
    r.setflags(write=False)
    return r


def check_match(A, B, mutual, what):
    want = ref.match(A, B, mutual)
    n, D = len(A), A.shape[1]
    assert want["band"].sum() <= 0.01 * n, (what, "the restatement has %d of %d rows in the band" % (want["band"].sum(), n))
    fa, fb = sga.Features.from_array(A), sga.Features.from_array(B)
    match, dist = np.full(n, -5, np.int64), np.full(n, -5.0)
    cnt = C.c_size_t(12345)
    api.check(sga.load().sga_features_match(fa.ctx.h, fa.h, fb.h, 1 if mutual else 0, match.ctypes.data_as(C.POINTER(C.c_int64)), api._dp(dist), C.byref(cnt)))
    good = ~want["band"]
    assert np.array_equal(match[good], want["match"][good]), (what, np.flatnonzero(match != want["match"])[:5])
    assert cnt.value == (match >= 0).sum()
    has = good & (want["match"] >= 0)
    assert np.all(np.abs(dist[has] - want["dist"][has]) <= 64 * D * ref.EPS * want["dist"][has]), what
    assert np.all(np.isinf(dist[match < 0])) and np.all(np.isfinite(dist[match >= 0])), what
    again = np.empty(n, np.int64)
    dist2 = np.empty(n)
    api.check(sga.load().sga_features_match(fa.ctx.h, fa.h, fb.h, 1 if mutual else 0, again.ctypes.data_as(C.POINTER(C.c_int64)), api._dp(dist2), None))
    assert again.tobytes() == match.tobytes() and dist2.tobytes() == dist.tobytes(), what  # two calls are identical
    return match


@pytest.mark.parametrize("mutual", [False, True], ids=["one-way", "mutual"])
def test_matching_sizes(mutual):
    for n in (1, 63, 64, 65, 1000):
        for m in (1, 63, 64, 65, 1000):
            check_match(rows(n, 33, 1), rows(m, 33, 2), mutual, "n %d m %d" % (n, m))


@pytest.mark.parametrize("D", [1, 7, 33, 128])
def test_matching_dimensions_and_duplicate_rows(D):
    A, B = rows(300, D, 3).copy(), rows(1000, D, 4).copy()
    B[500], B[7], B[999] = B[3], B[3], B[40]  # equal rows: the lowest index wins
    A[0], A[1], A[299] = B[3], B[40], B[999]  # at distance 0
    for mutual in (False, True):
        match = check_match(A, B, mutual, "D %d mutual %d" % (D, mutual))
        if D > 1:
            assert match[0] == 3 and match[1] == 40 or mutual
    f = sga.Features.from_array(B)
    assert f.size() == 1000 and f.dim == D and f.numpy().tobytes() == B.tobytes()


def test_matching_an_empty_side_and_the_launches():
    A = rows(65, 33, 5)
    fa, none = sga.Features.from_array(A), sga.Features.from_array(np.zeros((0, 33), F32))
    before = sga.features_match_launches()
    pairs, dist = sga.match_features(fa, none, mutual=True, return_dist=True)
    assert pairs.shape == (0, 2) and pairs.dtype == np.int64 and dist.shape == (0,)
    assert sga.match_features(none, fa).shape == (0, 2)
    assert sga.features_match_launches() == before  # nothing is launched
    pairs = sga.match_features(fa, fa, mutual=False)
    assert sga.features_match_launches() - before == 2 and np.array_equal(pairs, np.stack([np.arange(65), np.arange(65)], axis=1))
    before = sga.features_match_launches()
    pairs, dist = sga.match_features(fa, sga.Features.from_array(rows(1000, 33, 6)), mutual=True, return_dist=True)
    assert sga.features_match_launches() - before == 3
    want = ref.match(A, rows(1000, 33, 6), True)
    assert np.array_equal(pairs[:, 0], np.flatnonzero(want["match"] >= 0)) and np.array_equal(pairs[:, 1], want["match"][want["match"] >= 0])
    with pytest.raises(sga.SgaError, match="the source rows have 33 values, the target rows 7"):
        sga.match_features(fa, sga.Features.from_array(rows(10, 7, 1)))


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------------
T_PLANTED = rigid([0.3, -0.2, 0.9], 2.0, [4.0, -3.0, 1.0])


@functools.lru_cache(maxsize=None)
def planted(M=200, share=0.3, seed=9, origin=(0.0, 0.0, 0.0)):
    """source cloud (300), target cloud (320), M pairs of which the first share * M follow T_PLANTED (noise 0.01 m) and the rest are clutter;
    the pairs name points all over both clouds"""
    rng = np.random.default_rng(seed)
    src = rng.uniform(-15, 15, (300, 3)).astype(F32)
    tgt = rng.uniform(-15, 15, (320, 3)).astype(F32)
    pairs = np.stack([rng.permutation(300)[:M], rng.permutation(320)[:M]], axis=1).astype(np.int64)
    good = int(share * M)
    o = np.asarray(origin, dtype=np.float64)
    moved = (src[pairs[:good, 0]].astype(np.float64) + o) @ T_PLANTED[:3, :3].T + T_PLANTED[:3, 3] + rng.normal(0, 0.01, (good, 3))
    tgt[pairs[:good, 1]] = (moved - o).astype(F32)
    return src, tgt, pairs


def check_ransac(src, tgt, pairs, origin=ZERO, what="", **params):
    o = np.asarray(origin, dtype=np.float64)
    ps, pt = src[pairs[:, 0]].astype(np.float64) + o, tgt[pairs[:, 1]].astype(np.float64) + o
    p = dict(max_distance=0.1, iterations=4096, seed=0, edge_similarity=0.9, min_edge=0.0)
    p.update(params)
    want = ref.ransac(ps, pt, **p)
    cs, ct = upload_relative(src, None, None, o), upload_relative(tgt, None, None, o)
    got = sga.ransac_correspondences(cs, ct, pairs, **p)
    again = sga.ransac_correspondences(cs, ct, pairs, **p)
    assert all(np.array_equal(got[w], again[w]) for w in got), what  # two calls are identical
    h = got["best_hypothesis"]
    shaky = int(want["shaky"].sum())
    assert want["band"].max() <= 0.01 * len(pairs) and shaky <= 0.01 * p["iterations"], (what, "the restatement's band", want["band"].max(), shaky)
    assert abs(got["scored"] - int(want["valid"].sum())) <= shaky, what
    assert want["valid"][h] or want["shaky"][h], what
    assert abs(got["inliers"] - want["score"][h]) <= want["band"][h], (what, got["inliers"], want["score"][h])
    assert np.all(want["score"] <= got["inliers"] + want["band"]), what  # nobody scores above the winner
    b = want["best"]
    lead = want["score"][b] - np.where(np.arange(len(want["score"])) == b, -1, want["score"])
    if np.all(lead > want["band"] + want["band"][b]) or (want["band"].max() == 0 and shaky == 0):
        assert h == b, (what, h, b)  # (equal scores without a band: the lowest h, on both sides)
    # the pose: the hypothesis' own, or the least-squares fit over its inliers
    Th = np.eye(4)
    Th[:3, :3], Th[:3, 3] = want["R"][h], want["t"][h]
    r = np.linalg.norm(ps @ Th[:3, :3].T + Th[:3, 3] - pt, axis=1)
    inl = r <= p["max_distance"]
    dev = None
    if want["band"][h] == 0:
        assert got["inliers"] == inl.sum()
        # (a residual is a difference of coordinates: it carries a few ulps of the greatest coordinate, whatever its own size)
        assert abs(got["inlier_rmse"] - np.sqrt((r[inl] ** 2).mean())) <= 64 * ref.EPS * max(np.abs(ps).max(), np.abs(pt).max()), what
        if got["refit"]:
            dev = ref.pose_error(got["T"], ref.kabsch(ps[inl], pt[inl]))
            print("%s: best %d, inliers %d, scored %d, refit deviates from numpy's Kabsch by %.3e m, %.3e rad" % (what, h, got["inliers"], got["scored"], dev[0], dev[1]))
            assert dev[0] <= REFIT_TOL_M < 1e-6 and dev[1] <= REFIT_TOL_RAD < 1e-6, (what, dev)
        else:
            assert ref.pose_error(got["T"], Th) <= (1e-12, 1e-13), what
    return got, want, dev


def test_ransac_on_planted_pairs():
    src, tgt, pairs = planted()
    got, want, dev = check_ransac(src, tgt, pairs, what="planted")
    assert got["refit"] == 1 and dev is not None and 55 <= got["inliers"] <= 60
    dt, dr = ref.pose_error(got["T"], T_PLANTED)
    assert dt < 0.02 and dr < 0.002, (dt, dr)  # 60 inliers at 0.01 m noise
    assert set(want["triple"][got["best_hypothesis"]]) <= set(range(60))
    other, _, _ = check_ransac(src, tgt, pairs, what="another seed", seed=1)
    assert other["best_hypothesis"] != got["best_hypothesis"]
    assert ref.pose_error(other["T"], T_PLANTED) < (0.02, 0.002)


def test_ransac_on_a_far_origin_without_the_edge_test():
    o = (128000.0, -256000.0, 1280.0)
    src, tgt, pairs = planted(origin=o)
    got, _, dev = check_ransac(src, tgt, pairs, origin=o, what="far origin", edge_similarity=0.0, min_edge=2.0, iterations=8192)
    assert got["refit"] == 1 and ref.pose_error(got["T"], T_PLANTED)[1] < 0.002
    moved = (src[pairs[:60, 0]].astype(np.float64) + o) @ got["T"][:3, :3].T + got["T"][:3, 3] - (tgt[pairs[:60, 1]].astype(np.float64) + o)
    assert np.median(np.linalg.norm(moved, axis=1)) < 0.03


def test_ransac_small_cases_refusals_and_launches():
    src, tgt, pairs = planted()
    cs, ct = upload_relative(src, None, None, ZERO), upload_relative(tgt, None, None, ZERO)
    before = sga.ransac_launches()
    two = sga.ransac_correspondences(cs, ct, pairs[:2])
    assert two["inliers"] == 0 and two["scored"] == 0 and two["refit"] == 0 and np.array_equal(two["T"], np.eye(4))
    assert sga.ransac_correspondences(cs, ct, pairs[:0])["inliers"] == 0
    assert sga.ransac_launches() == before  # M < 3: nothing is launched
    three = sga.ransac_correspondences(cs, ct, pairs[:3], max_distance=0.1, iterations=64)
    assert sga.ransac_launches() - before == 4
    want = ref.ransac(src[pairs[:3, 0]].astype(np.float64), tgt[pairs[:3, 1]].astype(np.float64), 0.1, 64, 0, 0.9, 0.0)
    assert three["scored"] == want["valid"].sum() == 64 and three["inliers"] == 3 and three["best_hypothesis"] == 0  # every hypothesis is the one triangle
    # a triangle no rigid motion maps: every hypothesis is dropped
    none = sga.ransac_correspondences(cs, ct, pairs[100:103], iterations=64)
    assert none["scored"] == 0 and none["inliers"] == 0 and np.array_equal(none["T"], np.eye(4)) and none["refit"] == 0
    before = sga.ransac_launches()
    bad = pairs.copy()
    bad[150, 1] = 320
    with pytest.raises(sga.SgaError, match=r"pairs\[150\] names target point 320, outside a cloud of 320 points"):
        sga.ransac_correspondences(cs, ct, bad)
    bad = pairs.copy()
    bad[7, 0] = -1
    with pytest.raises(sga.SgaError, match=r"pairs\[7\] names source point -1"):
        sga.ransac_correspondences(cs, ct, bad)
    assert sga.ransac_launches() == before


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
T_TRUE = rigid([0.1, 0.2, 0.97], np.deg2rad(150.0), [12.0, -7.0, 1.5])
VOXEL, ABOVE = 0.5, (0.0, 0.0, 50.0)


@functools.lru_cache(maxsize=None)
def terrain_pair():
    target = synthetic.bumpy_terrain(60000, 1)
    world = synthetic.bumpy_terrain(60000, 2).astype(np.float64)
    Ti = np.linalg.inv(T_TRUE)
    return target, np.ascontiguousarray((world @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32))


@functools.lru_cache(maxsize=None)
def preprocessed():
    target, source = terrain_pair()
    tgt, ttree = sga.preprocess_points(target, VOXEL, 20)
    src, stree = sga.preprocess_points(source, VOXEL, 20)
    return tgt, ttree, src, stree


@functools.lru_cache(maxsize=None)
def restated_pairs():
    """the restatement's descriptors and mutual pairs of the two downsampled clouds (their records and normals are the inputs)"""
    tgt, _, src, _ = preprocessed()
    ft = ref.fpfh(records(tgt)[0], attributes(tgt)[0], 20, ABOVE)
    fs = ref.fpfh(records(src)[0], attributes(src)[0], 20, ABOVE)
    m = ref.match(fs["rows"].astype(F32), ft["rows"].astype(F32), True)
    keep = np.flatnonzero(m["match"] >= 0)
    return ft, fs, m, np.stack([keep, m["match"][keep]], axis=1)


def test_end_to_end_descriptors_and_pairs():
    tgt, ttree, src, stree = preprocessed()
    ft, fs, m, pairs = restated_pairs()
    assert not tgt.origin().any() and not src.origin().any()
    got_t, got_s = tgt.fpfh(ttree, 20, ABOVE), src.fpfh(stree, 20, ABOVE)
    check_fpfh(got_t.numpy(), ft, "target, %d points" % tgt.size())
    check_fpfh(got_s.numpy(), fs, "source, %d points" % src.size())
    assert m["band"].sum() <= 0.01 * len(m["band"])
    got = sga.match_features(got_s, got_t, mutual=True)
    ps, pt = src.xyz64()[pairs[:, 0]], tgt.xyz64()[pairs[:, 1]]
    true = np.linalg.norm(ps @ T_TRUE[:3, :3].T + T_TRUE[:3, 3] - pt, axis=1) < 1.5 * VOXEL
    print("%d / %d points, %d mutual pairs (device: %d), %d of them true" % (tgt.size(), src.size(), len(pairs), len(got), true.sum()))
    # the device's rows differ from the restatement's by an ulp here and there, so its pairs are compared as sets: all but a few agree
    same = len(set(map(tuple, got.tolist())) & set(map(tuple, pairs.tolist())))
    assert same >= 0.99 * max(len(got), len(pairs))
    # on the restatement's own rows the device finds the restatement's pairs
    exact = sga.match_features(sga.Features.from_array(fs["rows"].astype(F32)), sga.Features.from_array(ft["rows"].astype(F32)), mutual=True)
    good = ~m["band"][exact[:, 0]]
    assert np.array_equal(exact[good], pairs[~m["band"][pairs[:, 0]]])


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_end_to_end_pose(seed):
    tgt, ttree, src, stree = preprocessed()
    _, _, _, pairs = restated_pairs()
    setting = sga.make_setting("GICP")
    # the restatement first: its winner, refitted by numpy, lies in the basin
    ps, pt = src.xyz64()[pairs[:, 0]], tgt.xyz64()[pairs[:, 1]]
    want = ref.ransac(ps, pt, 1.5 * VOXEL, 20000, seed, 0.9, 2.0 * VOXEL)
    b = want["best"]
    inl = np.linalg.norm(ps @ want["R"][b].T + want["t"][b] - pt, axis=1) <= 1.5 * VOXEL
    dt, dr = ref.pose_error(ref.kabsch(ps[inl], pt[inl]), T_TRUE)
    print("seed %d restatement: %d pairs, best %d with %d inliers, coarse error %.3f m %.3f deg" % (seed, len(pairs), b, inl.sum(), dt, np.rad2deg(dr)))
    assert dt < 0.5 and dr < np.deg2rad(5.0)
    # the device, through global_align: the same chain on its own descriptors
    target, source = terrain_pair()
    coarse, refined = sga.global_align(target, source, VOXEL, k=20, iterations=20000, seed=seed, refine=True, setting=setting, viewpoint=ABOVE)
    dt, dr = ref.pose_error(coarse["T"], T_TRUE)
    print("seed %d device: %d pairs, best %d with %d inliers, coarse error %.3f m %.3f deg" % (seed, len(coarse["pairs"]), coarse["best_hypothesis"], coarse["inliers"], dt, np.rad2deg(dr)))
    assert dt < 0.5 and dr < np.deg2rad(5.0) and coarse["refit"] == 1
    # on the restatement's pairs the device's RANSAC is the restatement's
    on_ref = sga.ransac_correspondences(src, tgt, pairs, max_distance=1.5 * VOXEL, iterations=20000, seed=seed, min_edge=2.0 * VOXEL)
    assert on_ref["best_hypothesis"] == b or want["band"].max() > 0 or want["shaky"].any()
    assert abs(on_ref["inliers"] - want["score"][on_ref["best_hypothesis"]]) <= want["band"][on_ref["best_hypothesis"]]
    # refined: the pose align reaches from the truth, within twice the termination tolerances — which align from the identity does not reach
    from_truth = sga.Problem(ttree, src, T_TRUE).align(setting, T_TRUE)
    tol_t, tol_r = 2 * setting.translation_eps, 2 * setting.rotation_eps
    dt, dr = ref.pose_error(refined.T_target_source, from_truth.T_target_source)
    print("seed %d refined against align from the truth: %.2e m %.2e rad (allowed %.1e, %.1e)" % (seed, dt, dr, tol_t, tol_r))
    assert dt <= tol_t and dr <= tol_r
    from_identity = sga.Problem(ttree, src, np.eye(4)).align(setting, np.eye(4))
    dt, dr = ref.pose_error(from_identity.T_target_source, from_truth.T_target_source)
    assert not (dt <= tol_t and dr <= tol_r), "align from the identity reached the pose: the case proves nothing"


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_global_registration(tmp_path):
    """include/small_gicp_amd.hpp: Features, PointCloud::fpfh, match_features, Ransac and ransac_correspondences
    (tests/cpp/test_cpp_global_registration.cpp, compiled with g++ as test_cloud_outliers_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_global_registration"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_global_registration.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    target, source = terrain_pair()
    (tmp_path / "t.f32").write_bytes(target.tobytes())
    (tmp_path / "s.f32").write_bytes(source.tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "t.f32"), str(tmp_path / "s.f32"), "0.5", "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    out = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines()}
    tgt, _, src, _ = preprocessed()
    assert out["FEATURES"] == ["rows", str(src.size()), "dim", "33", "roundtrip", "1", "sums", "1"]
    assert out["REFUSE"] == ["k", "1", "pairs", "1"]
    # the same chain through Python gives the same numbers
    coarse, refined = sga.global_align(target, source, VOXEL, k=20, seed=1, viewpoint=ABOVE)
    g = out["GLOBAL"]
    assert [int(g[1]), int(g[3]), int(g[5]), int(g[7]), int(g[9])] == [len(coarse["pairs"]), coarse["inliers"], coarse["best_hypothesis"], coarse["scored"], coarse["refit"]]
    Tc = np.array([float(v) for v in out["COARSE"]]).reshape(4, 4).T
    assert np.array_equal(Tc, coarse["T"])
    assert ref.pose_error(Tc, T_TRUE) < (0.5, np.deg2rad(5.0))
    Tr = np.array([float(v) for v in out["REFINED"][2:]]).reshape(4, 4).T
    assert out["REFINED"][1] == "1" and ref.pose_error(Tr, refined.T_target_source) < (1e-9, 1e-9)

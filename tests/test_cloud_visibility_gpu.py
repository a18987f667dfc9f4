"""The free-space check on the device (csrc/cloud_visibility.hip: sga_cloud_visibility) against the fp64
restatement of tests/visibility_ref.py, which never goes through the library.

Inputs (test_cloud_overlap_gpu.py's): outliers_ref.planes_with_scatter for the map (target seed) and for the scene (source seed); the scan
is the scene seen from the pose (yaw 0.3, pitch -0.2, roll 0.1, t = (1.5, -2.0, 0.5)): fp32(T^-1 scene); both are uploaded relative to
a named origin (test_cloud_merge_gpu.upload_relative), so their records are known exactly.  Field of view +-60 degrees, ranges 0.5 / 12.0,
margin 0.1 m + 1 %.

The comparison rule is derived, not tuned.  With B_i = 64 eps64 (the magnitudes that enter s_i, rho_i and the window's ranges) a map
point is IN THE BAND when |rho - min_range|, |rho - max_range|, |(m - rho) - tol| or |(rho - M) - tol| lies within B_i, when its
projection is ambiguous (su or sv within 1e-9 of an integer: the device's atan2 / asin may differ from libm's by an ulp, its pose product
may contract into fused operations), or when its window holds a cell that an ambiguous scan return may land in.  Caps, asserted ON THE
REFERENCE before anything is compared: at most 2 band points per case and no ambiguous scan return (if a cap ever fails: another seed,
never a looser rule).  Reference figures of the six main cases, from the restatement on the CPU (no ambiguous projection and no band point
in any of them):
    map / scan seed            image, window       unobserved / consistent / occluded / seen through
    1 / 2 (n = 3000)           128 x 32, 1 x 1      113 / 2482 /  360 /  45
    1 / 2                       64 x 16, 0 x 0      164 /  491 / 2216 / 129
    1 / 2                      128 x 32, 2 x 1       90 / 2663 /  219 /  28
    3 / 4                      128 x 32, 1 x 1      105 / 2504 /  345 /  46
    5 / 6 (340 + 50: n = 730)  128 x 32, 1 x 1       58 /  515 /   95 /  62
    1 / 1                      128 x 32, 1 x 1       56 / 2603 /  341 /   0
Outside the band everything is exact: the states and the four counts, kept ascending, output records and attributes equal to input
[kept] bit for bit, the clearance within B_i and NaN exactly at state 0, two calls returning identical bytes.  A cell of the range image
lies within 4 eps64 rho of the restatement's (three rounded squares, two sums, one square root), +inf exactly where the restatement has
it.

Meaning: kitti_like_scan(0 and 3, n_rings=16, n_az=251) through synthetic.with_moving_sphere, image 128 x 16 over [-25, 3] degrees,
defaults otherwise, the ground-truth relative pose: of 3527 map points 17 lie on the sphere, 14 of them are seen through, and no static
point is."""
import functools
import os
import subprocess

import numpy as np
import pytest

import outliers_ref
import small_gicp_amd as sga
import visibility_ref as ref
from conftest import ROOT
from test_cloud_merge_gpu import FAR, QUARTER, attributes, pose, records, upload_relative
from test_cloud_outliers_gpu import attributes_for, synthetic_thinned

pytestmark = pytest.mark.gpu

F32 = np.float32
EPS64 = ref.EPS64
ZERO = np.zeros(3)
DEG = np.pi / 180.0
MAX_BAND = 2
POSE = pose(0.3, -0.2, 0.1, t=(1.5, -2.0, 0.5))
KEEPS = [None, "seen_through", "rest"]
BASE = dict(fov_up=60 * DEG, fov_down=-60 * DEG, min_range=0.5, max_range=12.0, margin=0.1, margin_ratio=0.01)
MAIN = [  # (map seed, scan seed, points per plane, scatter, width, height, window_h, window_v, the reference's counts)
    (1, 2, 1450, 100, 128, 32, 1, 1, (113, 2482, 360, 45)),
    (1, 2, 1450, 100, 64, 16, 0, 0, (164, 491, 2216, 129)),
    (1, 2, 1450, 100, 128, 32, 2, 1, (90, 2663, 219, 28)),
    (3, 4, 1450, 100, 128, 32, 1, 1, (105, 2504, 345, 46)),
    (5, 6, 340, 50, 128, 32, 1, 1, (58, 515, 95, 62)),
    (1, 1, 1450, 100, 128, 32, 1, 1, (56, 2603, 341, 0)),
]
NAMES = ("unobserved", "consistent", "occluded", "seen_through")


def image(width=128, height=32, window_h=1, window_v=1, **kw):
    p = dict(BASE, width=width, height=height, window_h=window_h, window_v=window_v)
    p.update(kw)
    return p


# ---- inputs and references, computed once -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene(seed, n_plane=1450, n_scatter=100):
    p = outliers_ref.planes_with_scatter(seed, n_plane, n_scatter)
    p.setflags(write=False)
    return p


def seen_from(points, T=POSE):
    """fp32(T^-1 points): the scene in the frame of a sensor at T"""
    Ti = np.linalg.inv(T)
    return np.ascontiguousarray((points.astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(F32))


@functools.lru_cache(maxsize=None)
def scan_of(seed, n_plane=1450, n_scatter=100):
    p = seen_from(scene(seed, n_plane, n_scatter))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def big_map():
    """9001 points: three scenes and one more point, so that the count kernel's stride loop and several compaction tiles are entered"""
    p = np.ascontiguousarray(np.concatenate([scene(1), scene(3), scene(7), scene(9)[:1]]))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def main_reference(mseed, sseed, n_plane, n_scatter, width, height, window_h, window_v, n=None):
    return ref.restate(scene(mseed, n_plane, n_scatter)[:n], scan_of(sseed, n_plane, n_scatter), T=POSE, **image(width, height, window_h, window_v))


# ---- the call and the comparison ------------------------------------------------------------------------------------------------------------
def run(cloud, scan, T, keep, kw, ctx=None):
    res = cloud.visibility(scan, T, keep=keep, return_state=True, return_clearance=True, return_image=True, return_kept=keep is not None, params=kw, ctx=ctx)
    k = 2 if keep else 1
    got = {"stats": res[0], "out": res[1] if keep else None, "state": res[k], "clearance": res[k + 1], "image": res[k + 2], "kept": res[k + 3] if keep else None}
    assert got["state"].dtype == np.uint8 and got["clearance"].dtype == np.float64 and got["image"].dtype == np.float64
    return got


def same_bytes(a, b):
    """two calls: every output identical"""
    assert a["stats"] == b["stats"]
    for name in ("state", "clearance", "image"):
        assert a[name].tobytes() == b[name].tobytes(), name
    if a["kept"] is not None:
        assert np.array_equal(a["kept"], b["kept"]) and a["out"].size() == b["out"].size()
        if a["out"].size():
            assert records(a["out"])[0].tobytes() == records(b["out"])[0].tobytes()


def check(got, want, rel, keep, nrm=None, cov6=None, origin=ZERO, what="", max_band=MAX_BAND):
    """the call's results `got` against the restatement `want` of the map's records `rel`"""
    n = len(rel)
    band = want["band"]
    assert len(band) <= max_band, (what, "the reference has %d points in the band" % len(band))
    assert want["ambiguous_scan"] == 0, (what, "the reference has %d ambiguous scan returns" % want["ambiguous_scan"])
    state, clearance, img, st = got["state"], got["clearance"], got["image"], got["stats"]
    sure = np.ones(n, bool)
    sure[band] = False
    # the range image: +inf exactly where the restatement has it, every cell within 4 eps64 rho
    assert img.shape == want["image"].shape and np.array_equal(np.isposinf(img), np.isposinf(want["image"])), what
    cells = np.isfinite(want["image"])
    cell_err = np.abs(img[cells] - want["image"][cells]) / want["image"][cells] if cells.any() else np.zeros(1)
    both = sure & (state != 0) & (want["state"] != 0)
    c_err = np.abs(clearance[both] - want["clearance"][both]) / want["B"][both] if both.any() else np.zeros(1)
    print("%s n %d keep %s: device %s, reference %s, band %d, %d cells, worst cell error %.3g eps64 rho (%d cells differ), worst clearance error %.3g of B"
          % (what, n, keep, [st[w] for w in NAMES], [want["counts"][w] for w in NAMES], len(band), int(cells.sum()), float(cell_err.max() / EPS64), int((cell_err != 0).sum()), float(c_err.max())))
    assert np.all(cell_err <= 4 * EPS64), what
    # states: the restatement's outside the band; the counts are those of the device's own states
    assert np.all(state <= 3) and np.array_equal(state[sure], want["state"][sure]), what
    assert st["points"] == n and [st[w] for w in NAMES] == [int((state == k).sum()) for k in range(4)], what
    if len(band) == 0:
        assert [st[w] for w in NAMES] == [want["counts"][w] for w in NAMES], what
    # clearance: NaN exactly at state 0, within B elsewhere
    assert np.array_equal(np.isnan(clearance), state == 0), what
    assert np.all(c_err <= 1.0), what
    if keep is None:
        assert got["out"] is None and got["kept"] is None
        return
    # the output cloud: the device's own states decide it, and they are the restatement's but for the band points
    out, kept = got["out"], got["kept"]
    assert kept.dtype == np.int64 and np.all(np.diff(kept) > 0), what  # ascending
    assert np.array_equal(kept, np.nonzero(((state == 3) if keep == "seen_through" else (state != 3)) & want["finite"])[0]), what
    assert np.all(np.isin(np.setxor1d(kept, ref.kept(want, keep)), band)), what
    assert out.size() == len(kept), what
    assert np.array_equal(out.origin(), np.asarray(origin, dtype=np.float64))  # the origin is kept
    if len(kept) == 0:
        assert out._has() == (False, False) and out._box() is None  # an empty cloud without attributes
        return
    assert out._has() == (nrm is not None, cov6 is not None)
    rec, _ = records(out)
    assert rec.tobytes() == np.ascontiguousarray(rel[kept]).tobytes(), what  # bit for bit
    nr, c6 = attributes(out)
    if nrm is not None:
        assert nr.tobytes() == np.ascontiguousarray(nrm[kept]).tobytes(), what
    if cov6 is not None:
        assert c6.tobytes() == np.ascontiguousarray(cov6[kept]).tobytes(), what
    lo, hi = out._box()  # the box of its own records, as the crop reports it
    assert np.array_equal(lo, rel[kept].min(axis=0)) and np.array_equal(hi, rel[kept].max(axis=0)), what


def compare(rel, scan_rel, T, kw, o_m=ZERO, o_s=ZERO, nrm=None, cov6=None, what="", max_band=MAX_BAND, keeps=KEEPS, want=None, twice=False):
    """upload, call with every keep, check against the restatement -> (the last call's results, the restatement)"""
    want = want if want is not None else ref.restate(rel, scan_rel, o_m=o_m, T=T, o_s=o_s, **kw)
    cloud = upload_relative(rel, nrm, cov6, o_m)
    scan = upload_relative(scan_rel, None, None, o_s)
    got = None
    for keep in keeps:
        got = run(cloud, scan, T, keep, kw)
        check(got, want, rel, keep, nrm=nrm, cov6=cov6, origin=o_m, what=what, max_band=max_band)
        if twice:
            same_bytes(got, run(cloud, scan, T, keep, kw))
    return got, want


# ---- 1. the main cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", MAIN, ids=lambda c: "m%d-s%d-n%d-%dx%d-w%dx%d" % (c[0], c[1], 2 * c[2] + c[3], c[4], c[5], c[6], c[7]))
def test_results_match_the_restatement(case):
    mseed, sseed, n_plane, n_scatter, width, height, wh, wv, counts = case
    want = main_reference(mseed, sseed, n_plane, n_scatter, width, height, wh, wv)
    assert tuple(want["counts"][w] for w in NAMES) == counts  # the figures in this file's docstring
    assert len(want["band"]) == 0 and want["ambiguous_scan"] == 0
    rel = scene(mseed, n_plane, n_scatter)
    nrm, cov6 = attributes_for(len(rel)) if case is MAIN[0] else (None, None)  # normals and covariances ride through keep
    kw = image(width, height, wh, wv)
    got, _ = compare(rel, scan_of(sseed, n_plane, n_scatter), POSE, kw, nrm=nrm, cov6=cov6, what=str(case[:8]), want=want, twice=True)
    # the optional outputs are optional, and the module function takes arrays
    cloud, scan = upload_relative(rel, None, None, ZERO), upload_relative(scan_of(sseed, n_plane, n_scatter), None, None, ZERO)
    st = cloud.visibility(scan, POSE, **kw)
    assert isinstance(st, dict) and st == got["stats"]
    assert sga.cloud_visibility(rel, scan_of(sseed, n_plane, n_scatter), POSE, **kw) == st
    st2, out = cloud.visibility(scan, POSE, keep="rest", **kw)
    assert st2 == st and out.size() == len(got["kept"])


# ---- 2. sizes at which the kernels can go wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_maps(n):
    want = main_reference(5, 6, 340, 50, 128, 32, 1, 1, n)
    compare(scene(5, 340, 50)[:n], scan_of(6, 340, 50), POSE, image(), what="map of %d" % n, want=want)


def test_a_map_of_9001_points():
    rel = big_map()
    assert len(rel) == 9001
    got, want = compare(rel, scan_of(2), POSE, image(), what="9001 points", twice=True)
    assert all(want["counts"][w] > 0 for w in NAMES)


def test_a_scan_of_one_point_and_an_empty_scan():
    rel = scene(5, 340, 50)
    got, want = compare(rel, scan_of(6, 340, 50)[:1], POSE, image(window_h=2, window_v=2), what="a scan of one point")
    assert np.isfinite(got["image"]).sum() == 1 and want["counts"]["unobserved"] < len(rel)
    got, want = compare(rel, np.zeros((0, 3), F32), POSE, image(), what="an empty scan")
    assert got["stats"]["unobserved"] == len(rel) and np.all(got["state"] == 0) and np.all(np.isnan(got["clearance"])) and np.all(np.isposinf(got["image"]))
    assert got["out"].size() == len(rel)  # nothing is seen through: the rest is everything


def test_an_empty_map_enqueues_nothing_unless_the_image_is_asked_for():
    scan_rel = scan_of(6, 340, 50)
    scan = upload_relative(scan_rel, None, None, ZERO)
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    kw = image()
    zero = {"points": 0, "unobserved": 0, "consistent": 0, "occluded": 0, "seen_through": 0}
    before = sga.cloud_visibility_launches()
    for keep in KEEPS:
        res = empty.visibility(scan, POSE, keep=keep, return_state=True, return_clearance=True, return_kept=keep is not None, params=kw)
        assert res[0] == zero and all(len(a) == 0 for a in res[(2 if keep else 1):])  # state, clearance and kept
        if keep:
            assert res[1].size() == 0 and res[1]._has() == (False, False)
    assert sga.cloud_visibility_launches() == before
    want_img, _, _ = ref.range_image(scan_rel, **kw)
    for keep in KEEPS:
        res = empty.visibility(scan, POSE, keep=keep, return_image=True, params=kw)
        assert res[0] == zero and np.array_equal(np.isposinf(res[-1]), np.isposinf(want_img))
        cells = np.isfinite(want_img)
        assert np.all(np.abs(res[-1][cells] - want_img[cells]) <= 4 * EPS64 * want_img[cells])
        if keep:
            assert res[1].size() == 0
    assert sga.cloud_visibility_launches() == before + 3 * 3  # the fill, the image, the export


# ---- 3. exact arithmetic, the seam, non-finite records --------------------------------------------------------------------------------------
def integer_points(seed, n=400):
    p = np.unique(np.random.default_rng(seed).integers(-9, 10, (n, 3)), axis=0).astype(np.float64)
    return p[np.abs(p).sum(axis=1) > 0]


@pytest.mark.parametrize("k", range(len(QUARTER)))
def test_quarter_turn_poses_with_integer_coordinates_have_no_band(k):
    """axis permutations and integer translations: s is exact, so nothing but the projection's own rounding is left.  Integer directions
    often sit on a cell's edge (y = 0, x = y, z = 0 ...): the points whose projection the restatement flags as ambiguous are left out of
    the INPUT, for the scan and for the map; then the band is empty."""
    T, Ti = QUARTER[k], np.linalg.inv(QUARTER[k])
    kw = image(max_range=20.0)
    scan_rel = integer_points(11 + k) @ Ti[:3, :3].T + Ti[:3, 3]
    scan_rel = scan_rel[~ref.project(scan_rel, kw["width"], kw["height"], kw["fov_up"], kw["fov_down"])["ambiguous"]].astype(F32)
    rel = integer_points(21 + k)
    s, _ = ref.sensor_points(rel.astype(F32), ZERO, T)
    rel = rel[~ref.project(s, kw["width"], kw["height"], kw["fov_up"], kw["fov_down"])["ambiguous"]].astype(F32)
    assert len(rel) > 200 and len(scan_rel) > 200
    got, want = compare(rel, scan_rel, T, kw, what="quarter turn %d" % k, max_band=0, twice=True)
    assert np.array_equal(want["s"], np.rint(want["s"])) and min(want["counts"][w] for w in NAMES) > 0


def test_a_pair_across_the_seam():
    kw = dict(ref.DEFAULTS, width=8, height=4, fov_up=30 * DEG, fov_down=-31 * DEG, window_v=0)
    scan_rel = np.array([[-10.0, -0.1, 0.0]], F32)  # az just above -pi: u = 0
    rel = np.array([[-5.0, 0.1, 0.0], [-15.0, 0.1, 0.0], [-3.0, 5.0, 0.0]], F32)  # az just below +pi: u = 7; the third further round: u = 6
    got, want = compare(rel, scan_rel, None, dict(kw, window_h=1), what="the seam, window 1", max_band=0)
    assert want["u"].tolist() == [7, 7, 6] and got["state"].tolist() == [ref.SEEN_THROUGH, ref.OCCLUDED, ref.UNOBSERVED]
    got, want = compare(rel, scan_rel, None, dict(kw, window_h=0), what="the seam, window 0", max_band=0)
    assert got["state"].tolist() == [0, 0, 0]
    got, want = compare(rel, scan_rel, None, dict(kw, window_h=16), what="the seam, a window wider than the image", max_band=0)
    assert got["state"].tolist() == [ref.SEEN_THROUGH, ref.OCCLUDED, ref.SEEN_THROUGH]
    # azimuth +pi exactly is cell 0, as -pi is
    got, want = compare(np.array([[-5.0, 0.0, 0.0], [-5.0, -0.0, 0.0]], F32), np.array([[-10.0, 0.0, 0.0]], F32), None, dict(kw, window_h=0), what="azimuth pi", max_band=0)
    assert got["state"].tolist() == [ref.SEEN_THROUGH, ref.SEEN_THROUGH] and np.isfinite(got["image"][:, 0]).sum() == 1


def test_non_finite_map_and_scan_records():
    rel = scene(5, 340, 50).copy()
    rel[17, 1] = np.nan
    rel[401] = [np.inf, 0.0, 0.0]
    rel[64, 2] = -np.inf
    scan_rel = scan_of(6, 340, 50).copy()
    scan_rel[3, 0] = np.nan
    scan_rel[100] = [np.inf, -np.inf, 0.0]
    scan_rel[640, 2] = np.inf
    got, want = compare(rel, scan_rel, POSE, image(), what="non-finite records", twice=True)
    assert np.all(got["state"][[17, 401, 64]] == 0) and got["stats"]["points"] == len(rel)
    for keep in ("seen_through", "rest"):
        _, _, kept = upload_relative(rel, None, None, ZERO).visibility(upload_relative(scan_rel, None, None, ZERO), POSE, keep=keep, return_kept=True, params=image())
        assert not np.isin([17, 401, 64], kept).any()  # counted in points and in unobserved, in no output cloud
    assert got["out"].size() == len(rel) - 3 - got["stats"]["seen_through"]


# ---- 4. frames ------------------------------------------------------------------------------------------------------------------------------
def test_far_device_frames_with_the_pose_carrying_the_difference():
    """the map's records are relative to FAR and the pose carries FAR; the scan's records are relative to an origin of its own, kilometres
    out, that the kernel adds back in double.  (The sensor frame is where the scan's records plus its origin are, so a scan cannot lie
    4 000 km from its own sensor: at (3000, -7000, 500) its records sit on fp32's grid of a quarter to half a millimetre, and the
    restatement sees the same records.)"""
    o_m, o_s = FAR, np.array([3000.0, -7000.0, 500.0])
    rel = scene(1)
    scan_rel = (scan_of(2).astype(np.float64) - o_s).astype(F32)
    T = POSE.copy()
    T[:3, 3] = POSE[:3, 3] + o_m
    got, want = compare(rel, scan_rel, T, image(), o_m=o_m, o_s=o_s, what="far frames", twice=True)
    plain = main_reference(1, 2, 1450, 100, 128, 32, 1, 1)
    assert np.abs(want["s"] - plain["s"]).max() < 1e-8 and np.abs(want["image"][np.isfinite(plain["image"])] - plain["image"][np.isfinite(plain["image"])]).max() < 0.5  # the same geometry


def test_no_pose_with_both_in_one_frame():
    rel, scan_rel = scene(1), scene(2)
    got, want = compare(rel, scan_rel, None, image(), what="T = None")
    assert np.array_equal(want["s"], rel.astype(np.float64)) and min(want["counts"][w] for w in NAMES) > 0


# ---- 5. refusals that need live handles, ordering across contexts ---------------------------------------------------------------------------
def test_a_cloud_on_another_device_is_refused():
    if sga.load().sga_device_count() < 2:
        pytest.skip("ONE DEVICE ONLY: the refusal of a cloud that lives on another device was NOT exercised")
    other = sga.Context(1)
    here, there = upload_relative(scene(5, 340, 50), None, None, ZERO), upload_relative(scan_of(6, 340, 50), None, None, ZERO, other)
    before = sga.cloud_visibility_launches()
    with pytest.raises(sga.SgaError, match="scan lives on another device"):
        here.visibility(there, POSE)
    with pytest.raises(sga.SgaError, match="map lives on another device"):
        there.visibility(here, POSE, ctx=sga.default_context())
    assert sga.cloud_visibility_launches() == before


def test_clouds_made_on_another_context_that_returned_early():
    rel, scan_rel, kw = scene(1), scan_of(2), image()
    plain = run(upload_relative(rel, None, None, ZERO), upload_relative(scan_rel, None, None, ZERO), POSE, "rest", kw)
    ctx, other = sga.Context(0), sga.Context(0)
    ctx.set_stream_ordered(True)
    other.set_stream_ordered(True)
    try:
        cloud = upload_relative(rel, None, None, ZERO, other)  # returns with its kernels in flight on the other context's stream
        scan = upload_relative(scan_rel, None, None, ZERO, other)
        got = run(cloud, scan, POSE, "rest", kw, ctx=ctx)
        same_bytes(got, plain)
        check(got, main_reference(1, 2, 1450, 100, 128, 32, 1, 1), rel, "rest", what="clouds of another context")
    finally:
        ctx.set_stream_ordered(False)
        other.set_stream_ordered(False)


# ---- 6. the launch counter ------------------------------------------------------------------------------------------------------------------
def test_the_launch_counter_rises_by_the_documented_amounts():
    outliers, crops, overlaps = sga.cloud_outliers_launches(), sga.cloud_crop_launches(), sga.cloud_overlap_launches()
    scan, none = upload_relative(scan_of(2), None, None, ZERO), upload_relative(np.zeros((0, 3), F32), None, None, ZERO)
    kw = image()
    for rel in (scene(1), big_map()):  # whatever the size
        cloud = upload_relative(rel, None, None, ZERO)
        for s, commands in ((scan, 4), (none, 3)):  # the fill, the image (none for an empty scan), the states, the counts
            before = sga.cloud_visibility_launches()
            cloud.visibility(s, POSE, **kw)
            assert sga.cloud_visibility_launches() - before == commands
            before = sga.cloud_visibility_launches()
            cloud.visibility(s, POSE, return_state=True, return_clearance=True, return_image=True, **kw)
            assert sga.cloud_visibility_launches() - before == commands
            before = sga.cloud_visibility_launches()
            cloud.visibility(s, POSE, keep="rest", return_kept=True, **kw)
            assert sga.cloud_visibility_launches() - before == commands + 2  # ... the compaction's table copy, the compaction
    assert (sga.cloud_outliers_launches(), sga.cloud_crop_launches(), sga.cloud_overlap_launches()) == (outliers, crops, overlaps)


# ---- 7. meaning -----------------------------------------------------------------------------------------------------------------------------
def test_a_moving_sphere_is_seen_through_and_no_static_point_is():
    from small_gicp_amd import synthetic

    frames = []
    for f in (0, 3):
        pts, Tws = synthetic.kitti_like_scan(f, n_rings=16, n_az=251)
        pts, changed = synthetic.with_moving_sphere(pts, Tws, synthetic._sensor_pose(0)[:3, 3] + np.array([12.0, -6.0 + 1.5 * f, -0.8]))
        frames.append((pts, changed, Tws))
    assert np.array_equal(synthetic.mover_centre(3), synthetic._sensor_pose(0)[:3, 3] + np.array([12.0, -1.5, -0.8]))
    (rel, on_sphere, T0), (scan_rel, _, T3) = frames
    T = np.linalg.inv(T0) @ T3  # the ground-truth relative pose: the later scan's sensor frame in the earlier one's
    kw = dict(ref.DEFAULTS, width=128, height=16)
    want = ref.restate(rel, scan_rel, T=T, **kw)
    seen = want["state"] == ref.SEEN_THROUGH
    assert (len(rel), int(on_sphere.sum()), int((seen & on_sphere).sum()), int((seen & ~on_sphere).sum())) == (3527, 17, 14, 0)
    got, _ = compare(rel, scan_rel, T, kw, what="the moving sphere", want=want)
    sure = np.ones(len(rel), bool)
    sure[want["band"]] = False
    dev = got["state"] == ref.SEEN_THROUGH
    assert int((dev & on_sphere & sure).sum()) == int((seen & on_sphere & sure).sum()) and not (dev & ~on_sphere & sure).any()
    # the cleaned map: everything but the seen-through points, by the library's defaults but for the image's size
    st, rest = upload_relative(rel, None, None, ZERO).visibility(upload_relative(scan_rel, None, None, ZERO), T, width=128, height=16, keep="rest")
    assert rest.size() == len(rel) - st["seen_through"] and st == got["stats"]


# ---- 8. the driver --------------------------------------------------------------------------------------------------------------------------
def test_submap_odometry_removes_the_trail_of_a_mover():
    from small_gicp_amd import odometry

    frames, window = 8, 5
    without = odometry.run_synthetic_submap(frames, window=window, mover=True)
    with_check = odometry.run_synthetic_submap(frames, window=window, mover=True, remove_seen_through=True)
    removed, entered = sum(with_check["removed_points"]), with_check["entered_points"]
    print("mover, %d frames, window %d: ghost points %d without the check, %d with it; removed %d of the %d points that entered the window (%.3f %%); ate_trans_m_max %.4f without, %.4f with"
          % (frames, window, without["ghost_points"], with_check["ghost_points"], removed, entered, 100.0 * removed / entered, without["ate_trans_m_max"], with_check["ate_trans_m_max"]))
    assert without["removed_points"] == [] and len(with_check["removed_points"]) == frames - 1
    assert without["ghost_points"] > 0 and 2 * with_check["ghost_points"] <= without["ghost_points"]
    assert removed < 0.01 * entered
    for res in (without, with_check):  # (tests/test_cloud_merge_gpu.py's check of the submap driver: each relative motion is the simulated 1 m)
        for f in range(1, frames):
            rel = np.linalg.inv(res["estimated"][f - 1]) @ res["estimated"][f]
            assert abs(np.linalg.norm(rel[:3, 3]) - 1.0) < 0.02
    # off, and without a mover: the poses are what they were
    plain = odometry.run_synthetic_submap(4, window=3)
    again = odometry.run_synthetic_submap(4, window=3, remove_seen_through=False, mover=False)
    assert plain["ghost_points"] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(plain["estimated"], again["estimated"]))


# ---- 9. the C++ header ----------------------------------------------------------------------------------------------------------------------
def test_cpp_visibility(tmp_path):
    """include/small_gicp_amd.hpp: Visibility and PointCloud::visibility against the C-ABI call (tests/cpp/test_cpp_cloud_visibility.cpp,
    compiled with g++ as test_cloud_overlap_gpu.py compiles its program)."""
    exe = tmp_path / "test_cpp_cloud_visibility"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_visibility.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    (tmp_path / "p.f32").write_bytes(synthetic_thinned().tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    out = [r for r in rows if r[0] == "VISIBILITY"]
    assert [r[2] for r in out] == ["0", "1", "2"]
    for r in out:  # VISIBILITY keep k points n seen m stats s kept k arrays a cloud c
        assert 0 < int(r[6]) < int(r[4]) and r[8] == "1" and r[10] == "1" and r[12] == "1" and r[14] == "1", r
    assert [r for r in rows if r[0] == "REFUSE"] == [["REFUSE", "equal", "1"]]

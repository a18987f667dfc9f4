#!/usr/bin/env python3
"""One sha256 per case over what the cloud operations leave behind, from seeded synthetic inputs: two builds of the library hold the same
bits exactly when they print the same lines (run it once per build: SGA_LIB_PATH names the library).

A digest covers, per cloud: its size, its device-frame origin, the box it carries (sga_debug_cloud_box), its attribute flags and
everything sga_cloud_download returns (points, normals, covariances); per case also the indices kept (crop, outlier removal) and the
outlier statistics (per-point statistic, mean, stddev, threshold, kept).

Cases, at about 256 and about 2048 points and at 133121 (66 tiles of the crop: a second look-back window):
  upload_*    pageable and pinned host arrays, near and far from the origin
  slice / select
  merge_*     with the origin chosen by the library and with a given one
  deskew_*    lone and in one batch (an empty member among them)
  crop_*      lone, box modes 1 and 2, a batch with an empty member and one that loses everything
  outliers_*  statistical and radius mode on the wave-per-query and the lane-per-query route
  voxelgrid_* lone and in one batch

  python scripts/cloud_ops_digest.py [--out file]
"""
import argparse
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

F32 = np.float32
FAR = np.array([4.5e5, -7.2e5, 300.0])
SIZES = (255, 257, 2047, 2049, 133121)
WAVE_DEFAULT = 81920  # sga_set_knn_wave_max's default (tests/test_cloud_outliers_gpu.py)


def arrays(n, seed, far=False):
    """points (float32, or float64 around FAR), unit normals, symmetric positive definite covariances (n, 6)"""
    rng = np.random.default_rng(seed)
    p = rng.uniform((-40, -40, -3), (40, 40, 3), (n, 3))
    v = rng.normal(size=(n, 3))
    nr = (v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-9)).astype(F32)
    a = rng.normal(size=(n, 3, 3)) * 0.05
    c6 = api.sym6_from_mats(a @ a.transpose(0, 2, 1) + 1e-4 * np.eye(3)).astype(F32)
    return (p + FAR if far else p.astype(F32)), nr, c6


def cloud(n, seed, far=False, normals=True, covs=True):
    p, nr, c6 = arrays(n, seed, far)
    return sga.PointCloud(p, normals=nr if normals else None, covs=c6 if covs else None)


def digest(h, c):
    n = c.size()
    hn, hc = c._has()
    box = c._box()
    h.update(np.int64([n, hn, hc, box is not None]).tobytes() + c.origin().tobytes())
    if box is not None:
        h.update(box[0].tobytes() + box[1].tobytes())
    xyz, nr, c6 = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros((n, 6), F32)
    api.check(sga.load().sga_cloud_download(c.ctx.h, c.h, api._fp(xyz), api._fp(nr) if hn else None, api._fp(c6) if hc else None))
    h.update(xyz.tobytes() + nr.tobytes() + c6.tobytes())


def case(out, name, clouds, extra=()):
    h = hashlib.sha256()
    for c in clouds:
        digest(h, c)
    for a in extra:
        h.update(np.ascontiguousarray(a).tobytes())
    out.append("%-34s %s  clouds %d points %d" % (name, h.hexdigest(), len(clouds), sum(c.size() for c in clouds)))


def upload_cases(out):
    for n in SIZES:
        made = []
        for far in (False, True):
            p, nr, c6 = arrays(n, 10 + n % 97, far)
            made += [sga.PointCloud(p, normals=nr, covs=c6), sga.PointCloud(p)]
            if not far:  # pinned float32 arrays are read in place
                made += [sga.PointCloud(api.pinned_copy(p), normals=api.pinned_copy(nr), covs=api.pinned_copy(c6)), sga.PointCloud(api.pinned_copy(p))]
        case(out, "upload_%d" % n, made)


def gather_cases(out):
    for n in SIZES:
        c, bare = cloud(n, 20 + n % 97, far=True), cloud(n, 21 + n % 97, normals=False, covs=False)
        idx = np.random.default_rng(n).integers(0, n, n // 2 + 3)
        made = []
        for m in (c, bare):
            made += [m.slice(0, 0), m.slice(3, 1), m.slice(3, n - 3), m.slice(0, n), m.slice(n - 1, 1), m.selected(idx), m.selected([]), m.selected(np.arange(n)[::-1])]
        case(out, "slice_select_%d" % n, made)


def pose(rx, ry, rz, t):
    T = np.eye(4)
    T[:3, :3] = sga.se3_exp([rx, ry, rz, 0, 0, 0])[:3, :3]
    T[:3, 3] = t
    return T


def merge_cases(out):
    members = [cloud(255, 30), cloud(2049, 31, far=True), cloud(4, 32).slice(0, 0), cloud(257, 33, covs=False), cloud(133121, 34)]
    Ts = [pose(0.1 * k, -0.05 * k, 0.3 + 0.2 * k, [3.0 * k, -2.0 * k, 0.5]) for k in range(len(members))]
    Ts[1][:3, 3] -= Ts[1][:3, :3] @ FAR  # the far member lands near the others
    case(out, "merge_origin_chosen", [sga.merge_clouds(members, Ts), sga.merge_clouds(members[:3], Ts[:3]), sga.merge_clouds(members), members[3].transformed(Ts[3])])
    case(out, "merge_origin_given", [sga.merge_clouds(members, Ts, origin=(128.0, -256.0, 0.0)), sga.merge_clouds(members[:1], Ts[:1], origin=(0.0, 0.0, 0.0)), members[4].transformed(Ts[4], origin=(1.0, 2.0, 3.0))])


def deskew_cases(out):
    members = [cloud(255, 40), cloud(2049, 41, far=True), cloud(4, 42).slice(0, 0), cloud(257, 43, normals=False), cloud(133121, 44, covs=False)]
    times = [np.random.default_rng(45 + k).uniform(0.0, 1.0, m.size()).astype(F32) for k, m in enumerate(members)]
    twists = [[0.02 * (k + 1), -0.01, 0.05, 1.5, -0.2 * k, 0.1] for k in range(len(members))]
    refs = [1.0, 0.5, 0.0, 0.25, 1.0]
    case(out, "deskew_lone", [m.deskewed(t, xi, r) for m, t, xi, r in zip(members, times, twists, refs) if m.size()])
    case(out, "deskew_batch", sga.deskew_clouds(members, times, twists, refs))


def crop_cases(out):
    members = [cloud(255, 50), cloud(2049, 51, far=True), cloud(4, 52).slice(0, 0), cloud(257, 53, normals=False), cloud(133121, 54), cloud(2047, 55, covs=False)]
    members[0] = sga.PointCloud(np.where(np.arange(255)[:, None] % 50 == 7, np.nan, members[0].xyz()).astype(F32))  # non-finite records are dropped
    box = ((-20.0, -30.0, -2.0), (25.0, 10.0, 2.5))
    crops = [dict(), dict(min_range=10.0, max_range=35.0, center=FAR), dict(min_range=1.0), dict(box=box, box_mode="outside"), dict(min_range=5.0, max_range=38.0, center=(3.0, -4.0, 1.0), box=box), dict(min_range=500.0)]
    lone = [m.cropped(return_kept=True, **cr) for m, cr in zip(members, crops)]
    case(out, "crop_lone", [o for o, _ in lone], [k for _, k in lone])
    case(out, "crop_box_inside", [members[4].cropped(box=box)])
    case(out, "crop_box_outside", [members[4].cropped(box=box, box_mode="outside"), members[1].cropped(box=(tuple(FAR - 10.0), tuple(FAR + 10.0)), box_mode="outside")])
    outs, kepts = sga.crop_clouds(members, crops, return_kept=True)
    case(out, "crop_batch", outs, kepts)


def outlier_cases(out):
    clouds = [cloud(257, 60), cloud(2049, 61, far=True, normals=False), cloud(133121, 62, covs=False)]
    for wave in (True, False):
        sga.load().sga_set_knn_wave_max(C.c_longlong(1 << 40 if wave else 0))
        made, extra = [], []
        for c in clouds:
            for kw in (dict(k=10), dict(k=7, std_mul=0.5), dict(k=5, radius=1.5)):
                o, kept, st = c.without_outliers(return_kept=True, return_stats=True, **kw)
                made.append(o)
                extra += [kept, st["stat"], np.float64([st["mean"], st["stddev"], st["threshold"], st["kept"]])]
        case(out, "outliers_%s_route" % ("wave" if wave else "lane"), made, extra)
    sga.load().sga_set_knn_wave_max(C.c_longlong(WAVE_DEFAULT))


def voxelgrid_cases(out):
    clouds = [cloud(255, 70), cloud(2049, 71, far=True), cloud(133121, 72), cloud(4, 73).slice(0, 0), cloud(2047, 74).slice(5, 2000)]
    case(out, "voxelgrid_lone", [sga.voxelgrid_sampling(c, 0.5) for c in clouds] + [sga.voxelgrid_sampling(clouds[2], 2.0)])
    case(out, "voxelgrid_batch", sga.voxelgrid_sampling_batch(clouds, 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for cases in (upload_cases, gather_cases, merge_cases, deskew_cases, crop_cases, outlier_cases, voxelgrid_cases):
        cases(out)
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Wall time of removing outliers on the device (PointCloud.without_outliers: sga_cloud_remove_outliers) beside the host route and beside
the call that runs the same search, in the same process and build (the protocol of scripts/cloud_crop_rate.py).

Two clouds, both on the device already: a downsampled C5 scan (synthetic.kitti_like_scan(3) through the 0.25 m voxel grid, about 11k
points: the wave-per-query route) and a raw sweep (synthetic.kitti_like_sweep(3), about 121k points: the lane-per-query route), each
with 1 % isolated returns scattered in (synthetic.with_isolated_returns).  Per cloud, k = 10, std_mul = 1:
      filter, tree   cloud.without_outliers(10, tree=tree)          the caller's tree: statistic, threshold, table copy, compaction, one wait
      filter, temp   cloud.without_outliers(10)                     a temporary tree: the lone kd build in front
      radius, tree   cloud.without_outliers(5, radius=0.5, tree=…)  radius mode: no threshold step
      covariances    estimate_covariances(twin, twin's tree, 10)    the yardstick: the same search with the same k on the same points and
                                                                    an eigen-decomposition per point behind it (a twin cloud, so that the
                                                                    filtered cloud carries no covariances the compaction would gather)
      kd build       KdTree(cloud)                                  what "temp" adds, for scale
      host route     sga_cloud_download, scipy's cKDTree k-NN (numpy brute force where scipy is missing and the cloud is small; else left
                     out), the definitions in float64, sga_cloud_create_f32
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/cloud_outliers_rate.py [--reps 9] [--out profiles/cloud_outliers_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

K, STD_MUL = 10, 1.0

try:
    from scipy.spatial import cKDTree
except Exception:  # noqa: BLE001
    cKDTree = None


def host_stat(xyz, k):
    """mean distance to the k nearest other records, float64"""
    r = xyz.astype(np.float64)
    if cKDTree is not None:
        d, _ = cKDTree(r).query(r, k=k + 1)
        return d[:, 1:].sum(axis=1) / k
    out = np.empty(len(r))
    step = max(1, (1 << 22) // len(r))
    for a in range(0, len(r), step):
        diff = r[a:a + step, None, :] - r[None, :, :]
        d = np.sqrt((diff * diff).sum(axis=2))
        out[a:a + step] = np.sort(np.partition(d, k, axis=1)[:, : k + 1], axis=1).sum(axis=1) / k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sga.Context(0)
    lib = sga.load()
    scan = sga.synthetic.with_isolated_returns(sga.synthetic.kitti_like_scan(3)[0], 0.01)[0]
    sweep = sga.synthetic.with_isolated_returns(sga.synthetic.kitti_like_sweep(3)[0], 0.01)[0]
    down = api.voxelgrid_sampling(sga.PointCloud(scan, ctx=ctx), 0.25).xyz()
    settings, notes = [], []
    for label, pts in (("down", down), ("raw", sweep)):
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        n = len(pts)
        cloud, twin = sga.PointCloud(pts, ctx=ctx), sga.PointCloud(pts, ctx=ctx)
        tree, twin_tree = sga.KdTree(cloud), sga.KdTree(twin)

        def host_route(cloud=cloud, n=n):
            xyz = np.empty((n, 3), np.float32)
            api.check(lib.sga_cloud_download(ctx.h, cloud.h, api._fp(xyz), None, None))
            d = host_stat(xyz, K)
            keep = d <= d.mean() + STD_MUL * d.std(ddof=1)
            return sga.PointCloud(np.ascontiguousarray(xyz[keep]), ctx=ctx)

        mine = [
            (label + " filter, tree", lambda cloud=cloud, tree=tree: cloud.without_outliers(K, STD_MUL, tree=tree)),
            (label + " filter, temp", lambda cloud=cloud: cloud.without_outliers(K, STD_MUL)),
            (label + " radius, tree", lambda cloud=cloud, tree=tree: cloud.without_outliers(5, radius=0.5, tree=tree)),
            (label + " covariances", lambda twin=twin, twin_tree=twin_tree: api.estimate_covariances(twin, twin_tree, K)),
            (label + " kd build", lambda cloud=cloud: sga.KdTree(cloud)),
        ]
        have_host = cKDTree is not None or n <= 20000
        if have_host:
            mine.append((label + " host route", host_route))
        settings += mine
        kept = cloud.without_outliers(K, STD_MUL, tree=tree).size()
        host_kept = host_route().size() if have_host else -1
        notes.append("%s = %d points, %d kept by the device, %s by the host route, wave-per-query route: %s" % (label, n, kept, host_kept if have_host else "n/a", "yes" if n <= 81920 else "no"))

    def region(fn):
        t0 = time.perf_counter()
        keep = fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        del keep
        return dt

    for _, fn in settings:
        region(fn)
        region(fn)
    t = {name: [] for name, _ in settings}
    for _ in range(a.reps):
        for name, fn in settings:
            t[name].append(region(fn))
    lines = ["# scripts/cloud_outliers_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# PointCloud.without_outliers(k = %d, std_mul = %g) with the caller's tree / a temporary tree, radius mode (k = 5, 0.5 m), estimate_covariances(k = %d) on a twin cloud and its tree (the same search, plus an"
             % (K, STD_MUL, K),
             "#     eigen-decomposition per point), the lone kd build, and the host route (download, %s k-NN, float64 definitions, upload)" % ("scipy cKDTree" if cKDTree is not None else "numpy brute-force")]
    lines += ["# " + s for s in notes]
    med, lo, hi = {}, {}, {}
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        med[name], lo[name], hi[name] = float(np.median(v)), float(v.min()), float(v.max())
        lines.append("%-18s %10.1f (%8.1f .. %8.1f)" % (name, med[name], lo[name], hi[name]))
    for label in ("down", "raw"):
        f, c = label + " filter, tree", label + " covariances"
        lines.append("%s: the filter with the caller's tree against estimate_covariances: median %.2f x; slowest filter region below the fastest covariance region: %s"
                     % (label, med[f] / med[c], "yes" if hi[f] < lo[c] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

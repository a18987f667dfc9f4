#!/usr/bin/env python3
"""Wall time of comparing a posed cloud with a target on the device (PointCloud.overlap: sga_cloud_overlap) beside the host route and
beside the closest device path the library had before, in the same process and build (the protocol of scripts/cloud_outliers_rate.py).

The target is a five-scan submap: synthetic.kitti_like_scan(0 .. 4), each through the 0.25 m voxel grid, merged at the generator's poses
(api.merge_clouds), with its KdTree and, for the map settings, the one-shot GaussianVoxelMap over it (leaf 0.5 m, covariances with k = 10,
search offsets 1).  Two clouds, both on the device already and posed by the generator's pose of scan 5: that scan through the voxel grid
(about 12.6k points) and the raw scan (about 121k points).  max_distance = 0.25 m.  Per cloud and target:
      stats          cloud.overlap(target, T, 0.25)                            the distances and the sums: two launches, one wait
      unmatched      cloud.overlap(target, T, 0.25, keep="unmatched")          ... and the compaction: table copy, launch, its wait
      knn path       cloud.transformed(T).to_torch(), target.batch_knn_search_torch(q, 1, 0.25^2), the distances .cpu()
                                                                               the closest existing device path: sga_cloud_transform,
                                                                               sga_cloud_export_device, sga_index_knn_device with k = 1,
                                                                               download of the distances (the mask would be the host's)
      host route     sga_cloud_download of the cloud and of the target's points (the submap, or the map's means), the pose in float64,
                     scipy's cKDTree build and query (k = 1), the mask, sga_cloud_create_f32 of the unmatched points
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/cloud_overlap_rate.py [--reps 9] [--out profiles/cloud_overlap_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

RES, LEAF, MAX_DISTANCE, WINDOW = 0.25, 0.5, 0.25, 5

try:
    from scipy.spatial import cKDTree
except Exception:  # noqa: BLE001
    cKDTree = None
try:
    import torch
except Exception:  # noqa: BLE001
    torch = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sga.Context(0)
    lib = sga.load()
    scans = [sga.synthetic.kitti_like_scan(f) for f in range(WINDOW + 1)]
    T0i = np.linalg.inv(scans[0][1])
    downs = [api.voxelgrid_sampling(sga.PointCloud(p, ctx=ctx), RES) for p, _ in scans]
    submap = api.merge_clouds(downs[:WINDOW], [T0i @ T for _, T in scans[:WINDOW]], ctx=ctx)
    tree = sga.KdTree(submap)
    api.estimate_covariances(submap, tree, 10)
    gmap = sga.GaussianVoxelMap.from_cloud(submap, LEAF)
    T = T0i @ scans[WINDOW][1]
    targets = [("kd", tree, submap.size(), lambda: submap.xyz64()), ("map", gmap, gmap.size(), lambda: gmap.download()[1].astype(np.float64))]
    clouds = [("down", downs[WINDOW]), ("raw", sga.PointCloud(np.ascontiguousarray(scans[WINDOW][0][:, :3], dtype=np.float32), ctx=ctx))]
    settings, notes = [], []
    for label, cloud in clouds:
        n = cloud.size()
        for tname, target, tn, target_points in targets:

            def host_route(cloud=cloud, n=n, target_points=target_points):
                xyz = np.empty((n, 3), np.float32)
                api.check(lib.sga_cloud_download(ctx.h, cloud.h, api._fp(xyz), None, None))
                q = xyz.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
                d, _ = cKDTree(target_points()).query(q, k=1)
                return sga.PointCloud(np.ascontiguousarray(xyz[~(d <= MAX_DISTANCE)]), ctx=ctx), int((d <= MAX_DISTANCE).sum())

            def knn_path(cloud=cloud, target=target):
                q = cloud.transformed(T).to_torch()
                _, d2 = target.batch_knn_search_torch(q, 1, MAX_DISTANCE * MAX_DISTANCE)
                return d2.cpu()

            name = "%s %s" % (label, tname)
            mine = [(name + " stats", lambda cloud=cloud, target=target: cloud.overlap(target, T, MAX_DISTANCE)),
                    (name + " unmatched", lambda cloud=cloud, target=target: cloud.overlap(target, T, MAX_DISTANCE, keep="unmatched"))]
            if torch is not None:
                mine.append((name + " knn path", knn_path))
            if cKDTree is not None:
                mine.append((name + " host route", host_route))
            settings += mine
            st = cloud.overlap(target, T, MAX_DISTANCE)
            extra = ""
            if torch is not None:
                extra += ", %d by the knn path" % int(np.isfinite(knn_path().numpy()).sum())
            if cKDTree is not None:
                extra += ", %d by the host route" % host_route()[1]
            notes.append("%s = %d points against %s of %d %s: %d matched (fitness %.4f, rmse %.4f m)%s" % (label, n, tname, tn, "points" if tname == "kd" else "voxels", st["matched"], st["fitness"], st["rmse"], extra))

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
    lines = ["# scripts/cloud_overlap_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# PointCloud.overlap(target, T, max_distance = %g m): statistics only / with the cloud of the unmatched points; the knn path (transformed, to_torch, batch_knn_search_torch k = 1, the distances"
             % MAX_DISTANCE,
             "#     downloaded: %s); the host route (download cloud and target, %s, mask, upload)" % ("measured" if torch is not None else "torch is missing: not measured", "scipy cKDTree" if cKDTree is not None else "scipy is missing: not measured"),
             "# target: %d scans through the %g m voxel grid merged at the generator's poses (%d points), its KdTree, and the one-shot Gaussian map over it (leaf %g m, %d voxels, search offsets 1)"
             % (WINDOW, RES, submap.size(), LEAF, gmap.size())]
    lines += ["# " + s for s in notes]
    lines.append("# (against the map the host route takes the nearest mean ANYWHERE, the device the mean of the query's own voxel: the host matches more)")
    med, lo, hi = {}, {}, {}
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        med[name], lo[name], hi[name] = float(np.median(v)), float(v.min()), float(v.max())
        lines.append("%-22s %10.1f (%8.1f .. %8.1f)" % (name, med[name], lo[name], hi[name]))
    for label, _ in clouds:
        for tname, _, _, _ in targets:
            name = "%s %s" % (label, tname)
            for other in (" knn path", " host route"):
                if name + other in med:
                    f, g = name + " stats", name + other
                    lines.append("%s: statistics only against the%s: median %.3f x; slowest overlap region below the other's fastest: %s" % (name, other, med[f] / med[g], "yes" if hi[f] < lo[g] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

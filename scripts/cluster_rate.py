#!/usr/bin/env python3
"""Wall time of the fixed-radius calls on the device beside the host route and beside the nearest existing walk,
in the same process and build (the protocol of scripts/place_rate.py).

Two clouds from synthetic.kitti_like_scan(0) with the ground cropped (z > -1.5 m in the sensor frame): the 0.25 m voxel grid ("down") and
the raw sweep ("raw"); eps 0.5 m.
      clusters mp1 tree     PointCloud.clusters(0.5, min_points 1, tree)           six commands, one wait
      clusters mp4 tree     ... min_points 4                                       eight commands
      clusters mp1 temp     ... min_points 1, a temporary tree
      clusters mp4 temp
      radius counts         KdTree.radius_search(cloud, 0.5, return_lists=False)   two commands, one wait
      radius lists          ... with lists, room for the total given               five commands, two waits
      covariances k20       estimate_covariances(cloud, tree, 20): the nearest existing walk, on the same points and tree
      host route            the cloud downloaded, scipy.spatial.cKDTree.query_pairs + connected_components (min_points 1), the labels
                            uploaded as a device array — `--host-reps` regions
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/cluster_rate.py [--reps 9] [--host-reps 3] [--out profiles/cloud_cluster_rate.txt]
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/cluster_rate.py --reps 3 --host-reps 0     (the kernel trace: a run of its own)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import synthetic  # noqa: E402

EPS = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sga.Context()
    pts, _ = synthetic.kitti_like_scan(0)
    raw = sga.PointCloud(pts, ctx=ctx).cropped(box=((-1e9, -1e9, -1.5), (1e9, 1e9, 1e9)))
    down = sga.voxelgrid_sampling(raw, 0.25)
    lines = ["# scripts/cluster_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps]

    def region(fn):
        t0 = time.perf_counter()
        keep = fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        del keep
        return dt

    for name, cloud in (("down", down), ("raw", raw)):
        tree = sga.KdTree(cloud)
        counts = tree.radius_search(cloud, EPS, return_lists=False)
        total = int(counts.sum())
        first = {mp: cloud.clusters(EPS, mp, tree=tree, return_table=False) for mp in (1, 4)}
        host_parts = []

        def host_route():
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import connected_components
            from scipy.spatial import cKDTree

            t0 = time.perf_counter()
            p = cloud.xyz().astype(np.float64)
            t1 = time.perf_counter()
            pairs = cKDTree(p).query_pairs(EPS, output_type="ndarray")
            t2 = time.perf_counter()
            g = coo_matrix((np.ones(len(pairs), np.int8), (pairs[:, 0], pairs[:, 1])), shape=(len(p), len(p)))
            _, labels = connected_components(g, directed=False)
            t3 = time.perf_counter()
            up = sga.PointCloud(np.stack([labels.astype(np.float32)] * 3, 1), ctx=ctx)  # the labels' way back: n x 12 bytes, three times what they need
            t4 = time.perf_counter()
            host_parts.append((t1 - t0, t2 - t1, t3 - t2, t4 - t3))
            return up

        settings = [
            ("clusters mp1 tree", lambda: cloud.clusters(EPS, 1, tree=tree, return_table=False)),
            ("clusters mp4 tree", lambda: cloud.clusters(EPS, 4, tree=tree, return_table=False)),
            ("clusters mp1 temp", lambda: cloud.clusters(EPS, 1, return_table=False)),
            ("clusters mp4 temp", lambda: cloud.clusters(EPS, 4, return_table=False)),
            ("radius counts", lambda: tree.radius_search(cloud, EPS, return_lists=False)),
            ("radius lists", lambda: tree.radius_search(cloud, EPS, capacity=total)),
            ("covariances k20", lambda: sga.estimate_covariances(cloud, tree, 20)),
        ]
        for _, fn in settings:
            region(fn)
            region(fn)
        t = {label: [] for label, _ in settings}
        for _ in range(a.reps):
            for label, fn in settings:
                t[label].append(region(fn))
        host = [region(host_route) for _ in range(a.host_reps)]
        lines.append("# %s: %d points, eps %.2f m: %d neighbours in all (%.1f per point, at most %d); min_points 1: %d clusters; min_points 4: %d clusters, %d noise points" % (
            name, cloud.size(), EPS, total, total / max(1, cloud.size()), int(counts.max()), first[1]["num_clusters"], first[4]["num_clusters"], first[4]["noise"]))
        for label, _ in settings:
            v = 1e6 * np.array(t[label])
            lines.append("%-5s %-18s %12.1f (%10.1f .. %10.1f)" % (name, label, float(np.median(v)), float(v.min()), float(v.max())))
        if host:
            v = 1e6 * np.array(host)
            lines.append("%-5s %-18s %12.1f (%10.1f .. %10.1f)   %d region(s); download %.1f ms, query_pairs %.1f ms, components %.1f ms, upload %.1f ms in the last" % (
                name, "host route", float(np.median(v)), float(v.min()), float(v.max()), len(host), *(1e3 * np.array(host_parts[-1]))))
            lines.append("%-5s host route, fastest region / clusters mp1 tree, slowest region: %.1f x" % (name, min(host) / max(t["clusters mp1 tree"])))
        else:
            lines.append("%-5s host route         not measured in this run" % name)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

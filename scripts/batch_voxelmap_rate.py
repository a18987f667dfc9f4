#!/usr/bin/env python3
"""Wall time per map of the batched Gaussian voxel-map build (sga_index_build_gaussian_voxelmap_batch) against the two lone ways of doing
the same work, on the same clouds in the same process (the protocol of scripts/batch_preprocess_rate.py).

Clouds: C5-shaped (synthetic.kitti_like_scan after the 0.25 m voxel grid, ~11k points, with covariances k = 20); the work is the one-shot
map of every cloud at a 1 m leaf.  Uploads, the voxel grid, the kd-trees and the covariances are outside the timed regions; a region ends
with the context(s) synchronised and includes destroying nothing (the maps are dropped after the clock stops).  For B in 1 .. 32:
  batch   one build_gaussian_voxelmaps over the B clouds
  lone    B GaussianVoxelMap.from_cloud calls one after the other on one stream-ordered context
  2ctx    the clouds spread over two stream-ordered contexts and two threads (what the flow driver does)
After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a repetition; median and
(min .. max) per map in microseconds.  --profile B: only the batch at that size, a few times (for a run under
rocprofv3 --kernel-trace --stats of its own).

  python scripts/batch_voxelmap_rate.py [--reps 9] [--sizes 1,2,4,8,16,32] [--leaf 1.0] [--out profiles/batch_voxelmap_rate.txt]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0)
    ap.add_argument("--leaf", type=float, default=1.0)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes + [a.profile])
    ctxs = [sga.Context(0), sga.Context(0)]
    for c in ctxs:
        c.set_stream_ordered(True)
    scans = [np.ascontiguousarray(sga.synthetic.kitti_like_scan(f)[0][:, :3], dtype=np.float32) for f in range(9)]
    # cloud k = scan k % 9 after the grid, with covariances; each context has its own copies
    clouds = [[sga.voxelgrid_sampling(sga.PointCloud(scans[k % 9], ctx=c), 0.25) for k in range(nmax)] for c in ctxs]
    for cs in clouds:
        sga.preprocess_batch(cs, 20)
    for c in ctxs:
        c.synchronize()
    sizes_pts = [cl.size() for cl in clouds[0][:9]]

    def lone_work(cs, keep):
        for cl in cs:
            keep.append(sga.GaussianVoxelMap.from_cloud(cl, a.leaf))

    def run_forest(B):
        t0 = time.perf_counter()
        maps = sga.build_gaussian_voxelmaps(clouds[0][:B], a.leaf)
        ctxs[0].synchronize()
        dt = time.perf_counter() - t0
        del maps
        return dt

    def run_lone(B):
        keep = []
        t0 = time.perf_counter()
        lone_work(clouds[0][:B], keep)
        ctxs[0].synchronize()
        return time.perf_counter() - t0

    def run_two(B):
        parts = [(0, clouds[0][0:B:2]), (1, clouds[1][1:B:2])]
        keep = [[], []]

        def work(ci, cs):
            lone_work(cs, keep[ci])
            ctxs[ci].synchronize()

        ths = [threading.Thread(target=work, args=p) for p in parts if p[1]]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        return time.perf_counter() - t0

    if a.profile:
        for _ in range(5):
            run_forest(a.profile)
        print("profiled %d batches of %d clouds" % (5, a.profile))
        return
    modes = [("batch", run_forest), ("lone", run_lone), ("2ctx", run_two)]
    for B in sizes:  # warm-up: code objects, allocator, first touch
        for _, fn in modes:
            fn(B)
            fn(B)
    t = {(m, B): [] for m, _ in modes for B in sizes}
    for _ in range(a.reps):
        for B in sizes:
            for m, fn in modes:
                t[(m, B)].append(fn(B))
    lines = ["# scripts/batch_voxelmap_rate.py: wall time per map [us] of the one-shot Gaussian voxel-map build (leaf %g m), median" % a.leaf + " (min .. max) of %d timed regions, settings alternating" % a.reps,
             "# C5-shaped clouds, %d .. %d points after the 0.25 m grid; uploads, the grid and the covariances outside the timed region; stream-ordered contexts, a region ends synchronised" % (min(sizes_pts), max(sizes_pts)),
             "# batch = one build_gaussian_voxelmaps; lone = B GaussianVoxelMap.from_cloud calls on one context; 2ctx = the clouds over two contexts and threads",
             "%4s  %28s  %28s  %28s  %11s  %11s  %s" % ("B", "batch", "lone", "2ctx", "lone/batch", "2ctx/batch", "batch max < lone min")]
    for B in sizes:
        cells, med, lo, hi = [], {}, {}, {}
        for m, _ in modes:
            v = 1e6 * np.array(t[(m, B)]) / B
            med[m], lo[m], hi[m] = float(np.median(v)), float(v.min()), float(v.max())
            cells.append("%8.1f (%7.1f .. %7.1f)" % (med[m], lo[m], hi[m]))
        lines.append("%4d  %28s  %28s  %28s  %11.2f  %11.2f  %s" % (B, cells[0], cells[1], cells[2], med["lone"] / med["batch"], med["2ctx"] / med["batch"], "yes" if hi["batch"] < lo["lone"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

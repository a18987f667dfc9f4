#!/usr/bin/env python3
"""Wall time per insert of the batched incremental voxel-map insert (sga_voxelmap_insert_batch) against the two lone ways of doing the same
work, on the same clouds in the same process (the protocol of scripts/batch_voxelmap_rate.py).

Clouds: C5-shaped (synthetic.kitti_like_scan after the 0.25 m voxel grid, ~11k points, with covariances k = 20); the maps are incremental
Gaussian maps at a 1 m leaf.  Before every timed region map k is made afresh and given scan k % 9 at the identity (outside the region); the
region inserts scan (k + 1) % 9 at a small forward motion into it, so existing and new voxels are mixed (and most maps grow).  Uploads, the
voxel grid, the covariances and the first inserts are outside the timed regions; a region ends with the context(s) synchronised.  For B in
1 .. 32:
  batch   one insert_batch over the B maps
  lone    B insert calls one after the other on one stream-ordered context
  2ctx    the maps spread over two stream-ordered contexts and two threads
After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a repetition; median and
(min .. max) per insert in microseconds.  --profile B: only the batch at that size, a few times (for a run under
rocprofv3 --kernel-trace --stats of its own).

  python scripts/batch_voxelmap_insert_rate.py [--reps 9] [--sizes 1,2,4,8,16,32] [--leaf 1.0] [--out profiles/batch_voxelmap_insert_rate.txt]
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
    # cloud k = scan k % 9 after the grid, with covariances; each context has its own copies (one more than maps: map k receives cloud k + 1)
    clouds = [[sga.voxelgrid_sampling(sga.PointCloud(scans[k % 9], ctx=c), 0.25) for k in range(nmax + 1)] for c in ctxs]
    for cs in clouds:
        sga.preprocess_batch(cs, 20)
    for c in ctxs:
        c.synchronize()
    sizes_pts = [cl.size() for cl in clouds[0][:9]]
    step = np.eye(4)  # the motion between two scans: a metre forward, a little yaw
    yaw = 0.01
    step[:2, :2] = [[np.cos(yaw), -np.sin(yaw)], [np.sin(yaw), np.cos(yaw)]]
    step[:3, 3] = [1.0, 0.05, 0.0]

    def models(ci, ks):
        """fresh maps holding scan k, for k in ks, on context ci"""
        maps = []
        for k in ks:
            m = sga.GaussianVoxelMap(a.leaf, ctx=ctxs[ci])
            m.insert(clouds[ci][k])
            maps.append(m)
        ctxs[ci].synchronize()
        return maps

    def run_batch(B):
        maps = models(0, range(B))
        t0 = time.perf_counter()
        sga.insert_batch(maps, clouds[0][1 : B + 1], [step] * B)
        ctxs[0].synchronize()
        return time.perf_counter() - t0

    def run_lone(B):
        maps = models(0, range(B))
        t0 = time.perf_counter()
        for k, m in enumerate(maps):
            m.insert(clouds[0][k + 1], step)
        ctxs[0].synchronize()
        return time.perf_counter() - t0

    def run_two(B):
        parts = [(0, list(range(0, B, 2))), (1, list(range(1, B, 2)))]
        maps = [models(ci, ks) for ci, ks in parts]

        def work(ci, ks):
            for k, m in zip(ks, maps[ci]):
                m.insert(clouds[ci][k + 1], step)
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
            run_batch(a.profile)
        print("profiled %d batches of %d inserts" % (5, a.profile))
        return
    modes = [("batch", run_batch), ("lone", run_lone), ("2ctx", run_two)]
    for B in sizes:  # warm-up: code objects, allocator, first touch
        for _, fn in modes:
            fn(B)
            fn(B)
    t = {(m, B): [] for m, _ in modes for B in sizes}
    for _ in range(a.reps):
        for B in sizes:
            for m, fn in modes:
                t[(m, B)].append(fn(B))
    lines = ["# scripts/batch_voxelmap_insert_rate.py: wall time per insert [us] into an incremental Gaussian voxel map (leaf %g m) that holds the scan before, median" % a.leaf + " (min .. max) of %d timed regions, settings alternating" % a.reps,
             "# C5-shaped clouds, %d .. %d points after the 0.25 m grid; uploads, the grid, the covariances and the first insert of every map outside the timed region; stream-ordered contexts, a region ends synchronised" % (min(sizes_pts), max(sizes_pts)),
             "# batch = one insert_batch; lone = B insert calls on one context; 2ctx = the maps over two contexts and threads",
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

#!/usr/bin/env python3
"""Wall time per cloud of the batched voxel grid (sga_voxelgrid_sampling_batch) against the two lone ways of doing the same work, on the
same clouds in the same process.

Clouds: C5-shaped raw scans (synthetic.kitti_like_scan, ~115k points), leaf 0.25 m.  Uploads are outside the timed regions; a region ends
with the context(s) synchronised and includes destroying nothing (the outputs are dropped after the clock stops).  For B in 1 .. 32:
  batch   one voxelgrid_sampling_batch over the B clouds
  lone    B voxelgrid_sampling calls one after the other on one stream-ordered context
  2ctx    the clouds spread over two stream-ordered contexts and two threads (what the flow driver does)
After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a repetition; median and
(min .. max) per cloud in microseconds.  --profile B: only the batched call at that size, a few times (for a run under
rocprofv3 --kernel-trace --stats of its own).

  python scripts/batch_voxelgrid_rate.py [--reps 9] [--sizes 1,2,4,8,16,32] [--out profiles/batch_voxelgrid_rate.txt]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

LEAF = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--sizes", default="1,2,4,8,16,32")
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", type=int, default=0)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes + [a.profile])
    ctxs = [sga.Context(0), sga.Context(0)]
    for c in ctxs:
        c.set_stream_ordered(True)
    scans = [np.ascontiguousarray(sga.synthetic.kitti_like_scan(f)[0][:, :3], dtype=np.float32) for f in range(9)]
    clouds = [[sga.PointCloud(scans[k % 9], ctx=c) for k in range(nmax)] for c in ctxs]  # cloud k = scan k % 9, a copy per context
    for c in ctxs:
        c.synchronize()
    sizes_pts = [cl.size() for cl in clouds[0][:9]]

    def run_batch(B):
        t0 = time.perf_counter()
        outs = sga.voxelgrid_sampling_batch(clouds[0][:B], LEAF)
        ctxs[0].synchronize()
        dt = time.perf_counter() - t0
        del outs
        return dt

    def run_lone(B):
        t0 = time.perf_counter()
        outs = [sga.voxelgrid_sampling(cl, LEAF) for cl in clouds[0][:B]]
        ctxs[0].synchronize()
        dt = time.perf_counter() - t0
        del outs
        return dt

    def run_two(B):
        parts = [(0, clouds[0][0:B:2]), (1, clouds[1][1:B:2])]
        keep = [[], []]

        def work(ci, cs):
            keep[ci].extend(sga.voxelgrid_sampling(cl, LEAF) for cl in cs)
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
        print("profiled %d batched voxel grids of %d clouds: plan %s" % (5, a.profile, api._voxelgrid_batch_plan(clouds[0][: a.profile], LEAF)))
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
    lines = ["# scripts/batch_voxelgrid_rate.py: wall time per cloud [us] of the voxel grid (leaf %.2f m), median (min .. max) of %d timed regions, settings alternating" % (LEAF, a.reps),
             "# C5-shaped raw scans, %d .. %d points; uploads outside the timed region; stream-ordered contexts, a region ends synchronised" % (min(sizes_pts), max(sizes_pts)),
             "# batch = one voxelgrid_sampling_batch; lone = B voxelgrid_sampling calls on one context; 2ctx = the clouds over two contexts and threads; key = bytes of the batch's composite sort key",
             "%4s  %3s  %28s  %28s  %28s  %10s  %10s  %s" % ("B", "key", "batch", "lone", "2ctx", "lone/batch", "2ctx/batch", "batch max < lone min")]
    for B in sizes:
        cells, med, lo, hi = [], {}, {}, {}
        for m, _ in modes:
            v = 1e6 * np.array(t[(m, B)]) / B
            med[m], lo[m], hi[m] = float(np.median(v)), float(v.min()), float(v.max())
            cells.append("%8.1f (%7.1f .. %7.1f)" % (med[m], lo[m], hi[m]))
        key = api._voxelgrid_batch_plan(clouds[0][:B], LEAF)["key_bytes"]
        lines.append("%4d  %3d  %28s  %28s  %28s  %10.2f  %10.2f  %s" % (B, key, cells[0], cells[1], cells[2], med["lone"] / med["batch"], med["2ctx"] / med["batch"], "yes" if hi["batch"] < lo["lone"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

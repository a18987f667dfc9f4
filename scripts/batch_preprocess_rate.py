#!/usr/bin/env python3
"""Wall time per cloud of the batched preprocessing (sga_index_build_kdtree_batch + sga_estimate_normals_covariances_batch) against the
two lone ways of doing the same work, on the same clouds in the same process.

Clouds: C5-shaped (synthetic.kitti_like_scan after the 0.25 m voxel grid, ~11k points: the scans scripts/batch_rate.py uses); the work is
the kd-tree and the covariances (k = 20) of every cloud.  Uploads and the voxel grid are outside the timed regions; a region ends with
the context(s) synchronised and includes destroying nothing (the trees are dropped after the clock stops).  For B in 1 .. 32:
  forest  one preprocess_batch over the B clouds
  lone    B (KdTree, estimate_covariances) call pairs one after the other on one stream-ordered context
  2ctx    the clouds spread over two stream-ordered contexts and two threads (what the flow driver does)
After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a repetition; median and
(min .. max) per cloud in microseconds.  --profile B: only the forest at that size, a few times (for a run under
rocprofv3 --kernel-trace --stats of its own).

  python scripts/batch_preprocess_rate.py [--reps 9] [--sizes 1,2,4,8,16,32] [--out profiles/batch_preprocess_rate.txt]
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
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes + [a.profile])
    ctxs = [sga.Context(0), sga.Context(0)]
    for c in ctxs:
        c.set_stream_ordered(True)
    scans = [np.ascontiguousarray(sga.synthetic.kitti_like_scan(f)[0][:, :3], dtype=np.float32) for f in range(9)]
    # cloud k = scan k % 9 after the grid; each context has its own copies (a cloud may appear once in a batched estimation)
    clouds = [[sga.voxelgrid_sampling(sga.PointCloud(scans[k % 9], ctx=c), 0.25) for k in range(nmax)] for c in ctxs]
    for c in ctxs:
        c.synchronize()
    sizes_pts = [cl.size() for cl in clouds[0][:9]]

    def lone_work(cs, keep):
        for cl in cs:
            tree = sga.KdTree(cl)
            sga.estimate_covariances(cl, tree, 20)
            keep.append(tree)

    def run_forest(B):
        t0 = time.perf_counter()
        pairs = sga.preprocess_batch(clouds[0][:B], 20)
        ctxs[0].synchronize()
        dt = time.perf_counter() - t0
        del pairs
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
        print("profiled %d forests of %d clouds" % (5, a.profile))
        return
    modes = [("forest", run_forest), ("lone", run_lone), ("2ctx", run_two)]
    for B in sizes:  # warm-up: code objects, allocator, first touch
        for _, fn in modes:
            fn(B)
            fn(B)
    t = {(m, B): [] for m, _ in modes for B in sizes}
    for _ in range(a.reps):
        for B in sizes:
            for m, fn in modes:
                t[(m, B)].append(fn(B))
    lines = ["# scripts/batch_preprocess_rate.py: wall time per cloud [us] of kd-tree build + covariances (k = 20), median (min .. max) of %d timed regions, settings alternating" % a.reps,
             "# C5-shaped clouds, %d .. %d points after the 0.25 m grid; uploads and the voxel grid outside the timed region; stream-ordered contexts, a region ends synchronised" % (min(sizes_pts), max(sizes_pts)),
             "# forest = one preprocess_batch; lone = B (build, estimate) call pairs on one context; 2ctx = the clouds over two contexts and threads",
             "%4s  %28s  %28s  %28s  %11s  %11s  %s" % ("B", "forest", "lone", "2ctx", "lone/forest", "2ctx/forest", "forest max < lone min")]
    for B in sizes:
        cells, med, lo, hi = [], {}, {}, {}
        for m, _ in modes:
            v = 1e6 * np.array(t[(m, B)]) / B
            med[m], lo[m], hi[m] = float(np.median(v)), float(v.min()), float(v.max())
            cells.append("%8.1f (%7.1f .. %7.1f)" % (med[m], lo[m], hi[m]))
        lines.append("%4d  %28s  %28s  %28s  %11.2f  %11.2f  %s" % (B, cells[0], cells[1], cells[2], med["lone"] / med["forest"], med["2ctx"] / med["forest"], "yes" if hi["forest"] < lo["lone"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

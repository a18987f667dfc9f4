#!/usr/bin/env python3
"""Wall time per problem of the batched problem creation (sga_problem_create_batch) against the two lone ways of doing the same work, on
the same clouds in the same process (the protocol of scripts/batch_voxelmap_insert_rate.py).

Clouds: C5-shaped (synthetic.kitti_like_scan after the 0.25 m voxel grid, ~11k points, with covariances k = 20).  Pair k is scan
(k + 1) % 9 against scan k % 9 from the identity — against the 1 m Gaussian voxel map of the scan before (`map`) and against its
kd-tree (`kd`).  Uploads, the voxel grid, the covariances, the maps and the trees are outside the timed regions, and so is the
destruction of the problems; a region ends with the context(s) synchronised.  For B in 1 .. 32:
  batch   one create_problems over the B pairs
  lone    B Problem(...) calls one after the other on one stream-ordered context
  2ctx    the pairs spread over two stream-ordered contexts and two threads
After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a repetition; median and
(min .. max) per problem in microseconds.  --label names the build in the header (two builds with different sorts in the chain are
compared by running the script once per library: SGA_LIB_PATH).  --append adds to --out.

  python scripts/batch_problem_rate.py [--reps 9] [--sizes 1,2,4,8,16,32] [--label merge_sort] [--out profiles/batch_problem_rate.txt] [--append]
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
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--label", default="")
    ap.add_argument("--leaf", type=float, default=1.0)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    nmax = max(sizes)
    ctxs = [sga.Context(0), sga.Context(0)]
    for c in ctxs:
        c.set_stream_ordered(True)
    scans = [np.ascontiguousarray(sga.synthetic.kitti_like_scan(f)[0][:, :3], dtype=np.float32) for f in range(9)]
    # cloud k = scan k % 9 after the grid, with covariances; each context has its own copies, maps and trees (pair k: target k, source k + 1)
    clouds = [[sga.voxelgrid_sampling(sga.PointCloud(scans[k % 9], ctx=c), 0.25) for k in range(nmax + 1)] for c in ctxs]
    trees = [[tree for _, tree in sga.preprocess_batch(cs, 20)] for cs in clouds]
    maps = [sga.build_gaussian_voxelmaps(cs, a.leaf) for cs in clouds]
    for c in ctxs:
        c.synchronize()
    sizes_pts = [cl.size() for cl in clouds[0][:9]]
    targets = {"map": maps, "kd": trees}
    eye = np.eye(4)

    def run_batch(kind, B):
        t0 = time.perf_counter()
        pbs = sga.create_problems(targets[kind][0][:B], clouds[0][1 : B + 1], None, ctx=ctxs[0])
        ctxs[0].synchronize()
        dt = time.perf_counter() - t0
        del pbs
        return dt

    def run_lone(kind, B):
        t0 = time.perf_counter()
        pbs = [sga.Problem(targets[kind][0][k], clouds[0][k + 1], eye, ctx=ctxs[0]) for k in range(B)]
        ctxs[0].synchronize()
        dt = time.perf_counter() - t0
        del pbs
        return dt

    def run_two(kind, B):
        parts = [(0, list(range(0, B, 2))), (1, list(range(1, B, 2)))]
        keep = [[], []]

        def work(ci, ks):
            keep[ci] = [sga.Problem(targets[kind][ci][k], clouds[ci][k + 1], eye, ctx=ctxs[ci]) for k in ks]
            ctxs[ci].synchronize()

        ths = [threading.Thread(target=work, args=p) for p in parts if p[1]]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        dt = time.perf_counter() - t0
        del keep
        return dt

    modes = [("batch", run_batch), ("lone", run_lone), ("2ctx", run_two)]
    kinds = ["map", "kd"]
    for kind in kinds:  # warm-up: code objects, allocator, first touch
        for B in sizes:
            for _, fn in modes:
                fn(kind, B)
                fn(kind, B)
    t = {(kind, m, B): [] for kind in kinds for m, _ in modes for B in sizes}
    for _ in range(a.reps):
        for kind in kinds:
            for B in sizes:
                for m, fn in modes:
                    t[(kind, m, B)].append(fn(kind, B))
    lines = ["# scripts/batch_problem_rate.py%s: wall time per problem [us], median (min .. max) of %d timed regions, settings alternating" % (" [" + a.label + "]" if a.label else "", a.reps),
             "# C5-shaped clouds, %d .. %d points after the 0.25 m grid, pair k = scan k + 1 against scan k from the identity; uploads, the grid, the covariances, the maps (leaf %g m), the trees and the destruction of the problems outside the timed region; stream-ordered contexts, a region ends synchronised"
             % (min(sizes_pts), max(sizes_pts), a.leaf),
             "# batch = one create_problems; lone = B Problem(...) calls on one context; 2ctx = the pairs over two contexts and threads"]
    for kind in kinds:
        lines.append("# target: %s" % ("the 1 m Gaussian voxel map of the scan before" if kind == "map" else "the kd-tree of the scan before"))
        lines.append("%4s  %28s  %28s  %28s  %11s  %11s  %s" % ("B", "batch", "lone", "2ctx", "lone/batch", "2ctx/batch", "batch max < lone min"))
        for B in sizes:
            cells, med, lo, hi = [], {}, {}, {}
            for m, _ in modes:
                v = 1e6 * np.array(t[(kind, m, B)]) / B
                med[m], lo[m], hi[m] = float(np.median(v)), float(v.min()), float(v.max())
                cells.append("%8.1f (%7.1f .. %7.1f)" % (med[m], lo[m], hi[m]))
            lines.append("%4d  %28s  %28s  %28s  %11.2f  %11.2f  %s" % (B, cells[0], cells[1], cells[2], med["lone"] / med["batch"], med["2ctx"] / med["batch"], "yes" if hi["batch"] < lo["lone"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "a" if a.append else "w").write(text + "\n")


if __name__ == "__main__":
    main()

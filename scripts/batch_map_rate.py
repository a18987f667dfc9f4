#!/usr/bin/env python3
"""Wall time per registered pair of sga_align_batch over voxel-map targets (VGICP) against the two lone ways of doing the same work, on the
same pairs in the same process (scripts/batch_rate.py's procedure; there the targets are kd-trees).

Pairs: C5-shaped (synthetic.kitti_like_scan, 0.25 m voxel grid, covariances k = 20, ~11k points), each scan registered from the identity
against a Gaussian voxel map (leaf 1.0 m) of the previous scan with the default setting (GICP factor, LM).  Preprocessing, the maps and
problem creation are outside the timed regions.  For B in 1 .. 32:
  batch   one BatchProblem.align over the B pairs
  lone    B Problem.align calls one after the other on one context
  2ctx    the pairs spread over two contexts and two threads (what the flow driver does)
After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a repetition; median and
(min .. max) per pair in microseconds.  --profile B: only the batched form at that size, a few times (for a run under
rocprofv3 --kernel-trace --stats of its own: the GPU time of batch_map_linearize_kernel / batch_reduce_rows_kernel per round).

  python scripts/batch_map_rate.py [--reps 9] [--sizes 1,2,4,8,16,32] [--out profiles/batch_map_rate.txt]
"""
import argparse
import os
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402


def preprocess(ctx, frame):
    pts, _ = sga.synthetic.kitti_like_scan(frame)
    cloud = sga.voxelgrid_sampling(sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32), ctx=ctx), 0.25)
    sga.estimate_covariances(cloud, sga.KdTree(cloud), 20)
    vmap = sga.GaussianVoxelMap(1.0, ctx=ctx)
    vmap.insert(cloud)
    return cloud, vmap


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
    st = sga.make_setting("GICP")
    # scans 0 .. 8 (nine distinct frames), pair k = (frame k % 8, frame k % 8 + 1); each context has its own copies of everything
    frames = [[preprocess(c, f) for f in range(9)] for c in ctxs]
    for c in ctxs:
        c.synchronize()
    sizes_pts = [frames[0][f][0].size() for f in range(9)]

    def problems(ci, ks):
        return [sga.Problem(frames[ci][k % 8][1], frames[ci][k % 8 + 1][0], np.eye(4), ctx=ctxs[ci]) for k in ks]

    pb_lone = problems(0, range(nmax))
    pb_batch = problems(0, range(nmax))
    pb_two = [problems(0, range(0, nmax, 2)), problems(1, range(1, nmax, 2))]
    batches = {B: sga.BatchProblem(pb_batch[:B]) for B in set(sizes + ([a.profile] if a.profile else []))}
    iters = {}

    def run_batch(B):
        t0 = time.perf_counter()
        res = batches[B].align(st)
        dt = time.perf_counter() - t0
        iters[B] = sum(r.iterations + 1 for r in res)
        return dt

    def run_lone(B):
        t0 = time.perf_counter()
        for pb in pb_lone[:B]:
            pb.align(st)
        return time.perf_counter() - t0

    def run_two(B):
        parts = [pb_two[0][: (B + 1) // 2], pb_two[1][: B // 2]]

        def work(ps):
            for pb in ps:
                pb.align(st)

        ths = [threading.Thread(target=work, args=(p,)) for p in parts if p]
        t0 = time.perf_counter()
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        return time.perf_counter() - t0

    if a.profile:
        for _ in range(5):
            run_batch(a.profile)
        print("profiled %d batched registrations of %d pairs, %d linearizations per pair on average" % (5, a.profile, iters[a.profile] / a.profile))
        return
    modes = [("batch", run_batch), ("lone", run_lone), ("2ctx", run_two)]
    for B in sizes:  # warm-up: code objects, allocator, first-touch
        for _, fn in modes:
            fn(B)
            fn(B)
    t = {(m, B): [] for m, _ in modes for B in sizes}
    for _ in range(a.reps):
        for B in sizes:
            for m, fn in modes:
                t[(m, B)].append(fn(B))
    lines = ["# scripts/batch_map_rate.py: wall time per registered pair [us], median (min .. max) of %d timed regions, settings alternating" % a.reps,
             "# C5-shaped pairs, %d .. %d points after the 0.25 m grid, against a Gaussian voxel map (leaf 1.0 m) of the previous scan, GICP factor, default setting, from the identity; maps and problems created outside the timed region" % (min(sizes_pts), max(sizes_pts)),
             "# batch = one sga_align_batch; lone = B sga_align_problem calls on one context; 2ctx = the pairs over two contexts and threads",
             "%4s  %28s  %28s  %28s  %10s  %10s  %s" % ("B", "batch", "lone", "2ctx", "lone/batch", "2ctx/batch", "linearizations/pair")]
    for B in sizes:
        cells, med = [], {}
        for m, _ in modes:
            v = 1e6 * np.array(t[(m, B)]) / B
            med[m] = float(np.median(v))
            cells.append("%8.1f (%7.1f .. %7.1f)" % (med[m], v.min(), v.max()))
        lines.append("%4d  %28s  %28s  %28s  %10.2f  %10.2f  %.2f" % (B, cells[0], cells[1], cells[2], med["lone"] / med["batch"], med["2ctx"] / med["batch"], iters[B] / B))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")
    for b in batches.values():
        b.__del__()  # before their problems


if __name__ == "__main__":
    main()

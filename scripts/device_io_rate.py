#!/usr/bin/env python3
"""Wall time of making a cloud from data that is on the device already (PointCloud.from_torch: sga_cloud_create_device) against the two
host uploads of the same values, in the same process and build (the protocol of scripts/batch_problem_rate.py).

Two sizes: the C5-shaped raw scan (synthetic.kitti_like_scan, ~115k points) and a 1M-point cloud (the shape of fresh_align_c3).  For each
  create    cloud creation alone
  chain     creation + 0.25 m voxel grid + kd-tree + covariances (k = 10)
from
  device    a float32 (N,3) tensor on the GPU (already there: its production is not part of the region)
  pinned    a pinned host array (sga_host_alloc: the device reads it in place)
  pageable  an ordinary numpy array (one CPU pass into the staging ring)
A blocking context; a region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting,
the settings ALTERNATING within a repetition; median and (min .. max) in microseconds.  The baseline is the host path of the same
build, whose code the device path leaves untouched.

  python scripts/device_io_rate.py [--reps 9] [--out profiles/device_io_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sga.Context(0)
    scan = np.ascontiguousarray(sga.synthetic.kitti_like_scan(0)[0][:, :3], dtype=np.float32)
    big = np.ascontiguousarray(sga.synthetic.scene(1_000_000, 5), dtype=np.float32)
    shapes = [("C5 raw scan", scan), ("1M points", big)]
    stream = torch.cuda.current_stream(0).cuda_stream

    def chain(cloud):
        down = sga.voxelgrid_sampling(cloud, 0.25)
        tree = sga.KdTree(down)
        sga.estimate_covariances(down, tree, 10)
        return down, tree

    table = []
    for name, pts in shapes:
        sources = {"device": torch.from_numpy(pts).to("cuda:0"), "pinned": api.pinned_copy(pts), "pageable": pts}
        torch.cuda.synchronize()

        def make(kind):
            if kind == "device":
                return sga.PointCloud.from_torch(sources[kind], ctx=ctx, stream=stream)
            return sga.PointCloud(sources[kind], ctx=ctx)

        def region(kind, full):
            t0 = time.perf_counter()
            keep = make(kind)
            if full:
                keep = (keep, chain(keep))
            ctx.synchronize()
            dt = time.perf_counter() - t0
            del keep
            return dt

        settings = [(kind, full) for full in (False, True) for kind in ("device", "pinned", "pageable")]
        for s in settings:  # warm-up: code objects, allocator, the staging ring
            region(*s)
            region(*s)
        t = {s: [] for s in settings}
        for _ in range(a.reps):
            for s in settings:
                t[s].append(region(*s))
        table.append((name, len(pts), t))
    lines = ["# scripts/device_io_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a blocking context, a region ends synchronised" % a.reps,
             "# create = the cloud alone; chain = cloud + 0.25 m voxel grid + kd-tree + covariances (k = 10); device = PointCloud.from_torch of a float32 tensor, pinned / pageable = PointCloud(host array)"]
    for name, n, t in table:
        lines.append("# %s, %d points" % (name, n))
        lines.append("%8s  %32s  %32s  %32s  %s" % ("", "device", "pinned", "pageable", "device max < pinned min"))
        for full in (False, True):
            cells, lo, hi = [], {}, {}
            for kind in ("device", "pinned", "pageable"):
                v = 1e6 * np.array(t[(kind, full)])
                lo[kind], hi[kind] = float(v.min()), float(v.max())
                cells.append("%10.1f (%8.1f .. %8.1f)" % (float(np.median(v)), lo[kind], hi[kind]))
            lines.append("%8s  %32s  %32s  %32s  %s" % ("chain" if full else "create", cells[0], cells[1], cells[2], "yes" if hi["device"] < lo["pinned"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

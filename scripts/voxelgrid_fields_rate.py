#!/usr/bin/env python3
"""Wall time of the voxel grid that carries per-point columns (api.voxelgrid_sampling_fields: sga_voxelgrid_sampling_fields) against
(a) the plain voxel grid of the same input — the floor it cannot beat: the difference is the price of the columns — and (b) the host
route there was before it (download the records, partition and reduce in numpy, upload), in the same process and build (the protocol of
scripts/cloud_crop_rate.py).

Inputs: one raw C5 sweep (synthetic.kitti_like_sweep(3): about 121k points, on the device already; leaf 0.25) and a cloud of 1M points
(a Gaussian scene; leaf 0.25).  Per input:
      plain          voxelgrid_sampling(cloud, leaf)
      1 column       voxelgrid_sampling_fields(cloud, times, leaf, reduce="nearest")                the fields a Features on the device already
      4 columns      the same with four columns: nearest, mean, max, first
      4 + members    the same with return_counts and return_voxel_of (two downloads)
      host route     (the sweep only) download, numpy: keys, a stable sort, the mean of one column per run, upload of both
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.  Run it at the parent commit with --plain-only for the
    plain call's time before this change.

  python scripts/voxelgrid_fields_rate.py [--reps 9] [--plain-only] [--out profiles/voxelgrid_fields_rate.txt]
  python scripts/voxelgrid_fields_rate.py --kernels    five calls each of plain, 1 column and 4 columns on the sweep and nothing else: for a
                                                       kernel trace in a run of its own (profiles/voxelgrid_fields_kernel_stats.csv)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

LEAF = 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    ctx = sga.Context(0)
    lib = sga.load()
    pts, times = sga.synthetic.kitti_like_sweep(3)[:2]
    rng = np.random.default_rng(1)
    big = rng.normal(0.0, 20.0, (1_000_000, 3)).astype(np.float32)
    big[:, 2] = rng.uniform(-2.0, 6.0, len(big))
    inputs = [("sweep", np.ascontiguousarray(pts[:, :3], dtype=np.float32), np.asarray(times, dtype=np.float32)), ("1M", big, rng.random(len(big)).astype(np.float32))]
    settings = []
    for name, p, t in inputs:
        cloud = sga.PointCloud(p, ctx=ctx)
        settings.append((name + " plain", lambda cloud=cloud: sga.voxelgrid_sampling(cloud, LEAF)))
        if a.plain_only:
            continue
        f1 = sga.Features.from_array(t[:, None], ctx)
        f4 = sga.Features.from_array(np.stack([t, t * 255.0, np.floor(t * 20.0), 1.0 - t], axis=1), ctx)
        four = ["nearest", "mean", "max", "first"]
        settings.append((name + " 1 column", lambda cloud=cloud, f1=f1: sga.voxelgrid_sampling_fields(cloud, f1, LEAF, reduce="nearest")))
        settings.append((name + " 4 columns", lambda cloud=cloud, f4=f4: sga.voxelgrid_sampling_fields(cloud, f4, LEAF, reduce=four)))
        settings.append((name + " 4 + members", lambda cloud=cloud, f4=f4: sga.voxelgrid_sampling_fields(cloud, f4, LEAF, reduce=four, return_counts=True, return_voxel_of=True)))
        if name == "sweep":
            n = len(p)

            def host_route(cloud=cloud, t=t, n=n):
                xyz = np.empty((n, 3), np.float32)
                api.check(lib.sga_cloud_download(ctx.h, cloud.h, api._fp(xyz), None, None))
                c = np.floor(xyz.astype(np.float64) * (1.0 / LEAF)).astype(np.int64) + (1 << 20)
                key = c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)
                order = np.argsort(key, kind="stable")
                starts = np.flatnonzero(np.r_[True, key[order][1:] != key[order][:-1]])
                counts = np.diff(np.r_[starts, n])
                means = np.add.reduceat(xyz[order].astype(np.float64), starts, axis=0) / counts[:, None]
                tm = np.add.reduceat(t[order].astype(np.float64), starts) / counts
                return sga.PointCloud(means.astype(np.float32), ctx=ctx), sga.Features.from_array(tm.astype(np.float32)[:, None], ctx)

            settings.append((name + " host route", host_route))

    if a.kernels:
        for name, fn in settings:
            if name in ("sweep plain", "sweep 1 column", "sweep 4 columns"):
                for _ in range(5):
                    fn()
        ctx.synchronize()
        return

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
    lines = ["# scripts/voxelgrid_fields_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# sweep: a raw C5 sweep of %d points; 1M: a Gaussian scene of %d points; leaf %g.  plain = voxelgrid_sampling; 1 column / 4 columns = voxelgrid_sampling_fields with the fields on the device already"
             % (len(inputs[0][1]), len(big), LEAF),
             "# (nearest | nearest, mean, max, first); 4 + members = with counts and voxel_of brought to the host; host route = download, numpy partition and mean of one column, upload"]
    med = {}
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        med[name] = float(np.median(v))
        lines.append("%-18s %10.1f (%8.1f .. %8.1f)" % (name, med[name], float(v.min()), float(v.max())))
    if not a.plain_only:
        for name, _, _ in inputs:
            lines.append("%s: the price of the columns over the plain call: 1 column %+.1f us, 4 columns %+.1f us" % (name, med[name + " 1 column"] - med[name + " plain"], med[name + " 4 columns"] - med[name + " plain"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Wall time of deskewing a raw sweep on the device (PointCloud.deskewed / deskew_clouds: sga_cloud_deskew) against the only route there
was before it, in the same process and build (the protocol of scripts/cloud_merge_rate.py).

(a) One raw C5 sweep (synthetic.kitti_like_sweep(3): about 115k points, on the device already) and its times:
      host-times   cloud.deskewed(times as a numpy array, xi)       the times through the staging ring, one table copy, one launch
      tensor       cloud.deskewed(times as a torch tensor, xi)      the times read where they are
      ordered      the host-times form on a stream-ordered context  no box reduction and no wait inside the call
      host route   sga_cloud_download, the deskew in numpy float64 (one exponential per azimuth column), sga_cloud_create_f32
(b) Eight sweeps in ONE deskew_clouds call against eight lone calls.
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.
--profile: the sweep deskewed a few times from host times, for a run under
    rocprofv3 --kernel-trace --stats -- python scripts/cloud_deskew_rate.py --profile [--ordered]
(a run of its own; --ordered: a stream-ordered context, the form without the box reduction); --stats CSV then turns that run's
kernel_stats.csv into a line (mean time of deskew_cloud_kernel; 36 B per point: 16 in, 4 of time, 16 out, against the 8.0 TB/s HBM peak)
and appends it to --out.

  python scripts/cloud_deskew_rate.py [--reps 9] [--out profiles/cloud_deskew_rate.txt]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second (HBM3E, specification)


def stats_line(path, points, ordered=False):
    rows = [r for r in csv.DictReader(open(path)) if "deskew_cloud_kernel" in r["Name"]]
    if not rows:
        raise SystemExit("no deskew_cloud_kernel in " + path)
    ns = float(rows[0]["AverageNs"])
    rate = 36.0 * points / (ns * 1e-9)
    form = "stream-ordered context: no box reduction" if ordered else "blocking context: with the box reduction"
    return ("# rocprofv3 --kernel-trace --stats (a run of its own; %s): deskew_cloud_kernel, one sweep of %d points, %s calls: mean %.1f us"
            " -> 36 B x %d points / time = %.3f TB/s = %.2f %% of the 8.0 TB/s HBM peak" % (form, points, rows[0]["Calls"], ns / 1e3, points, rate / 1e12, 100.0 * rate / HBM_PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--ordered", action="store_true", help="--profile / --stats: the stream-ordered form (no box reduction)")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a --profile run under rocprofv3: append its line to --out")
    ap.add_argument("--no-torch", action="store_true", help="leave the tensor setting out")
    a = ap.parse_args()
    pts, times, _, xi, _ = sga.synthetic.kitti_like_sweep(3)
    if a.stats:
        line = stats_line(a.stats, len(pts), a.ordered)
        print(line)
        if a.out:
            open(a.out, "a").write(line + "\n")
        return
    ctx = sga.Context(0)
    cloud = sga.PointCloud(pts, ctx=ctx)
    if a.profile:
        ctx.set_stream_ordered(a.ordered)
        for _ in range(10):
            keep = sga.deskew_clouds([cloud], [times], [xi], ctx=ctx)[0]
        ctx.synchronize()
        print("profiled 10 deskews of %d points (%d)" % (len(pts), keep.size()))
        return
    octx = sga.Context(0)
    octx.set_stream_ordered(True)
    ocloud = sga.PointCloud(pts, ctx=octx)
    lib = sga.load()
    n = len(pts)
    stamps, column = np.unique(times, return_inverse=True)

    def host_times():
        return cloud.deskewed(times, xi)

    def ordered():
        return ocloud.deskewed(times, xi)

    def host_route():
        xyz = np.empty((n, 3), np.float32)
        api.check(lib.sga_cloud_download(ctx.h, cloud.h, api._fp(xyz), None, None))
        T = np.stack([sga.se3_exp((float(s) - 1.0) * xi) for s in stamps])[column]  # one exponential per azimuth column
        out = np.einsum("nij,nj->ni", T[:, :3, :3], xyz.astype(np.float64)) + T[:, :3, 3]
        return sga.PointCloud(np.ascontiguousarray(out, dtype=np.float32), ctx=ctx)

    settings = [("host-times", host_times, ctx), ("ordered", ordered, octx), ("host route", host_route, ctx)]
    if not a.no_torch:
        import torch

        dev = torch.from_numpy(times).to("cuda:0")
        torch.cuda.synchronize()
        settings.insert(1, ("tensor", lambda: cloud.deskewed(dev, xi), ctx))

    def region(fn, c):
        t0 = time.perf_counter()
        keep = fn()
        c.synchronize()
        dt = time.perf_counter() - t0
        del keep
        return dt

    # ---- (b)
    B = 8
    many = [sga.PointCloud(sga.synthetic.kitti_like_sweep(f + 1)[0], ctx=ctx) for f in range(B)]
    many_t = [sga.synthetic.kitti_like_sweep(f + 1)[1] for f in range(B)]
    xis = [xi] * B
    settings += [("8 in one call", lambda: sga.deskew_clouds(many, many_t, xis, ctx=ctx), ctx), ("8 lone calls", lambda: [c.deskewed(t, xi) for c, t in zip(many, many_t)], ctx)]
    for _, fn, c in settings:
        region(fn, c)
        region(fn, c)
    t = {name: [] for name, _, _ in settings}
    for _ in range(a.reps):
        for name, fn, c in settings:
            t[name].append(region(fn, c))
    lines = ["# scripts/cloud_deskew_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# (a) one raw C5 sweep of %d points deskewed to its end: host-times / tensor = PointCloud.deskewed on a blocking context (times from numpy / from a torch tensor); ordered = host times on a stream-ordered context (no box);" % n,
             "#     host route = download, numpy float64 deskew (one exponential per column), upload.  (b) %d sweeps (%d points) in one deskew_clouds call / in %d lone calls" % (B, sum(c.size() for c in many), B)]
    lo, hi = {}, {}
    for name, _, _ in settings:
        v = 1e6 * np.array(t[name])
        lo[name], hi[name] = float(v.min()), float(v.max())
        lines.append("%-14s %10.1f (%8.1f .. %8.1f)" % (name, float(np.median(v)), lo[name], hi[name]))
    ours = [name for name in ("host-times", "tensor", "ordered") if name in hi]
    lines.append("the library's slowest region below the host route's fastest: %s" % ("yes" if max(hi[k] for k in ours) < lo["host route"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

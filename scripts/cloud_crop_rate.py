#!/usr/bin/env python3
"""Wall time of cropping a raw sweep on the device (PointCloud.cropped / crop_clouds: sga_cloud_crop) against the only route there was
before it, in the same process and build (the protocol of scripts/cloud_deskew_rate.py).

(a) One raw C5 sweep (synthetic.kitti_like_sweep(3): about 121k points, on the device already), ranges (4, 30):
      crop           cloud.cropped(4, 30) on a blocking context             one table copy, one launch, one wait
      crop+kept      the same with return_kept=True                         the indices through the staging ring, widened on the host
      ordered        cloud.cropped(4, 30) on a stream-ordered context       it waits too: the count has to reach the host
      ordered+kept   the same with return_kept=True
      host route     sga_cloud_download, the mask in numpy float64, sga_cloud_create_f32
      deskew         cloud.deskewed(times, xi) of the same cloud            the like-sized one-launch operation, for scale
(b) Eight sweeps in ONE crop_clouds call against eight lone calls.
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/cloud_crop_rate.py [--reps 9] [--out profiles/cloud_crop_rate.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

MIN_RANGE, MAX_RANGE = 4.0, 30.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pts, times, _, xi, _ = sga.synthetic.kitti_like_sweep(3)
    ctx = sga.Context(0)
    cloud = sga.PointCloud(pts, ctx=ctx)
    octx = sga.Context(0)
    octx.set_stream_ordered(True)
    ocloud = sga.PointCloud(pts, ctx=octx)
    lib = sga.load()
    n = len(pts)

    def host_route():
        xyz = np.empty((n, 3), np.float32)
        api.check(lib.sga_cloud_download(ctx.h, cloud.h, api._fp(xyz), None, None))
        r = xyz.astype(np.float64)
        d2 = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2]
        keep = np.isfinite(r).all(axis=1) & (d2 >= MIN_RANGE * MIN_RANGE) & (d2 <= MAX_RANGE * MAX_RANGE)
        return sga.PointCloud(np.ascontiguousarray(xyz[keep]), ctx=ctx)

    settings = [
        ("crop", lambda: cloud.cropped(MIN_RANGE, MAX_RANGE), ctx),
        ("crop+kept", lambda: cloud.cropped(MIN_RANGE, MAX_RANGE, return_kept=True), ctx),
        ("ordered", lambda: ocloud.cropped(MIN_RANGE, MAX_RANGE), octx),
        ("ordered+kept", lambda: ocloud.cropped(MIN_RANGE, MAX_RANGE, return_kept=True), octx),
        ("host route", host_route, ctx),
        ("deskew", lambda: cloud.deskewed(times, xi), ctx),
    ]

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
    one = dict(min_range=MIN_RANGE, max_range=MAX_RANGE)
    settings += [("8 in one call", lambda: sga.crop_clouds(many, one, ctx=ctx), ctx), ("8 lone calls", lambda: [c.cropped(MIN_RANGE, MAX_RANGE) for c in many], ctx)]
    kept = cloud.cropped(MIN_RANGE, MAX_RANGE).size()
    assert kept == host_route().size()
    for _, fn, c in settings:
        region(fn, c)
        region(fn, c)
    t = {name: [] for name, _, _ in settings}
    for _ in range(a.reps):
        for name, fn, c in settings:
            t[name].append(region(fn, c))
    lines = ["# scripts/cloud_crop_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# (a) one raw C5 sweep of %d points cropped to ranges (%g, %g), %d kept: crop / crop+kept = PointCloud.cropped on a blocking context (without / with the indices kept); ordered / ordered+kept = the same on a"
             % (n, MIN_RANGE, MAX_RANGE, kept),
             "#     stream-ordered context; host route = download, numpy float64 mask, upload; deskew = PointCloud.deskewed of the same cloud, for scale.  (b) %d sweeps (%d points) in one crop_clouds call / in %d lone calls"
             % (B, sum(c.size() for c in many), B)]
    lo, hi = {}, {}
    for name, _, _ in settings:
        v = 1e6 * np.array(t[name])
        lo[name], hi[name] = float(v.min()), float(v.max())
        lines.append("%-14s %10.1f (%8.1f .. %8.1f)" % (name, float(np.median(v)), lo[name], hi[name]))
    ours = ("crop", "crop+kept", "ordered", "ordered+kept")
    lines.append("the crop's slowest region below the host route's fastest: %s" % ("yes" if max(hi[k] for k in ours) < lo["host route"] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Wall time of joining posed clouds into one submap cloud on the device (merge_clouds: sga_cloud_merge) against the only route there was
before it, in the same process and build (the protocol of scripts/device_io_rate.py).

(a) Ten C5-sized downsampled scans with covariances (synthetic.kitti_like_scan, 0.25 m voxel grid, k = 10), posed along the sequence's
    ground truth, joined into one cloud with covariances:
      merge   merge_clouds(clouds, poses, origin)                                              one table copy and one launch
      host    sga_cloud_download_f64 + the covariances of every scan, the transform in numpy, sga_cloud_create_f64_origin of the joined
              points, and the covariances estimated AGAIN (no host entry point takes rotated covariances in double): kd-tree + k = 10
    A blocking context; a region ends with the context synchronised.  After a warm-up of both settings, `--reps` timed regions per
    setting, the settings ALTERNATING within a repetition; median and (min .. max) in microseconds.
(c) the driver: run_synthetic_submap(20, window=5) beside run_synthetic(20) of the same run: registration ms per scan, and the submap
    driver's ate_trans_m_max.
--profile: (b) only — 8 x 125 000 points with normals and covariances merged a few times, for a run under
    rocprofv3 --kernel-trace --stats -- python scripts/cloud_merge_rate.py --profile [--ordered]
(a run of its own; --ordered: a stream-ordered context with the origin given, the form without the box reduction); --stats CSV then turns that run's kernel_stats.csv into the share of the HBM peak: 128 B per point (64 in, 64 out)
over the mean time of merge_cloud_kernel, against 8.0 TB/s, and appends it to --out.

  python scripts/cloud_merge_rate.py [--reps 9] [--out profiles/cloud_merge_rate.txt]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api, odometry  # noqa: E402

HBM_PEAK = 8.0e12  # bytes per second (HBM3E, specification)
PROFILE_MEMBERS, PROFILE_POINTS = 8, 125_000


def profile_clouds(ctx):
    rng = np.random.default_rng(0)
    clouds = []
    for _ in range(PROFILE_MEMBERS):
        p = rng.uniform(-50.0, 50.0, (PROFILE_POINTS, 3)).astype(np.float32)
        n = rng.normal(size=(PROFILE_POINTS, 3)).astype(np.float32)
        c = rng.uniform(0.0, 0.01, (PROFILE_POINTS, 6)).astype(np.float32)
        clouds.append(sga.PointCloud(p, n, c, ctx=ctx))
    return clouds


def yaw_pose(k):
    a = 0.01 * k
    T = np.eye(4)
    T[:2, :2] = [[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]]
    T[:3, 3] = (1.0 * k, 0.1 * k, 0.0)
    return T


def stats_line(path, ordered=False):
    rows = [r for r in csv.DictReader(open(path)) if "merge_cloud_kernel" in r["Name"]]
    if not rows:
        raise SystemExit("no merge_cloud_kernel in " + path)
    ns = float(rows[0]["AverageNs"])
    total = PROFILE_MEMBERS * PROFILE_POINTS
    rate = 128.0 * total / (ns * 1e-9)
    form = "stream-ordered context, origin given: no box reduction" if ordered else "blocking context: with the box reduction"
    return ("# (b) rocprofv3 --kernel-trace --stats (a run of its own; %s): merge_cloud_kernel, %d x %d points with normals and covariances, %s calls: mean %.1f us"
            " -> 128 B x %d points / time = %.2f TB/s = %.1f %% of the 8.0 TB/s HBM peak" % (form, PROFILE_MEMBERS, PROFILE_POINTS, rows[0]["Calls"], ns / 1e3, total, rate / 1e12, 100.0 * rate / HBM_PEAK))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--ordered", action="store_true", help="--profile / --stats: the stream-ordered form (no box reduction)")
    ap.add_argument("--stats", default=None, help="kernel_stats.csv of a --profile run under rocprofv3: append its line to --out")
    ap.add_argument("--frames", type=int, default=20, help="frames of the driver comparison (0: skip it)")
    a = ap.parse_args()
    if a.stats:
        line = stats_line(a.stats, a.ordered)
        print(line)
        if a.out:
            open(a.out, "a").write(line + "\n")
        return
    ctx = sga.Context(0)
    if a.profile:
        clouds = profile_clouds(ctx)
        ctx.set_stream_ordered(a.ordered)
        Ts = [yaw_pose(k) for k in range(PROFILE_MEMBERS)]
        for _ in range(10):
            keep = sga.merge_clouds(clouds, Ts, origin=np.zeros(3), ctx=ctx)
        ctx.synchronize()
        print("profiled 10 merges of %d x %d points (%d)" % (PROFILE_MEMBERS, PROFILE_POINTS, keep.size()))
        return

    # ---- (a)
    K, k_nn = 10, 10
    clouds, Ts = [], []
    T0 = None
    for f in range(K):
        pts, Tws = sga.synthetic.kitti_like_scan(f)
        T0 = Tws if T0 is None else T0
        down = sga.voxelgrid_sampling(sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32), ctx=ctx), 0.25)
        sga.estimate_covariances(down, None, k_nn)
        clouds.append(down)
        Ts.append(np.linalg.inv(T0) @ Tws)
    origin = np.zeros(3)
    lib = sga.load()

    def merge():
        return sga.merge_clouds(clouds, Ts, origin=origin, ctx=ctx)

    def host():
        parts = []
        for c, T in zip(clouds, Ts):
            n = c.size()
            xyz, c6 = np.empty((n, 3), np.float64), np.empty((n, 6), np.float32)
            api.check(lib.sga_cloud_download_f64(ctx.h, c.h, api._dp(xyz), None, api._fp(c6)))  # (the covariances come along, as the route demands, and cannot be used)
            parts.append(xyz @ T[:3, :3].T + T[:3, 3])
        joined = np.ones((sum(len(p) for p in parts), 4))
        joined[:, :3] = np.concatenate(parts)
        h = api.C.c_void_p()
        api.check(lib.sga_cloud_create_f64_origin(ctx.h, api._dp(joined), None, None, len(joined), api._dp(origin), api.C.byref(h)))
        out = sga.PointCloud(ctx=ctx, _handle=h)
        sga.estimate_covariances(out, None, k_nn)
        return out

    def region(fn):
        t0 = time.perf_counter()
        keep = fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        del keep
        return dt

    settings = [("merge", merge), ("host", host)]
    for _, fn in settings:
        region(fn)
        region(fn)
    t = {name: [] for name, _ in settings}
    for _ in range(a.reps):
        for name, fn in settings:
            t[name].append(region(fn))
    total = sum(c.size() for c in clouds)
    lines = ["# scripts/cloud_merge_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a blocking context, a region ends synchronised" % a.reps,
             "# (a) %d downsampled C5 scans with covariances (%d points in all) joined at their poses: merge = merge_clouds; host = download_f64 + covariances, numpy transform, create_f64_origin, covariances estimated again (k = %d)" % (K, total, k_nn)]
    cells, lo, hi = [], {}, {}
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        lo[name], hi[name] = float(v.min()), float(v.max())
        cells.append("%10.1f (%8.1f .. %8.1f)" % (float(np.median(v)), lo[name], hi[name]))
    lines.append("%32s  %32s  %s" % ("merge", "host", "merge max < host min"))
    lines.append("%32s  %32s  %s" % (cells[0], cells[1], "yes" if hi["merge"] < lo["host"] else "no"))
    # ---- (c)
    if a.frames:
        del clouds
        sub = odometry.run_synthetic_submap(a.frames, window=5)
        s2s = odometry.run_synthetic(a.frames)
        lines.append("# (c) the drivers over %d synthetic frames, same run: registration ms per scan (preprocessing of the scan + registration), iterations, error" % a.frames)
        lines.append("run_synthetic_submap(window=5)   registration %.3f ms/scan  mean iterations %.2f  ate_trans_m_max %.4f  (submap of %d points)" % (sub["registration_ms_per_scan"], sub["mean_iterations"], sub["ate_trans_m_max"], sub["num_points"]))
        lines.append("run_synthetic (scan to scan)     registration %.3f ms/scan  mean iterations %.2f  rpe_trans_m_mean %.4f" % (s2s["registration_ms_per_scan"], s2s["mean_iterations"], s2s["rpe_trans_m_mean"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

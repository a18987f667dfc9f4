#!/usr/bin/env python3
"""Wall time of the plane segmentation on the device beside the host route, in the same process and build (the
protocol of scripts/cluster_rate.py).

Two clouds from synthetic.kitti_like_scan(0): the raw sweep ("raw", 114k points) and its 0.25 m voxel grid ("down"); threshold 0.1 m,
axis +z within 15 degrees, as odometry.run_synthetic_ground calls it.
      plane H             PointCloud.segment_plane(iterations=H), H = 100 / 1000 / 10000        five commands, two waits
      plane H rest        ... keep="rest", return_kept                                          seven commands, two waits
      plane H no refit    ... refit=False                                                       four commands, one wait
      host route H        the cloud downloaded, the scores of tests/plane_ref.py's numpy restatement (hypotheses + the chunked H x N
                          product), the best plane's inlier flags uploaded as a device array — `--host-reps` regions, H = 100 and 1000
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.  "faster" is claimed only where the device call's slowest
    region lies below the host route's fastest.

  python scripts/plane_rate.py [--reps 9] [--host-reps 3] [--out profiles/cloud_plane_rate.txt]
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/plane_rate.py --reps 3 --host-reps 0     (the kernel trace: a run of its own)

With --kernel-trace <csv> (the trace's kernel_trace file, one row per dispatch) the score kernel's time per setting — the dispatches
are told apart by their grid, ceil(N / 1024) x ceil(H / 32) workgroups — is written beside N x H point-plane tests at the part's fp64
vector rate: a test is 3 subtractions, 1 product, 2 fused multiply-adds and 1 comparison = 7 fp64 vector instructions per point, and
the rate is 256 CUs x 4 SIMDs x 16 fp64 lanes per clock x 2.4 GHz = 39.3e12 lane-instructions per second (78.6 TFLOPS
counts a fused multiply-add as two)."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import synthetic  # noqa: E402

THRESHOLD, AXIS, ANGLE = 0.1, (0.0, 0.0, 1.0), float(np.radians(15.0))
FP64_LANE_RATE = 256 * 4 * 16 * 2.4e9
OPS_PER_TEST = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    ctx = sga.Context()
    pts, _ = synthetic.kitti_like_scan(0)
    raw = sga.PointCloud(pts, ctx=ctx)
    down = sga.voxelgrid_sampling(raw, 0.25)
    lines = ["# scripts/plane_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps]

    def region(fn):
        t0 = time.perf_counter()
        keep = fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        del keep
        return dt

    sizes = {}
    for name, cloud in (("raw", raw), ("down", down)):
        sizes[name] = cloud.size()
        first = cloud.segment_plane(THRESHOLD, 1000, axis=AXIS, max_angle=ANGLE)
        host_parts = {}

        def host_route(H):
            import plane_ref

            t0 = time.perf_counter()
            p = cloud.xyz()
            t1 = time.perf_counter()
            hyp = plane_ref.hypotheses(p, H, 0, AXIS, ANGLE)
            scores, _ = plane_ref.score(p.astype(np.float64), hyp, THRESHOLD)
            best = int(np.argmax(np.where(hyp["valid"], scores.astype(np.int64), -1)))
            dist, _ = plane_ref.distances(p.astype(np.float64), hyp["nhat"][best][None], hyp["a"][best][None])
            flags = (np.abs(dist[0]) <= THRESHOLD).astype(np.float32)
            t2 = time.perf_counter()
            up = sga.PointCloud(np.stack([flags] * 3, 1), ctx=ctx)  # the flags' way back: n x 12 bytes, three times what they need
            t3 = time.perf_counter()
            host_parts[H] = (t1 - t0, t2 - t1, t3 - t2)
            return up

        settings = []
        for H in (100, 1000, 10000):
            settings.append(("plane %d" % H, lambda H=H: cloud.segment_plane(THRESHOLD, H, axis=AXIS, max_angle=ANGLE)))
            settings.append(("plane %d rest" % H, lambda H=H: cloud.segment_plane(THRESHOLD, H, axis=AXIS, max_angle=ANGLE, keep="rest", return_kept=True)))
            settings.append(("plane %d no refit" % H, lambda H=H: cloud.segment_plane(THRESHOLD, H, axis=AXIS, max_angle=ANGLE, refit=False)))
        for _, fn in settings:
            region(fn)
            region(fn)
        t = {label: [] for label, _ in settings}
        for _ in range(a.reps):
            for label, fn in settings:
                t[label].append(region(fn))
        lines.append("# %s: %d points, threshold %.2f m, axis +z within 15 degrees; 1000 hypotheses: %d scored, best %d with %d inliers, %d after the refit, plane (%.5f %.5f %.5f %.5f)" % (
            name, cloud.size(), THRESHOLD, first["scored"], first["best_hypothesis"], first["hypothesis_inliers"], first["inliers"], *first["plane"]))
        for label, _ in settings:
            v = 1e6 * np.array(t[label])
            lines.append("%-5s %-22s %12.1f (%10.1f .. %10.1f)" % (name, label, float(np.median(v)), float(v.min()), float(v.max())))
        for H in (100, 1000):
            host = [region(lambda: host_route(H)) for _ in range(a.host_reps)]
            if not host:
                lines.append("%-5s host route %-11d not measured in this run" % (name, H))
                continue
            v = 1e6 * np.array(host)
            lines.append("%-5s %-22s %12.1f (%10.1f .. %10.1f)   %d region(s); download %.1f ms, hypotheses and scores %.1f ms, upload %.1f ms in the last" % (
                name, "host route %d" % H, float(np.median(v)), float(v.min()), float(v.max()), len(host), *(1e3 * np.array(host_parts[H]))))
            slowest = max(t["plane %d rest" % H])
            lines.append("%-5s host route %d, fastest region / plane %d rest, slowest region: %.1f x%s" % (name, H, H, min(host) / slowest, "" if min(host) > slowest else "   (NOT faster)"))
    lines.append("# the score kernel beside its bound: N x H tests x %d fp64 lane-instructions at %.1fe12 per second; kernel: median (min .. max) of the trace's dispatches [us]" % (OPS_PER_TEST, FP64_LANE_RATE / 1e12))
    seen = {}
    if a.kernel_trace:
        for row in csv.DictReader(open(a.kernel_trace)):
            if "plane_score_kernel" in row.get("Kernel_Name", ""):
                grid = (int(row["Grid_Size_X"]) // int(row["Workgroup_Size_X"]), int(row["Grid_Size_Y"]) // int(row["Workgroup_Size_Y"]))
                seen.setdefault(grid, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for name in ("raw", "down"):
        for H in (100, 1000, 10000):
            v = seen.get(((sizes[name] + 1023) // 1024, (H + 31) // 32))
            kernel = "%10.2f (%10.2f .. %10.2f), %d dispatches" % (float(np.median(v)), min(v), max(v), len(v)) if v else "not traced in this run"
            lines.append("#   %-5s H %-6d bound %10.2f us   kernel %s" % (name, H, 1e6 * sizes[name] * H * OPS_PER_TEST / FP64_LANE_RATE, kernel))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

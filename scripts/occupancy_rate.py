#!/usr/bin/env python3
"""Wall time of the occupancy grid on the device (OccupancyGrid: sga_occupancy_*), in one process and build (the
protocol of scripts/cloud_visibility_rate.py).

The scan is synthetic.kitti_like_scan(3) through synthetic.with_moving_sphere, raw (about 123k returns), on the device already, at the
generator's pose; the grid covers 100 m x 100 m x 8 m around the sensor, ranges 1 .. 50 m.  Per leaf (0.2 m and 0.5 m):
      integrate            grid.integrate(scan, T)             the endpoints and the walk: two launches, no host wait
      endpoints only       grid.integrate(scan, T, mode=1)     one launch: what the traversal costs is the difference
      classify             grid.classify(keyframe, T, keep=("unknown", "occupied"))   the 0.25 m voxel grid of the scan (about 12k points)
                           against the grid: one launch, the compaction, one wait (the cleaner of a keyframe)
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/occupancy_rate.py [--reps 9] [--out profiles/occupancy_rate.txt]
  rocprofv3 --kernel-trace --stats ... -- python scripts/occupancy_rate.py --profile --leaves 0.2     (the kernels' own times: 20 calls per setting)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

LEAVES = (0.2, 0.5)
EXTENT, OFFSET = (100.0, 100.0, 8.0), (-50.13, -49.87, -3.31)
MIN_RANGE, MAX_RANGE, RES = 1.0, 50.0, 0.25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leaves", default=",".join("%g" % v for v in LEAVES), help="the leaves of the grids, comma-separated")
    ap.add_argument("--profile", action="store_true", help="20 calls of every setting and nothing else: for a run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    leaves = tuple(float(v) for v in a.leaves.split(","))
    ctx = sga.Context(0)
    pts, Tws = sga.synthetic.kitti_like_scan(3)
    pts, _ = sga.synthetic.with_moving_sphere(pts, Tws, sga.synthetic.mover_centre(3))
    scan = sga.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32), ctx=ctx)
    keyframe = api.voxelgrid_sampling(scan, RES)
    settings, notes = [], []
    for leaf in leaves:
        dims = [int(np.ceil(e / leaf)) for e in EXTENT]
        grid = sga.OccupancyGrid(Tws[:3, 3] + np.array(OFFSET), leaf, dims, ctx=ctx)
        st = grid.integrate(scan, Tws, MIN_RANGE, MAX_RANGE, return_stats=True)
        counts = grid.classify(keyframe, Tws)
        notes.append("leaf %g: %d x %d x %d cells (%.0f MB); a scan of %d returns: %d ignored, %d hits, %d truncated, %d cells hit, %d cells freed; the keyframe's %d points: %d unknown, %d free, %d occupied"
                     % (leaf, dims[0], dims[1], dims[2], 8e-6 * grid.cells, st["beams"], st["ignored"], st["hits"], st["truncated"], st["cells_hit"], st["cells_freed"], counts["total"], counts["unknown"], counts["free"],
                        counts["occupied"]))
        tag = "leaf %g " % leaf
        settings += [(tag + "integrate", lambda grid=grid: grid.integrate(scan, Tws, MIN_RANGE, MAX_RANGE)), (tag + "endpoints only", lambda grid=grid: grid.integrate(scan, Tws, MIN_RANGE, MAX_RANGE, mode=1)),
                     (tag + "classify", lambda grid=grid: grid.classify(keyframe, Tws, keep=("unknown", "occupied")))]
    if a.profile:
        for _, fn in settings:
            for _ in range(20):
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
    lines = ["# scripts/occupancy_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# OccupancyGrid over %g m x %g m x %g m around the sensor, ranges %g .. %g m: integrate (endpoints + walk), endpoints only (mode 1), classify of the %g m keyframe with the cloud of the unknown"
             % (EXTENT[0], EXTENT[1], EXTENT[2], MIN_RANGE, MAX_RANGE, RES), "#     and occupied points"]
    lines += ["# " + s for s in notes]
    med = {}
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        med[name] = float(np.median(v))
        lines.append("%-26s %10.1f (%8.1f .. %8.1f)" % (name, med[name], float(v.min()), float(v.max())))
    for leaf in leaves:
        tag = "leaf %g " % leaf
        lines.append("leaf %g: the traversal over the endpoints alone: %.1f us (median integrate - median endpoints only)" % (leaf, med[tag + "integrate"] - med[tag + "endpoints only"]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

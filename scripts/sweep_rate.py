#!/usr/bin/env python3
"""Wall time of sweep registration on the device (api.linearize_sweep / api.align_sweep: sga_sweep_linearize / sga_align_sweep; DESIGN.md
section 3.30) beside the route the library had before for the same job — deskew with a known twist, then register rigidly — in the same
process and build (the protocol of scripts/cloud_overlap_rate.py).

The target is synthetic.kitti_like_scan(2) through the 0.25 m voxel grid with its KdTree and covariances (k = 20): the previous scan of an
odometry loop.  The source is the RAW sweep synthetic.kitti_like_sweep(3) (about 121k points, covariances with k = 20, no voxel grid:
it cannot carry times) and an even sample of about 12k points of it.  GICP, max_correspondence_distance = 1 m.  Per source:
      linearize      api.linearize_sweep at the identity and a zero twist             one pass: two launches, one wait
      align          api.align_sweep from the identity and a zero twist               the whole loop
      deskew+align   source.deskewed(times, the PREVIOUS motion's twist), Problem, align from the identity
                                                                                      the earlier route: a twist it has to be given
      overlap        source.overlap(tree, identity, 1 m)                              the same walk without the factor
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.  The two routes do different work (the sweep call estimates
    six more numbers and has no warm pass); no ratio is asked of them.

  python scripts/sweep_rate.py [--reps 9] [--out profiles/sweep_registration_rate.txt]
  python scripts/sweep_rate.py --kernels      five linearizations and five overlaps of the raw sweep and nothing else: for a kernel trace
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

RES, K, SAMPLE = 0.25, 20, 12000


def pose_error(T, T_true):
    E = np.linalg.inv(T_true) @ T
    return float(np.linalg.norm(E[:3, 3])), float(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    ctx = sga.Context(0)
    tgt_pts, T2 = sga.synthetic.kitti_like_scan(2)
    pts, times, T3, xi_true, _ = sga.synthetic.kitti_like_sweep(3)
    _, T1 = sga.synthetic.kitti_like_scan(1)
    xi_prev = api.se3_log(np.linalg.inv(T1) @ T2)  # the previous motion: what an odometry loop would deskew with
    T_true = np.linalg.inv(T2) @ T3
    target = api.voxelgrid_sampling(sga.PointCloud(tgt_pts, ctx=ctx), RES)
    tree = sga.KdTree(target)
    api.estimate_covariances(target, tree, K)
    raw = sga.PointCloud(np.ascontiguousarray(pts, dtype=np.float32), ctx=ctx)
    idx = np.arange(0, raw.size(), max(1, -(-raw.size() // SAMPLE)), dtype=np.int64)
    sources = [("raw", raw, times), ("sample", raw.selected(idx), np.ascontiguousarray(times[idx]))]
    for _, cloud, _ in sources:
        api.estimate_covariances(cloud, None, K)
    setting = api.make_setting("GICP", 1.0)
    if a.kernels:
        for _ in range(5):
            api.linearize_sweep(target, raw, times, tree, setting=setting, return_nearest=False)
            raw.overlap(tree, np.eye(4), 1.0)
        ctx.synchronize()
        return
    settings, notes = [], []
    for label, cloud, t in sources:

        def parent(cloud=cloud, t=t):
            return api.Problem(tree, cloud.deskewed(t, xi_prev, 1.0), np.eye(4), ctx=ctx).align(setting, np.eye(4))

        settings += [
            (label + " linearize", lambda cloud=cloud, t=t: api.linearize_sweep(target, cloud, t, tree, setting=setting, return_nearest=False)),
            (label + " align", lambda cloud=cloud, t=t: api.align_sweep(target, cloud, t, tree, setting=setting)),
            (label + " deskew+align", parent),
            (label + " overlap", lambda cloud=cloud: cloud.overlap(tree, np.eye(4), 1.0)),
        ]
        res, old = api.align_sweep(target, cloud, t, tree, setting=setting), parent()
        notes.append("%s = %d points against %d: align_sweep %d iterations, pose error %.4f m %.5f rad, twist error %.4f m %.5f rad; deskew (previous motion) + align %d iterations, pose error %.4f m %.5f rad"
                     % ((label, cloud.size(), target.size(), res.iterations + 1) + pose_error(res.T_target_source, T_true) + (float(np.linalg.norm(res.twist[3:] - xi_true[3:])), float(np.linalg.norm(res.twist[:3] - xi_true[:3])),
                        old.iterations + 1) + pose_error(old.T_target_source, T_true)))

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
    lines = ["# scripts/sweep_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# target: kitti_like_scan(2) through the %g m voxel grid, KdTree, covariances k = %d; source: the raw kitti_like_sweep(3) and an even sample of it, covariances k = %d; GICP, 1 m" % (RES, K, K),
             "# (on the arc the previous motion IS the sweep's motion: the earlier route is given the right twist here)"]
    lines += ["# " + s for s in notes]
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        lines.append("%-22s %10.1f (%8.1f .. %8.1f)" % (name, float(np.median(v)), float(v.min()), float(v.max())))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

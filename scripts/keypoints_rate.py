#!/usr/bin/env python3
"""Wall time of the ISS keypoints on the device and of global_align with and without them, in one process and
build (the protocol of scripts/plane_rate.py).

Clouds: the target of the terrain pair of tests/test_global_registration_gpu.py (synthetic.bumpy_terrain(60000, 1)) on a 0.5 m and on a
0.25 m voxel grid, and the raw sweep synthetic.kitti_like_scan(0).
      iss (rs, rn)            PointCloud.iss_keypoints(rs, rn, tree=the cloud's tree)                 three commands, one wait
      iss (rs, rn) cloud      ... keep=True                                                          four commands, one wait
      match all / keypoints   match_features over all FPFH rows of the pair / over the keypoints' rows (Features.selected)
      global / + keypoints    global_align(target, source, voxel, refine=True) without / with keypoints=True
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.  "faster" is claimed only where one form's slowest region
    lies below the other's fastest.

  python scripts/keypoints_rate.py [--reps 9] [--out profiles/cloud_keypoints_rate.txt]
  rocprofv3 --kernel-trace -d <dir> -- python scripts/keypoints_rate.py --reps 3 --iss-only          (the kernel trace: a run of its own)
  python scripts/keypoints_rate.py --trace <kernel_trace.csv> [--out <file to append to>]            (no device: the two kernels' times)

The trace's dispatches of iss_saliency_kernel and iss_nms_kernel are told apart by their grid, ceil(n / 64) workgroups of one wave."""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rigid(axis, angle, t):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T


T_TRUE = rigid([0.1, 0.2, 0.97], np.deg2rad(150.0), [12.0, -7.0, 1.5])
ABOVE = (0.0, 0.0, 50.0)


def stats(label, v, lines):
    v = 1e6 * np.array(v)
    lines.append("%-44s %12.1f (%10.1f .. %10.1f)" % (label, float(np.median(v)), float(v.min()), float(v.max())))


def verdict(what, a_label, a, b_label, b, lines):
    if max(a) < min(b):
        lines.append("#   %s: %s is faster (its slowest region %.1f us lies below the other's fastest %.1f us)" % (what, a_label, 1e6 * max(a), 1e6 * min(b)))
    elif max(b) < min(a):
        lines.append("#   %s: %s is faster (its slowest region %.1f us lies below the other's fastest %.1f us)" % (what, b_label, 1e6 * max(b), 1e6 * min(a)))
    else:
        lines.append("#   %s: NO claim either way (the regions overlap: %s %.1f .. %.1f us, %s %.1f .. %.1f us)" % (what, a_label, 1e6 * min(a), 1e6 * max(a), b_label, 1e6 * min(b), 1e6 * max(b)))


def trace_lines(path):
    seen = {}
    for row in csv.DictReader(open(path)):
        name = row.get("Kernel_Name", "")
        for k in ("iss_saliency_kernel", "iss_nms_kernel", "iss_list_kernel", "features_gather_kernel", "feature_match"):
            if k in name:
                groups = int(row["Grid_Size_X"]) // max(1, int(row["Workgroup_Size_X"]))
                seen.setdefault((k, groups), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    lines = ["# kernel times from a kernel trace in a run of its own [us]: median (min .. max), dispatches; told apart by their workgroups"]
    for (k, groups), v in sorted(seen.items()):
        lines.append("#   %-24s %8d workgroups %10.2f (%10.2f .. %10.2f), %d dispatches" % (k, groups, float(np.median(v)), min(v), max(v), len(v)))
    if len(lines) == 1:
        lines.append("#   not measured yet: the trace holds none of the kernels")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--iss-only", action="store_true")
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        text = "\n".join(trace_lines(a.trace))
        print(text)
        if a.out:
            open(a.out, "a").write(text + "\n")
        return
    import small_gicp_amd as sga
    from small_gicp_amd import synthetic

    ctx = sga.default_context()
    target = synthetic.bumpy_terrain(60000, 1)
    Ti = np.linalg.inv(T_TRUE)
    source = np.ascontiguousarray((synthetic.bumpy_terrain(60000, 2).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32))
    lines = ["# scripts/keypoints_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps]

    def region(fn):
        t0 = time.perf_counter()
        keep = fn()
        ctx.synchronize()
        dt = time.perf_counter() - t0
        del keep
        return dt

    def measure(settings):
        for _, fn in settings:
            region(fn)
            region(fn)
        t = {label: [] for label, _ in settings}
        for _ in range(a.reps):
            for label, fn in settings:
                t[label].append(region(fn))
        for label, _ in settings:
            stats(label, t[label], lines)
        return t

    clouds = {}
    for voxel in (0.5, 0.25):
        clouds[voxel] = sga.preprocess_points(target, voxel, 20) + sga.preprocess_points(source, voxel, 20)
    raw = sga.PointCloud(synthetic.kitti_like_scan(0)[0])
    raw_tree = sga.KdTree(raw)
    # ---- the detector alone
    cases = [("terrain 0.5 m", clouds[0.5][0], clouds[0.5][1], (1.5, 0.75)), ("terrain 0.5 m", clouds[0.5][0], clouds[0.5][1], (3.0, 2.0)),
             ("terrain 0.25 m", clouds[0.25][0], clouds[0.25][1], (0.75, 0.375)), ("kitti_like_scan raw", raw, raw_tree, (1.5, 0.75))]
    settings = []
    for name, cloud, tree, (rs, rn) in cases:
        got = cloud.iss_keypoints(rs, rn, tree=tree)
        lines.append("# %s: %d points, radii (%.3f, %.3f): %d keypoints, %d workgroups per walk kernel" % (name, cloud.size(), rs, rn, got["count"], (cloud.size() + 63) // 64))
        settings.append(("%s iss (%.3g, %.3g)" % (name, rs, rn), lambda c=cloud, t=tree, rs=rs, rn=rn: c.iss_keypoints(rs, rn, tree=t)))
        settings.append(("%s iss (%.3g, %.3g) cloud" % (name, rs, rn), lambda c=cloud, t=tree, rs=rs, rn=rn: c.iss_keypoints(rs, rn, tree=t, keep=True)))
    measure(settings)
    if not a.iss_only:
        # ---- the matcher over all rows and over the keypoints' rows; global_align with and without
        for voxel in (0.5, 0.25):
            tgt, ttree, src, stree = clouds[voxel]
            ft, fs = tgt.fpfh(ttree, 20, ABOVE), src.fpfh(stree, 20, ABOVE)
            kt = tgt.iss_keypoints(3.0 * voxel, 1.5 * voxel, tree=ttree)["indices"]
            ks = src.iss_keypoints(3.0 * voxel, 1.5 * voxel, tree=stree)["indices"]
            fts, fss = ft.selected(kt), fs.selected(ks)
            lines.append("# voxel %.2f m: %d / %d points (source / target), %d / %d keypoints, %d mutual pairs over all rows, %d over the keypoints' rows" % (
                voxel, src.size(), tgt.size(), len(ks), len(kt), len(sga.match_features(fs, ft)), len(sga.match_features(fss, fts))))
            t = measure([("voxel %.2f match all rows" % voxel, lambda: sga.match_features(fs, ft)), ("voxel %.2f match keypoint rows" % voxel, lambda: sga.match_features(fss, fts)),
                         ("voxel %.2f select both" % voxel, lambda: (fs.selected(ks), ft.selected(kt)))])
            verdict("matching at %.2f m" % voxel, "keypoint rows", t["voxel %.2f match keypoint rows" % voxel], "all rows", t["voxel %.2f match all rows" % voxel], lines)
            outs = {}

            def align(kp, voxel=voxel):
                outs[kp] = sga.global_align(target, source, voxel, k=20, seed=0, viewpoint=ABOVE, keypoints=kp)
                return outs[kp]

            t = measure([("voxel %.2f global_align" % voxel, lambda: align(None)), ("voxel %.2f global_align + keypoints" % voxel, lambda: align(True))])
            for kp, label in ((None, "without"), (True, "with")):
                c, r = outs[kp]
                dt = np.linalg.norm(c["T"][:3, 3] - T_TRUE[:3, 3])
                dr = np.arccos(np.clip((np.trace(c["T"][:3, :3].T @ T_TRUE[:3, :3]) - 1) / 2, -1, 1))
                lines.append("#   voxel %.2f %s keypoints: %d pairs, %d inliers, coarse error %.3f m %.3f deg, refined in %d iterations" % (voxel, label, len(c["pairs"]), c["inliers"], dt, np.rad2deg(dr), r.iterations))
            verdict("global_align at %.2f m" % voxel, "with keypoints", t["voxel %.2f global_align + keypoints" % voxel], "without", t["voxel %.2f global_align" % voxel], lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

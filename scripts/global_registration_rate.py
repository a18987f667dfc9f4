#!/usr/bin/env python3
"""Wall time of the global registration on the device beside the host route, in the same process and build (the
protocol of scripts/cloud_outliers_rate.py).

The end-to-end case of tests/test_global_registration_gpu.py: synthetic.bumpy_terrain(60000, 1) against bumpy_terrain(60000, 2) moved by
150 degrees and 14 m, voxel 0.5 m (about 8.5k / 8.8k points), k = 20, 20000 hypotheses.  Both clouds are preprocessed once (voxel grid,
trees, normals); then
      fpfh           source.fpfh(tree, 20, viewpoint)                    three launches, one wait
      match          match_features(fs, ft, mutual=True)                 three launches, one wait, the host's compaction of match[]
      compaction     the host's compaction alone, on a stored match[]    what device-resident pair lists would save
      ransac         ransac_correspondences(source, target, pairs, ...)  four commands, one wait, the host's 4x4 eigen-solver
      global_align   the whole chain from the raw arrays, GICP included  (both preprocessings, both descriptors, matching, RANSAC, align)
      host route     the numpy float64 restatement of tests/global_ref.py over the downloaded clouds (brute-force neighbours, FPFH, screened
                     mutual matching, RANSAC over the hypotheses that pass the tests) — `--host-reps` regions (default 1: it takes seconds)
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/global_registration_rate.py [--reps 9] [--host-reps 1] [--out profiles/global_registration_rate.txt]
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/global_registration_rate.py --reps 3 --host-reps 0     (the kernel trace: a run of its own)
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

VOXEL, K, H, ABOVE = 0.5, 20, 20000, (0.0, 0.0, 50.0)


def rigid(axis, angle, t):
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)
    T[:3, 3] = t
    return T


def pose_error(T, T_ref):
    E = np.linalg.inv(T_ref) @ T
    return float(np.linalg.norm(E[:3, 3])), float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(E[:3, :3] - np.eye(3)) / (2.0 * np.sqrt(2.0))))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = sga.default_context()
    T_true = rigid([0.1, 0.2, 0.97], np.deg2rad(150.0), [12.0, -7.0, 1.5])
    target = sga.synthetic.bumpy_terrain(60000, 1)
    Ti = np.linalg.inv(T_true)
    source = np.ascontiguousarray((sga.synthetic.bumpy_terrain(60000, 2).astype(np.float64) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32))
    tgt, ttree = sga.preprocess_points(target, VOXEL, K)
    src, stree = sga.preprocess_points(source, VOXEL, K)
    ft, fs = tgt.fpfh(ttree, K, ABOVE), src.fpfh(stree, K, ABOVE)
    pairs = sga.match_features(fs, ft, mutual=True)
    match = np.full(src.size(), -1, np.int64)
    match[pairs[:, 0]] = pairs[:, 1]
    ransac = dict(max_distance=1.5 * VOXEL, iterations=H, seed=0, min_edge=2.0 * VOXEL)
    coarse = sga.ransac_correspondences(src, tgt, pairs, **ransac)

    def compaction():
        keep = np.nonzero(match >= 0)[0]
        return np.ascontiguousarray(np.stack([keep.astype(np.int64), match[keep]], axis=1))

    def host_route():
        import global_ref as ref

        t0 = time.perf_counter()
        rt, nt = tgt.xyz(), tgt.normals()[:, :3].astype(np.float32)
        rs, ns = src.xyz(), src.normals()[:, :3].astype(np.float32)
        a_, b_ = ref.fpfh(rt, nt, K, ABOVE), ref.fpfh(rs, ns, K, ABOVE)
        t1 = time.perf_counter()
        m = ref.match(b_["rows"].astype(np.float32), a_["rows"].astype(np.float32), True)
        keep = np.flatnonzero(m["match"] >= 0)
        t2 = time.perf_counter()
        r = ref.ransac(rs[keep].astype(np.float64), rt[m["match"][keep]].astype(np.float64), 1.5 * VOXEL, H, 0, 0.9, 2.0 * VOXEL)
        t3 = time.perf_counter()
        host_parts.append((t1 - t0, t2 - t1, t3 - t2))
        return r["best"]

    host_parts = []
    settings = [
        ("fpfh", lambda: src.fpfh(stree, K, ABOVE)),
        ("match", lambda: sga.match_features(fs, ft, mutual=True)),
        ("compaction", compaction),
        ("ransac", lambda: sga.ransac_correspondences(src, tgt, pairs, **ransac)),
        ("global_align", lambda: sga.global_align(target, source, VOXEL, k=K, iterations=H, seed=0, viewpoint=ABOVE)),
    ]

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
    host = [region(host_route) for _ in range(a.host_reps)]
    dt, dr = pose_error(coarse["T"], T_true)
    lines = ["# scripts/global_registration_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# bumpy_terrain(60000, 1) / (60000, 2) at a %.2f m voxel: %d / %d points, k = %d, %d mutual pairs, %d hypotheses of which %d passed the tests; best %d with %d inliers, refit %d," % (
                 VOXEL, tgt.size(), src.size(), K, len(pairs), H, coarse["scored"], coarse["best_hypothesis"], coarse["inliers"], coarse["refit"]),
             "#     coarse pose %.3f m and %.3f degrees from the truth" % (dt, dr)]
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        lines.append("%-14s %12.1f (%10.1f .. %10.1f)" % (name, float(np.median(v)), float(v.min()), float(v.max())))
    if host:
        v = 1e6 * np.array(host)
        lines.append("%-14s %12.1f (%10.1f .. %10.1f)   %d region(s); descriptors of both clouds %.2f s, mutual matching %.2f s, RANSAC %.2f s in the last" % (
            "host route", float(np.median(v)), float(v.min()), float(v.max()), len(host), *host_parts[-1]))
        chain = 2 * np.median(t["fpfh"]) + np.median(t["match"]) + np.median(t["ransac"])
        lines.append("host route / (2 x fpfh + match + ransac) on the device: %.0f x" % (np.median(host) / chain))
    else:
        lines.append("host route     not measured in this run")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

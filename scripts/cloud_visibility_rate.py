#!/usr/bin/env python3
"""Wall time of the free-space check on the device (PointCloud.visibility: sga_cloud_visibility) beside the host route, in the same
process and build (the protocol of scripts/cloud_overlap_rate.py).

The scan is synthetic.kitti_like_scan(3) through synthetic.with_moving_sphere, raw (about 123k returns), on the device already; the map is
scan 0 — also with the sphere, three frames earlier — once through the 0.25 m voxel grid (a keyframe, about 11k points) and once raw.  The
pose is the generator's.  The library's defaults: image 1024 x 64 over [-25, +3] degrees, window 1 x 1, margin 0.2 m + 1 %.  Per map:
      stats          map.visibility(scan, T)                     the fill, the image, the states, the counts: four commands, one wait
      rest           map.visibility(scan, T, keep="rest")        ... and the compaction: table copy, launch, its wait (the cleaned map)
      host route     sga_cloud_download of the map and of the scan (into buffers made once), the rule in numpy float64 (this file's
                     restatement: np.minimum.at for the image, one gather per window cell), sga_cloud_create_f32 of the points that are
                     not seen through
    A region ends with the context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings
    ALTERNATING within a repetition; median and (min .. max) in microseconds.

  python scripts/cloud_visibility_rate.py [--reps 9] [--out profiles/cloud_visibility_rate.txt]
  rocprofv3 --kernel-trace --stats ... -- python scripts/cloud_visibility_rate.py --profile     (the kernels' own times: 20 calls per setting)
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

RES, W, H, WH, WV = 0.25, 1024, 64, 1, 1
FOV_UP, FOV_DOWN, MIN_RANGE, MAX_RANGE, MARGIN, RATIO = 3.0 * np.pi / 180.0, -25.0 * np.pi / 180.0, 0.5, 60.0, 0.2, 0.01


def project(s):
    rho = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        su = (np.arctan2(s[:, 1], s[:, 0]) / (2.0 * np.pi) + 0.5) * W
        sv = (FOV_UP - np.arcsin(s[:, 2] / rho)) / (FOV_UP - FOV_DOWN) * H
    ok = (rho > 0) & np.isfinite(su) & np.isfinite(sv) & (sv >= 0) & (np.floor(sv) < H)
    u = np.where(ok, su, 0.0).astype(np.int64)
    u[u == W] = 0
    return rho, u, np.where(ok, np.floor(sv), 0.0).astype(np.int64), ok


def host_states(map_xyz, scan_xyz, T):
    """the rule of sga_cloud_visibility in numpy float64 -> the state per map point"""
    rho, u, v, ok = project(scan_xyz.astype(np.float64))
    use = ok & (rho >= MIN_RANGE)
    img = np.full(H * W, np.inf)
    np.minimum.at(img, v[use] * W + u[use], rho[use])
    img = img.reshape(H, W)
    w = map_xyz.astype(np.float64) - T[:3, 3]
    rho, u, v, ok = project(w @ T[:3, :3])
    ok &= (rho >= MIN_RANGE) & (rho <= MAX_RANGE)
    m, M = np.full(len(w), np.inf), np.full(len(w), -np.inf)
    for dv in range(-WV, WV + 1):
        vv = v + dv
        row = (vv >= 0) & (vv < H)
        for du in range(-WH, WH + 1):
            c = np.where(row, img[np.clip(vv, 0, H - 1), (u + du) % W], np.inf)
            m = np.minimum(m, c)
            M = np.maximum(M, np.where(np.isfinite(c), c, -np.inf))
    ok &= np.isfinite(m)
    tol = MARGIN + RATIO * rho
    state = np.zeros(len(w), np.uint8)
    state[ok] = 1
    state[ok & (rho - tol > M)] = 2
    state[ok & (rho + tol < m)] = 3
    return state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="20 calls of every device setting and nothing else: for a run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    ctx = sga.Context(0)
    lib = sga.load()
    frames = []
    for f in (0, 3):
        pts, Tws = sga.synthetic.kitti_like_scan(f)
        pts, _ = sga.synthetic.with_moving_sphere(pts, Tws, sga.synthetic.mover_centre(f))
        frames.append((np.ascontiguousarray(pts[:, :3], dtype=np.float32), Tws))
    T = np.linalg.inv(frames[0][1]) @ frames[1][1]
    raw = sga.PointCloud(frames[0][0], ctx=ctx)
    maps = [("down", api.voxelgrid_sampling(raw, RES)), ("raw", raw)]
    scan = sga.PointCloud(frames[1][0], ctx=ctx)
    ns = scan.size()
    settings, notes = [], []
    for label, cloud in maps:
        n = cloud.size()

        xyz, sxyz = np.empty((n, 3), np.float32), np.empty((ns, 3), np.float32)  # (the download buffers of a loop that runs per scan: made once)

        def host_route(cloud=cloud, xyz=xyz, sxyz=sxyz):
            api.check(lib.sga_cloud_download(ctx.h, cloud.h, api._fp(xyz), None, None))
            api.check(lib.sga_cloud_download(ctx.h, scan.h, api._fp(sxyz), None, None))
            state = host_states(xyz, sxyz, T)
            return sga.PointCloud(np.ascontiguousarray(xyz[state != 3]), ctx=ctx), state

        settings += [(label + " stats", lambda cloud=cloud: cloud.visibility(scan, T, ctx=ctx)), (label + " rest", lambda cloud=cloud: cloud.visibility(scan, T, keep="rest", ctx=ctx)),
                     (label + " host route", host_route)]
        st, state = cloud.visibility(scan, T, return_state=True, ctx=ctx)
        host = host_route()[1]
        notes.append("%s = %d map points against a scan of %d returns: unobserved %d, consistent %d, occluded %d, seen through %d; the host route states %d points otherwise"
                     % (label, n, ns, st["unobserved"], st["consistent"], st["occluded"], st["seen_through"], int((host != state).sum())))
    if a.profile:
        for name, fn in settings:
            if not name.endswith("host route"):
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
    lines = ["# scripts/cloud_visibility_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps,
             "# PointCloud.visibility(scan, T): image %d x %d over [%g, %g] degrees, window %d x %d, ranges %g .. %g m, margin %g m + %g of the range; statistics only / with the cloud of the"
             % (W, H, np.rad2deg(FOV_DOWN), np.rad2deg(FOV_UP), WH, WV, MIN_RANGE, MAX_RANGE, MARGIN, RATIO),
             "#     points that are not seen through; the host route (download map and scan, the rule in numpy float64, upload)"]
    lines += ["# " + s for s in notes]
    med, lo, hi = {}, {}, {}
    for name, _ in settings:
        v = 1e6 * np.array(t[name])
        med[name], lo[name], hi[name] = float(np.median(v)), float(v.min()), float(v.max())
        lines.append("%-22s %10.1f (%8.1f .. %8.1f)" % (name, med[name], lo[name], hi[name]))
    for label, _ in maps:
        f, g = label + " rest", label + " host route"
        lines.append("%s: the cleaned map against the host route: median %.4f x; slowest device region below the host's fastest: %s" % (label, med[f] / med[g], "yes" if hi[f] < lo[g] else "no"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

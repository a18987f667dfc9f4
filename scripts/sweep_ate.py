#!/usr/bin/env python3
"""ate_trans_m_max of the scan-to-scan driver over raw sweeps (odometry.run_synthetic(sweeps=True)) with the sweep's twist estimated
(estimate_twist=True: api.align_sweep) and with the previous motion as the twist (the default), on the slalom
— speed and yaw rate change from frame to frame — and on the constant-velocity arc, where the previous motion is the right twist.

  python scripts/sweep_ate.py [--out profiles/sweep_odometry_ate.txt]
  python scripts/sweep_ate.py --sweep-sources [--out ...]   only the full-sensor slalom with the twist estimated, once per sweep_source
                                                            ("sample", "voxelgrid": DESIGN.md section 3.31), APPENDED to --out
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from small_gicp_amd import odometry  # noqa: E402

RUNS = [
    ("slalom, 6 sweeps of 16 x 500 rays", dict(num_frames=6, trajectory="slalom", n_rings=16, n_az=500)),
    ("slalom, 6 sweeps of 32 x 1000 rays", dict(num_frames=6, trajectory="slalom", n_rings=32, n_az=1000)),
    ("slalom, 8 sweeps of 64 x 2030 rays", dict(num_frames=8, trajectory="slalom")),
    ("arc, 8 sweeps of 64 x 2030 rays", dict(num_frames=8)),
]
WAYS = [("previous motion", dict()), ("twist estimated", dict(estimate_twist=True)), ("twist estimated, prior 1e4 I on the previous motion", dict(estimate_twist=True, twist_prior_information=1e4))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--sweep-sources", action="store_true")
    a = ap.parse_args()
    if a.sweep_sources:
        name, kw = RUNS[2]
        lines = ["# scripts/sweep_ate.py --sweep-sources: what of the raw sweep align_sweep registers; total_ms = the whole estimate() per scan (wall, mean)"]
        for src in ("sample", "voxelgrid"):
            r = odometry.run_synthetic(sweeps=True, estimate_twist=True, sweep_source=src, **kw)
            lines.append("%-36s %-52s ate_max %.4f  rpe_mean %.4f  reg_ms %.2f  total_ms %.2f" % (name, "twist estimated, sweep_source=" + src, r["ate_trans_m_max"], r["rpe_trans_m_mean"], r["registration_ms_per_scan"], r["total_ms_per_scan"]))
            print(lines[-1], flush=True)
        if a.out:
            open(a.out, "a").write("\n".join(lines) + "\n")
        return
    lines = ["# scripts/sweep_ate.py: odometry.run_synthetic(sweeps=True, ...): ate_trans_m_max [m], mean relative translation error [m], registration ms per scan (wall, mean)"]
    for name, kw in RUNS:
        for way, extra in WAYS:
            r = odometry.run_synthetic(sweeps=True, **kw, **extra)
            lines.append("%-36s %-52s ate_max %.4f  rpe_mean %.4f  reg_ms %.2f" % (name, way, r["ate_trans_m_max"], r["rpe_trans_m_mean"], r["registration_ms_per_scan"]))
            print(lines[-1], flush=True)
    text = "\n".join(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

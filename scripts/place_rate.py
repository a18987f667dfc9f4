#!/usr/bin/env python3
"""Wall time of the place recognition on the device beside the host route, in the same process and build (the
protocol of scripts/cloud_outliers_rate.py), on a blocking and on a stream-ordered context.

The scan of synthetic.scan_at at frame 40 (about 120k returns) and its 0.5 m voxel grid (about 12k points); databases of N = 256 and
N = 4096 entries at the default 20 x 60: the descriptors of the keyframes 0, 2, .., 78 turned by every shift and thinned at random, so
that the entries differ and a few lie near the query.
      add raw         PlaceDatabase.add(raw scan)                         three commands; no host wait on the stream-ordered context
      add down        PlaceDatabase.add(downsampled scan)
      query 256       PlaceDatabase.query(downsampled revisit, k = 10)    four commands, one wait
      query 4096      the same over 4096 entries
      host route 256  the cloud downloaded and tests/place_ref.py run over the 256 downloaded entries — `--host-reps` regions
    The adds go to a database of their own, filled to 70 entries beforehand so that no region holds a growth.  A region ends with the
    context synchronised.  After a warm-up of every setting, `--reps` timed regions per setting, the settings ALTERNATING within a
    repetition; median and (min .. max) in microseconds.

  python scripts/place_rate.py [--reps 9] [--host-reps 3] [--out profiles/place_recognition_rate.txt]
  rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/place_rate.py --reps 3 --host-reps 0     (the kernel trace: a run of its own)
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
from small_gicp_amd import synthetic  # noqa: E402

K = 10


def entries(n, base, seed=7):
    """n images: the base descriptors turned by all shifts in turn, each with a random tenth of its cells emptied"""
    rng = np.random.default_rng(seed)
    out = np.empty((n,) + base[0].shape, np.float32)
    for i in range(n):
        out[i] = np.roll(base[i % len(base)], -(i // len(base)) % base[0].shape[1], axis=1)
        out[i][rng.uniform(size=out[i].shape) < 0.1] = 0.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    raw = synthetic.scan_at(synthetic._sensor_pose(40))
    Tq = synthetic._sensor_pose(40).copy()
    Tq[:3, 3] += [0.2, -0.1, 0.0]
    Tq[:3, :3] = Tq[:3, :3] @ synthetic._rot([0, 0, 1], np.deg2rad(75.0))
    revisit = synthetic.scan_at(Tq, seed=1040)
    base = None
    lines = ["# scripts/place_rate.py: wall time [us], median (min .. max) of %d timed regions, settings alternating; a region ends synchronised" % a.reps]
    host, host_parts = [], []
    for ordered in (False, True):
        ctx = sga.Context()
        ctx.set_stream_ordered(ordered)
        raw_c, rev_c = sga.PointCloud(raw, ctx=ctx), sga.PointCloud(revisit, ctx=ctx)
        down_c, rev_down = sga.voxelgrid_sampling(raw_c, 0.5), sga.voxelgrid_sampling(rev_c, 0.5)
        if base is None:
            base = [sga.PointCloud(synthetic.scan_at(synthetic._sensor_pose(f), n_az=600), ctx=ctx).scan_context() for f in range(0, 80, 2)]
            base[20] = raw_c.scan_context()
            images = entries(4096, base)
        dbs = {}
        for n in (256, 4096):
            dbs[n] = sga.PlaceDatabase(ctx)
            for i in range(n):
                dbs[n].add_descriptor(images[i])
        adds = sga.PlaceDatabase(ctx)
        for i in range(70):
            adds.add_descriptor(images[i])
        ctx.synchronize()
        first = dbs[256].query(rev_down, k=K)

        def host_route():
            import place_ref as ref

            t0 = time.perf_counter()
            rec = rev_down.xyz()
            stored = dbs[256].descriptors()
            t1 = time.perf_counter()
            q = ref.descriptor(rec)
            t2 = time.perf_counter()
            r = ref.query(q, stored, k=K)
            t3 = time.perf_counter()
            host_parts.append((t1 - t0, t2 - t1, t3 - t2))
            return r["index"]

        settings = [
            ("add raw", lambda: adds.add(raw_c)),
            ("add down", lambda: adds.add(down_c)),
            ("query 256", lambda: dbs[256].query(rev_down, k=K)),
            ("query 4096", lambda: dbs[4096].query(rev_down, k=K)),
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
        if not ordered:
            host = [region(host_route) for _ in range(a.host_reps)]
            lines.append("# scan_at(frame 40): %d returns, %d points at a 0.5 m voxel; the revisit (0.22 m aside, turned 75 degrees): %d points; 20 x 60, k = %d; best of 256: entry %d at shift %d, distance %.3f" % (
                raw_c.size(), down_c.size(), rev_down.size(), K, first["index"][0], first["shift"][0], first["distance"][0]))
        lines.append("# %s context" % ("stream-ordered" if ordered else "blocking"))
        for name, _ in settings:
            v = 1e6 * np.array(t[name])
            lines.append("%-16s %12.1f (%10.1f .. %10.1f)" % (name, float(np.median(v)), float(v.min()), float(v.max())))
        if not ordered:
            query_256 = np.array(t["query 256"])
    if host:
        v = 1e6 * np.array(host)
        lines.append("%-16s %12.1f (%10.1f .. %10.1f)   %d region(s); downloads %.1f ms, descriptor %.1f ms, search %.1f ms in the last" % (
            "host route 256", float(np.median(v)), float(v.min()), float(v.max()), len(host), *(1e3 * np.array(host_parts[-1]))))
        lines.append("host route 256, fastest region / query 256 on the blocking context, slowest region: %.0f x" % (min(host) / query_256.max()))
    else:
        lines.append("host route 256   not measured in this run")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""One sha256 per case over what the voxel-map routines leave behind, from seeded synthetic inputs: two builds of the library hold the
same bits exactly when they print the same lines (run it once per build: SGA_LIB_PATH names the library).

A digest covers, per map: its size and device-frame origin, everything download() returns (Gaussian maps: sga_index_voxelmap_download;
flat maps: sga_flatmap_download_contents) and the nearest-neighbour answers over 1, 7 and 27 search offsets for a query set derived from
the map's own records — the answers show what the hash table holds without depending on its slot layout.

Cases, at the smallest shapes where the kernels can go wrong:
  build_*   one-shot maps, lone and batched (B = 1, 8) from the same clouds, and from_voxels of what was downloaded: 255 / 256 / 257 points,
            127 / 128 / 129 runs, a geo-referenced cloud, negative coordinates, a NaN point, a point beyond +-2^20 voxels, an all-dropped
            and an empty member
  insert_*  three posed rounds into incremental Gaussian maps, lone and batched (B = 1, 8), across a rehash (more than 512 voxels), a
            growth (more than 1024) and an LRU sweep (clear_cycle 2, horizon 1); rotations that are not axis-aligned, a translation
            kilometres away, the block-edge clouds of the builds, NaN / far / all-dropped / empty members
  flat_*    the four kinds of flat maps, two rounds, max_num_points_in_cell 3, min_sq_dist_in_cell 0.01

  python scripts/voxelmap_digest.py [--out file]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import api  # noqa: E402

F32 = np.float32
FLAT_KINDS = [sga.IncrementalVoxelMap, sga.IncrementalVoxelMapNormal, sga.IncrementalVoxelMapCov, sga.IncrementalVoxelMapNormalCov]


def attrs(n, seed):
    """covariances (n, 6: symmetric positive definite) and unit normals (n, 3)"""
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 0.1, (n, 3, 3))
    Cm = A @ A.transpose(0, 2, 1) + 1e-3 * np.eye(3)
    nr = rng.normal(0, 1, (n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    return Cm[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]].astype(F32), nr.astype(F32)


def cloud(points, seed, normals=False, covs=True):
    points = np.ascontiguousarray(points)
    if len(points) == 0:  # an empty cloud that has the attributes
        return cloud(np.ones((4, 3), F32), seed, normals, covs).slice(0, 0)
    c6, nr = attrs(len(points), seed)
    return sga.PointCloud(points, normals=nr if normals else None, covs=c6 if covs else None)


def box(n, seed, lo=(-20, -20, -2), hi=(20, 20, 2)):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F32)


def runs(r, seed, per=3):
    """r voxels at a 1 m leaf (2 m apart, negative coordinates among them), `per` points in each, in shuffled order"""
    rng = np.random.default_rng(seed)
    g = np.arange(-3, 5, dtype=np.float64)
    cells = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)[:r] * 2.0
    p = np.repeat(cells, per, axis=0) + rng.uniform(0.2, 0.8, (r * per, 3))
    return p[rng.permutation(len(p))].astype(F32)


def pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def edge_points():
    """the eight members of the block-edge cases"""
    nan = box(300, 11)
    nan[7] = np.nan
    nan[100, 1] = np.nan
    far = box(300, 12)
    far[5] = [3e6, 0, 0]
    far[299] = [1.0, -2e6, 0.5]
    geo = np.random.default_rng(13).uniform((-30, -30, -3), (30, 30, 3), (257, 3)) + np.array([4.5e5, -7.2e5, 300.0])  # float64: an origin of its own
    return [box(255, 1), box(256, 2), geo, runs(127, 3), runs(128, 4), runs(129, 5), nan, far]


def digest(h, m):
    """the map's size, origin, contents and nearest-neighbour answers into the hash"""
    n = m.size()
    origin = np.zeros(3)
    api.check(sga.load().sga_index_origin(m.h, api._dp(origin)))
    h.update(np.int64(n).tobytes() + origin.tobytes())
    if n == 0:
        return
    flat = isinstance(m, api._FlatVoxelMap)
    parts = m._download(m.contents & api._lib.FLAT_NORMALS, m.contents & api._lib.FLAT_COVS) if flat else m.download()
    for a in parts:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    rec = np.asarray(parts[2] if flat else parts[1], dtype=np.float64)
    rec = rec[np.isfinite(rec).all(axis=1)]
    if len(rec) == 0:
        return
    step = max(1, len(rec) // 96)
    q = rec[::step] + np.random.default_rng(len(rec)).uniform(-0.6, 0.6, (len(rec[::step]), 3))
    for offsets in (1, 7, 27):
        m.set_search_offsets(offsets)
        idx, d2 = m.batch_knn_search(q, 1)
        h.update(idx.tobytes() + d2.tobytes())
    m.set_search_offsets(1)


def case(out, name, maps):
    h = hashlib.sha256()
    for m in maps:
        digest(h, m)
    out.append("%-42s %s  maps %d voxels %d" % (name, h.hexdigest(), len(maps), sum(m.size() for m in maps)))


def build_cases(out):
    members = [cloud(p, 100 + i) for i, p in enumerate(edge_points())]
    gone = cloud(box(64, 20) + F32(2e6), 120)
    empty = cloud(np.zeros((0, 3), F32), 121)
    lone = [sga.GaussianVoxelMap.from_cloud(c, 1.0) for c in members + [gone, empty]]
    case(out, "build_lone", lone)
    case(out, "build_batch_B1", [sga.build_gaussian_voxelmaps([c], 1.0)[0] for c in members])
    case(out, "build_batch_B8", sga.build_gaussian_voxelmaps(members, 1.0))
    case(out, "build_batch_dropped_empty", sga.build_gaussian_voxelmaps([members[6], gone, empty, members[7], members[3], empty, members[2], members[0]], 1.0))
    case(out, "build_batch_leaf_0.3", sga.build_gaussian_voxelmaps(members, 0.3))
    again = []
    for m in lone:
        coords, means, c6, _ = m.download()
        again.append(sga.GaussianVoxelMap.from_voxels(1.0, coords, means, c6))
    case(out, "build_from_voxels", again)


def insert_rounds(B):
    """per round the (cloud, pose) of each of B maps: ~200 voxels, then past 512 (rehash; the sweep of round 2 drops what only round 1
    touched), then past 1024 (growth)"""
    far_t = np.array([3456.7, -2345.6, 12.3])
    rounds = []
    for r, (n, half) in enumerate([(260, 6.0), (700, 12.0), (1500, 20.0)]):
        row = []
        for k in range(B):
            c = cloud(box(n + 17 * k, 1000 + 10 * r + k, (-half, -half, -1), (half, half, 1)), 2000 + 10 * r + k)
            row.append((c, pose(0.2 + 0.01 * k, -0.1, 0.3 + 0.05 * r, far_t * (k % 2) + np.array([25.0 * r, -3.0 * k, 0.4]))))
        rounds.append(row)
    return rounds


def gaussian_maps(B):
    maps = [sga.GaussianVoxelMap(1.0) for _ in range(B)]
    for m in maps:
        m.set_lru(1, 2)
    return maps


def insert_cases(out):
    for B in (1, 8):
        rounds = insert_rounds(B)
        lone, batch = gaussian_maps(B), gaussian_maps(B)
        for r, row in enumerate(rounds):
            for m, (c, T) in zip(lone, row):
                m.insert(c, T)
            sga.insert_batch(batch, [c for c, _ in row], [T for _, T in row])
            case(out, "insert_lone_B%d_round%d" % (B, r + 1), lone)
            case(out, "insert_batch_B%d_round%d" % (B, r + 1), batch)
    # the block-edge members, dropped and empty ones, two rounds under two poses (the geo-referenced member: next to its own origin)
    pts = edge_points()
    members = [cloud(p, 300 + i) for i, p in enumerate(pts)]
    gone = cloud(box(64, 20) + F32(2e6), 320)
    empty = cloud(np.zeros((0, 3), F32), 321)
    T1, T2 = pose(0.1, 0.2, -0.4, [1.5, -2.5, 0.3]), pose(-0.3, 0.05, 0.7, [-4.0, 3.0, -0.6])
    row1 = [(c, T1) for c in members]
    row2 = [(members[1], T2), (gone, T2), (empty, T2), (members[0], T2), (members[5], T2), (members[4], T2), (members[7], T2), (members[6], T2)]
    for name, B in (("B1", 1), ("B8", 8)):
        lone, batch = gaussian_maps(8), gaussian_maps(8)
        for row in (row1, row2):
            for m, (c, T) in zip(lone, row):
                m.insert(c, T)
            for i in range(0, 8, B):
                sga.insert_batch(batch[i : i + B], [c for c, _ in row[i : i + B]], [T for _, T in row[i : i + B]])
        case(out, "insert_edges_lone_%s" % name, lone)
        case(out, "insert_edges_batch_%s" % name, batch)


def flat_cases(out):
    T1, T2 = pose(0.1, 0.2, -0.4, [1.5, -2.5, 0.3]), pose(-0.3, 0.05, 0.7, [3456.7, -2345.6, 12.3])
    p1, p2 = box(900, 31, (-6, -6, -1), (6, 6, 1)), box(1100, 32, (-9, -9, -1), (9, 9, 1))
    p1[3] = np.nan
    p2[10] = [3e6, 0, 0]
    for kind in FLAT_KINDS:
        nrm, cov = bool(kind.CONTENTS & api._lib.FLAT_NORMALS), bool(kind.CONTENTS & api._lib.FLAT_COVS)
        lone, batch = kind(1.0), kind(1.0)
        for m in (lone, batch):
            m.set_setting(0.01, 3)
            m.set_lru(1, 2)
        for r, (p, T) in enumerate(((p1, T1), (p2, T2))):
            c = cloud(p, 400 + r, normals=nrm, covs=cov)
            lone.insert(c, T)
            sga.insert_batch([batch], [c], [T])
        case(out, "flat_%s_lone" % kind.__name__, [lone])
        case(out, "flat_%s_batch" % kind.__name__, [batch])
        got = lone._download(nrm, cov)
        case(out, "flat_%s_from_voxels" % kind.__name__, [kind._from_voxels(1.0, got[0], got[1], got[2], got[3], got[4], 1, None)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    build_cases(out)
    insert_cases(out)
    flat_cases(out)
    text = "\n".join(out)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text + "\n")


if __name__ == "__main__":
    main()

"""sga_cloud_overlap (include/small_gicp_amd.h) restated in numpy float64.  No device and no project code.

For a cloud of fp32 records r_i in the device frame at origin o_c, a pose T (cloud -> target; None: the identity) and a target whose fp32
records live in the device frame at o_t:
    c   = ((R0 o0 + R1 o1) + R2 o2) + t per row (the order the header states, every operation rounded on its own),
    q_i = R r_i + (c - o_t).
kd-tree target: the nearest target record to q_i by brute force, d_i its Euclidean distance.  Voxel maps: the voxel of q_i is
fast_floor((q_i + o_t) / leaf); the voxels at the search offsets are looked up in a dict of the map's contents in the reference's order
(the centre, then +x +y +z -x -y -z, or the 3 x 3 x 3 cube in i, j, k order); a Gaussian voxel offers its mean, a flat voxel its points in
slot order; a strictly smaller distance wins, so the first of equal distances is kept.
Point i is matched iff it has a winner and d_i <= max_distance.  A q_i with a non-finite coordinate is unmatched.  Unmatched points report
d = +inf and nearest = -1.  kept(keep): the indices of the matched (keep "matched") or unmatched (keep "unmatched") points whose RECORD
is finite — the compaction keeps finite records only."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
CAP = 16
LIMIT = 1 << 20
_CUBE = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)]
OFFSETS = {
    1: [(0, 0, 0)],
    7: [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)],
    27: [(0, 0, 0)] + _CUBE,  # (the cube's own centre is a second visit of the first voxel: an equal distance never replaces the first)
}


def frame_offset(T, o_c):
    """c = R o_c + t per row: ((R0 o0 + R1 o1) + R2 o2) + t"""
    return np.array([((T[k, 0] * o_c[0] + T[k, 1] * o_c[1]) + T[k, 2] * o_c[2]) + T[k, 3] for k in range(3)])


def queries(rel, o_c=(0.0, 0.0, 0.0), T=None, o_t=(0.0, 0.0, 0.0)):
    """-> (q (n, 3) float64 in the target's device frame, mag (n,)).  mag_i = sum over the axes k of (sum_j |R_kj r_j| + |c_k - o_k|): the
    magnitudes that enter q_i; an error of eps mag_ik on every axis moves a distance from q_i by at most eps mag_i (the 1-norm bounds the
    2-norm)."""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64).reshape(4, 4)
    R, r = T[:3, :3], np.asarray(rel, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    d = frame_offset(T, np.asarray(o_c, dtype=np.float64)) - np.asarray(o_t, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (R[:, 0] * r[:, 0:1] + R[:, 1] * r[:, 1:2]) + R[:, 2] * r[:, 2:3] + d
        mag = np.abs(R[:, 0] * r[:, 0:1]) + np.abs(R[:, 1] * r[:, 1:2]) + np.abs(R[:, 2] * r[:, 2:3]) + np.abs(d)
    return q, mag.sum(axis=1)


def brute_nearest(q, target, chunk=512):
    """-> (index (n,) int64 or -1, d (n,), runner-up d (n,)): the nearest and second nearest target record by brute force; the first of
    equal distances wins.  Non-finite queries find nothing."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    t = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    n = len(q)
    idx, best, second = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    fin = np.isfinite(q).all(1)
    if len(t) == 0:
        return idx, best, second
    for a in range(0, n, chunk):
        sel = np.nonzero(fin[a : a + chunk])[0] + a
        if len(sel) == 0:
            continue
        dx = t[None, :, 0] - q[sel, None, 0]
        dy = t[None, :, 1] - q[sel, None, 1]
        dz = t[None, :, 2] - q[sel, None, 2]
        d2 = dx * dx + dy * dy + dz * dz
        j = np.argmin(d2, axis=1)  # (the first of equal values)
        rows = np.arange(len(sel))
        idx[sel], best[sel] = j, np.sqrt(d2[rows, j])
        if t.shape[0] > 1:
            d2[rows, j] = np.inf
            second[sel] = np.sqrt(d2.min(axis=1))
    return idx, best, second


def fast_floor(x):
    n = np.trunc(x)
    return (n - (x < n)).astype(np.int64)


def map_nearest(q, coords, leaf, org, offsets, means=None, points=None, counts=None):
    """-> (index (n,) int64, d (n,), runner-up d (n,)).  index: the voxel id (means given: a Gaussian map) or voxel * 16 + slot (points
    (V, 16, 3) and counts (V,) given: a flat map); -1 where nothing is found."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    coords = np.asarray(coords, dtype=np.int64).reshape(-1, 3)
    table = {(int(c[0]), int(c[1]), int(c[2])): v for v, c in enumerate(coords)}
    assert len(table) == len(coords)
    flat = means is None
    rec = np.asarray(points, dtype=np.float64).reshape(-1, CAP, 3) if flat else np.asarray(means, dtype=np.float64).reshape(-1, 1, 3)
    cnt = np.asarray(counts, dtype=np.int64).reshape(-1) if flat else np.ones(len(rec), np.int64)
    n = len(q)
    idx, best, second = np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, np.inf)
    inv = 1.0 / float(leaf)
    org = np.asarray(org, dtype=np.float64)
    for i in range(n):
        if not np.isfinite(q[i]).all():
            continue
        x, y, z = (float(v) for v in q[i])
        c = fast_floor((q[i] + org) * inv)
        b, s2, w = np.inf, np.inf, -1
        for o in OFFSETS[offsets]:
            key = (int(c[0]) + o[0], int(c[1]) + o[1], int(c[2]) + o[2])
            if max(abs(key[0]), abs(key[1]), abs(key[2])) >= LIMIT:
                continue
            v = table.get(key)
            if v is None:
                continue
            for s in range(int(cnt[v])):
                px, py, pz = (float(u) for u in rec[v, s])
                dx, dy, dz = px - x, py - y, pz - z
                d2 = dx * dx + dy * dy + dz * dz
                if d2 < b:
                    b, s2, w = d2, b, (v * CAP + s if flat else v)
                elif d2 < s2:
                    s2 = d2
        idx[i], best[i], second[i] = w, np.sqrt(b), np.sqrt(s2)
    return idx, best, second


def derive(rel, found, max_distance):
    """What sga_cloud_overlap reports, from (index, d, runner-up d) of a search: a dict with d, nearest, matched (bool mask), points,
    n_matched, fitness, rmse, mean_distance, second (the runner-up distance, for the near-tie rule) and raw_d (the winner's distance
    whether it is within max_distance or not, for the band rule)."""
    idx, d, second = found
    rel = np.asarray(rel, dtype=np.float32).reshape(-1, 3)
    n = len(rel)
    matched = (idx >= 0) & (d <= max_distance)
    dm = d[matched]
    m = int(matched.sum())
    return {
        "d": np.where(matched, d, np.inf),
        "nearest": np.where(matched, idx, -1).astype(np.int64),
        "matched": matched,
        "points": n,
        "n_matched": m,
        "fitness": (m / n) if n else 0.0,
        "rmse": float(np.sqrt(np.sum(dm * dm) / m)) if m else 0.0,
        "mean_distance": float(np.sum(dm) / m) if m else 0.0,
        "second": second,
        "raw_d": d,
        "finite": np.isfinite(rel).all(1),
    }


def kept(res, keep):
    """the indices of the output cloud for keep = "matched" | "unmatched": finite records only, ascending"""
    want = res["matched"] if keep == "matched" else ~res["matched"]
    return np.nonzero(want & res["finite"])[0].astype(np.int64)


def restate_kd(rel, target, max_distance, o_c=(0.0, 0.0, 0.0), T=None, o_t=(0.0, 0.0, 0.0)):
    """rel: the cloud's fp32 records; target: the target's fp32 records in ITS device frame, in the order of its original indices"""
    q, mag = queries(rel, o_c, T, o_t)
    res = derive(rel, brute_nearest(q, target), max_distance)
    res["q"], res["mag"] = q, mag
    return res


def restate_map(rel, coords, leaf, offsets, max_distance, o_c=(0.0, 0.0, 0.0), T=None, o_t=(0.0, 0.0, 0.0), means=None, points=None, counts=None):
    q, mag = queries(rel, o_c, T, o_t)
    res = derive(rel, map_nearest(q, coords, leaf, o_t, offsets, means, points, counts), max_distance)
    res["q"], res["mag"] = q, mag
    return res


# ---- the comparison rule for kd-tree targets (tests/test_cloud_overlap_gpu.py) ---------------------------------------------------------------
def kd_bound(res):
    """How far above the restatement's distance the device's may lie: 2 e_i + 1e-6 d_ref + 64 eps64 mag_i, e_i = |q_i - float(q_i)| — the
    walk minimises an fp32 squared distance measured from float(q_i), which differs from the true one by at most e_i plus 3 ulp of fp32 on
    d.  Below the restatement's distance only the 64 eps64 mag_i term is allowed (kd_floor)."""
    q = res["q"]
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.linalg.norm(q - q.astype(np.float32).astype(np.float64), axis=1)
        d = np.where(np.isfinite(res["raw_d"]), res["raw_d"], 0.0)
        return np.nan_to_num(2.0 * e + 1e-6 * d + 64 * EPS64 * res["mag"], nan=0.0, posinf=0.0)


def kd_floor(res):
    return np.nan_to_num(64 * EPS64 * res["mag"], nan=0.0, posinf=0.0)


def band(res, max_distance, bound):
    """the points that may fall either way: |d_ref - max_distance| within the bound"""
    d = res["raw_d"]
    with np.errstate(invalid="ignore"):
        return np.nonzero(np.isfinite(d) & (np.abs(d - max_distance) <= bound))[0]


def near_ties(res, bound):
    """the points whose two nearest target records differ in distance by no more than the bound: either may be reported"""
    with np.errstate(invalid="ignore"):
        return np.nonzero(np.isfinite(res["second"]) & (res["second"] - res["raw_d"] <= bound))[0]

"""The fp64 restatement of sga_cloud_remove_outliers (include/small_gicp_amd.h), in numpy and never through the
library: brute-force distances over the cloud's fp32 records, np.sort, and the definitions as the header states them.

For a cloud of n points the point itself is its own nearest record at distance 0; s_i(j) is the j-th smallest Euclidean distance from
point i to the records of the cloud (s_i(0) = 0).
    statistical (k, std_mul): d_i = (s_i(0) + ... + s_i(k')) / k', k' = min(k, n - 1) (n = 1: d_0 = 0); mean = sum d_i / n;
                              stddev = sqrt(sum (d_i - mean)^2 / (n - 1)), 0 for n < 2; threshold = mean + std_mul stddev; keep d_i <= threshold
    radius (k, radius):       d_i = s_i(k), +inf when n <= k; keep d_i <= radius; threshold = radius, mean / stddev those of the d_i
Also here: the test clouds (two jittered planes and uniform scatter) and the comparison rule's band."""
import numpy as np

F32 = np.float32


def sorted_distances(records, cols):
    """(n, min(cols, n)) float64: row i holds the smallest distances from record i to all records (itself included), ascending.
    records: (n, 3) float32 — the device's records, i.e. relative to the cloud's origin."""
    r = np.asarray(records, dtype=F32).astype(np.float64).reshape(-1, 3)
    n = len(r)
    m = min(cols, n)
    out = np.empty((n, m))
    step = max(1, (1 << 22) // max(n, 1))  # rows per block: ~32 MB of float64 at a time
    for a in range(0, n, step):
        diff = r[a:a + step, None, :] - r[None, :, :]
        d = np.sqrt((diff * diff).sum(axis=2))
        out[a:a + step] = np.sort(d, axis=1)[:, :m]
    return out


def restate(records, k, std_mul=1.0, radius=None):
    """dict(stat (n,), mean, stddev, threshold, kept (int64, ascending)) of the definitions above"""
    r = np.asarray(records, dtype=F32).reshape(-1, 3)
    n = len(r)
    if n == 0:
        return {"stat": np.zeros(0), "mean": 0.0, "stddev": 0.0, "threshold": 0.0, "kept": np.zeros(0, np.int64)}
    s = sorted_distances(r, k + 1)
    if radius is None:
        kp = min(k, n - 1)
        stat = s[:, : kp + 1].sum(axis=1) / kp if kp > 0 else np.zeros(n)
    else:
        stat = s[:, k].copy() if n > k else np.full(n, np.inf)
    with np.errstate(invalid="ignore"):
        mean = float(stat.sum() / n)
        stddev = float(np.sqrt(((stat - mean) ** 2).sum() / (n - 1))) if n >= 2 else 0.0
    threshold = mean + std_mul * stddev if radius is None else float(radius)
    return {"stat": stat, "mean": mean, "stddev": stddev, "threshold": threshold, "kept": np.flatnonzero(stat <= threshold).astype(np.int64)}


BAND = 1e-5  # a point with |d_i - threshold| <= BAND * threshold may fall either way
MAX_BAND_POINTS = 2


def band(ref):
    """indices of the points the comparison rule lets fall either way"""
    t = ref["threshold"]
    if not np.isfinite(t):
        return np.zeros(0, np.int64)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero(np.abs(ref["stat"] - t) <= BAND * t).astype(np.int64)


def planes_with_scatter(seed, n_plane=1450, n_scatter=100, sigma=0.02):
    """Two jittered planes of n_plane points each (z = 0 and x = 0, 10 m x 10 m, sigma of jitter along the normal) plus n_scatter points
    uniform in the 20 m cube around them, shuffled, float32, from a fixed seed: n = 2 n_plane + n_scatter."""
    rng = np.random.default_rng(seed)
    a = np.stack([rng.uniform(-5, 5, n_plane), rng.uniform(-5, 5, n_plane), rng.normal(0.0, sigma, n_plane)], axis=1)
    b = np.stack([rng.normal(0.0, sigma, n_plane) + 5.0, rng.uniform(-5, 5, n_plane), rng.uniform(0, 10, n_plane)], axis=1)
    s = rng.uniform(-10, 10, (n_scatter, 3))
    pts = np.concatenate([a, b, s])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))], dtype=F32)

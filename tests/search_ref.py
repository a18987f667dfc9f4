"""tests/search_ref.py — float64 restatements of the standalone kNN (sga_index_knn / sga_index_knn_f64, csrc/problem.hip: knn_kernel) and of
normal / covariance estimation (sga_estimate_normals_covariances, csrc/preprocess.hip), the yardsticks of tests/test_search_matrix.py.
Pinned to the CPU oracle by tests/test_search_ref.py.

Frames.  An index holds fp32 records p' = fl32(p - origin) in its device frame (common.hpp, "device frames"); the host moves a double
query there as q' = q - origin (in double) and the walk searches from its fp32 rounding fl32(q').  Both helpers take the DEVICE-frame fp32
records and the origin; distances are measured in that frame, where they are the caller's distances for records that fp32 holds exactly
relative to the origin (the test scenes are built that way)."""
import numpy as np
from scipy.spatial import cKDTree

EPS32 = 2.0**-24  # unit roundoff of fp32 (half an ulp at 1)
EPS64 = 2.0**-53
KD_DIST_ULPS = 6  # kd_dist2 = fma(dx, dx, fma(dy, dy, dz * dz)) from fp32 differences: < 6 roundings of relative EPS32


def tie_bound(d2, e):
    """B(q, d): how far apart two squared distances d2 (float64, from the double query) can lie and still be ordered the other way by the
    device's fp32 walk, for a query whose fp32 rounding moved it by e = |q' - fl32(q')| (<= 2^-24 |q'| per axis).

    A record at distance d from q' lies at distance d32 from fl32(q') with |d32^2 - d^2| = |2 (c - q').(q' - q32) + e^2| <= 2 d e + e^2,
    and kd_dist2 rounds d32^2 by at most KD_DIST_ULPS * EPS32 * d32^2 <= 6 EPS32 (d + e)^2.  Two candidates a, b can therefore swap when
    |d2_a - d2_b| <= delta(d_a) + delta(d_b) <= 2 delta(max(d_a, d_b)); the double evaluation adds a few EPS64 (counted as 8 EPS64 d^2)."""
    d2 = np.asarray(d2, dtype=np.float64)
    d = np.sqrt(np.where(np.isfinite(d2), d2, 0.0))
    delta = 2.0 * d * e + e * e + KD_DIST_ULPS * EPS32 * (d + e) ** 2 + 8 * EPS64 * d2
    return 2.0 * delta


def query_rounding(queries64, origin=None):
    """(q' (m, 3) float64 in the device frame, e (m,) = |q' - fl32(q')|): the host's shift and the walk's rounding of each query."""
    q = np.asarray(queries64, dtype=np.float64)[:, :3]
    if origin is not None and np.any(np.asarray(origin) != 0):
        q = q - np.asarray(origin, dtype=np.float64)
    e = np.sqrt(((q - q.astype(np.float32).astype(np.float64)) ** 2).sum(-1))
    return q, e


def knn_ref(points32, queries64, k, max_sq=-1.0, origin=None, e=None, order=True, chunk=1 << 22):
    """Exact kNN in float64 over fp32 records.

    points32: (n, 3) device-frame records; queries64: (m, 3) caller-frame double queries (moved by -origin in double, like the host).
    Kept iff d2 <= max_sq (max_sq < 0: no bound), as the reference's KnnResult does.  Returns (idx (m, k) int64 -1-padded, d2 (m, k)
    float64 +inf-padded, ascending; ties by index), band (m,) bool: the rows whose selection or order the device's fp32 walk may decide
    differently (the k-th and (k+1)-th kept distances, or two returned distances, closer than tie_bound), and e (m,).
    e: the query rounding to assume (default: the actual rounding of q'; pass zeros for a search from fp32-exact queries).
    order=False: the band covers the selection only (a consumer of the set, not of its order)."""
    p = np.asarray(points32, dtype=np.float32).astype(np.float64)
    q, e_act = query_rounding(queries64, origin)
    e = e_act if e is None else np.broadcast_to(np.asarray(e, dtype=np.float64), (len(q),))
    n, m = len(p), len(q)
    kk = min(k + 1, n)
    cand = np.zeros((m, kk), np.int64)
    if n == 0:
        cand = np.zeros((m, 0), np.int64)
    elif n * m <= chunk:
        d2all = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
        cand = np.argsort(d2all, axis=1, kind="stable")[:, :kk]
    else:  # candidates from a kd-tree with a margin, the distances recomputed below
        extra = min(n, kk + 16)
        _, c = cKDTree(p).query(q, k=extra)
        c = np.asarray(c).reshape(m, extra)
        dd = ((q[:, None, :] - p[c]) ** 2).sum(-1)
        cand = np.take_along_axis(c, np.lexsort((c, dd), axis=-1), 1)[:, :kk]  # by (d2, index)
    d2c = ((q[:, None, :] - p[cand]) ** 2).sum(-1) if n else np.zeros((m, 0))
    kept = d2c <= max_sq if max_sq >= 0 else np.ones_like(d2c, dtype=bool)
    idx = np.full((m, k), -1, np.int64)
    d2 = np.full((m, k), np.inf)
    nk = min(k, n)
    idx[:, :nk] = np.where(kept[:, :nk], cand[:, :nk], -1)
    d2[:, :nk] = np.where(kept[:, :nk], d2c[:, :nk], np.inf)
    band = np.zeros(m, bool)
    # the k-th against the (k+1)-th (selection), each against the threshold is exact (double on both sides)
    if kk > k:
        dk, dk1 = d2c[:, k - 1], d2c[:, k]
        band |= (dk1 - dk <= tie_bound(dk1, e)) & (kept[:, k - 1] & (kept[:, k]))
    if order and nk > 1:  # order inside the row (equal distances: the device breaks them by kd position, the reference by its own order)
        gap = np.diff(d2[:, :nk], axis=1)
        fin = np.isfinite(d2[:, 1:nk])
        band |= (fin & (gap <= tie_bound(np.where(fin, d2[:, 1:nk], 0.0), e[:, None]))).any(axis=1)
    return idx, d2, band, e


def features_ref(points32, k, origin=None, gap_min=1e-3):
    """Normals and regularised covariances (util/normal_estimation.hpp) in float64 over fp32 device-frame records.

    Neighbourhoods: knn_ref over the records themselves (the point included, fp32-exact queries).  Fewer than 5 neighbours: normal 0,
    covariance I (normal_estimation.hpp:33-37).  Otherwise the covariance of the neighbourhood, centred two-pass in float64; its
    smallest eigenvector by np.linalg.eigh, turned away from the CALLER's origin (p . n > 0 -> -n, p = record + origin); C = V diag(1e-3,
    1, 1) V^T = I - (1 - 1e-3) n n^T.

    Returns a dict: normals (n, 3), covs (n, 3, 3), found (n,), lam (n, 3) ascending, sep (n,) bool: the spectrum separates the smallest
    eigenvalue ((lam1 - lam0) > gap_min lam2, so the normal is defined to ~cond / gap), band (n,) bool: the k-th and (k+1)-th neighbours near-tied,
    sign_amb (n,) bool: the point lies (to 1e-9) in the plane through the origin normal to n, where the sign is the solver's,
    cov (n, 3, 3) the neighbourhood covariance, dev_err (n,): a bound on how far the device's one-pass sum in its own frame
    (sum x x^T / n - mean mean^T, fp64) can lie from the centred covariance, relative to lam2 — ~8 EPS64 max|p'|^2 / lam2."""
    p32 = np.asarray(points32, dtype=np.float32)
    p = p32.astype(np.float64)
    n = len(p)
    org = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    idx, _, band, _ = knn_ref(p32, p, k, -1.0, e=np.zeros(n), order=False)  # (the search runs in the device frame; the sums ignore the order)
    found = (idx >= 0).sum(1)
    nrm = np.zeros((n, 3))
    covs = np.tile(np.eye(3), (n, 1, 1))
    lam = np.zeros((n, 3))
    cov = np.zeros((n, 3, 3))
    sep = np.zeros(n, bool)
    dev_err = np.zeros(n)
    sign_amb = np.zeros(n, bool)
    ok = found >= 5
    for f in np.unique(found[ok]):
        rows = np.flatnonzero(found == f)
        nb = p[idx[rows, :f]]  # (r, f, 3)
        mu = nb.mean(axis=1)
        c = nb - mu[:, None, :]
        cv = np.einsum("rki,rkj->rij", c, c) / f
        w, v = np.linalg.eigh(cv)
        n0 = v[:, :, 0]
        dp = ((p[rows] + org) * n0).sum(-1)
        n0 = np.where(dp[:, None] > 0, -n0, n0)
        sign_amb[rows] = np.abs(dp) <= 1e-9 * np.linalg.norm(p[rows] + org, axis=1)
        nrm[rows] = n0
        covs[rows] = np.eye(3) - (1.0 - 1e-3) * np.einsum("ri,rj->rij", n0, n0)
        lam[rows] = w
        cov[rows] = cv
        scale = np.maximum(np.abs(w[:, 2]), 1e-300)
        sep[rows] = (w[:, 1] - w[:, 0]) > gap_min * scale
        dev_err[rows] = 8 * EPS64 * (np.abs(nb).max(axis=(1, 2)) ** 2) / scale
    return {"normals": nrm, "covs": covs, "found": found, "lam": lam, "sep": sep, "band": band, "cov": cov, "dev_err": dev_err, "sign_amb": sign_amb}


def compute_direct(cov, point, origin=None):
    """The device's answer where np.linalg.eigh's is not unique: Eigen's computeDirect on the neighbourhood covariance (the oracle's
    restatement, orc.eigen_sym3(m, 0)), its first eigenvector as the normal with the caller-frame sign rule, and C = V diag(1e-3, 1, 1) V^T
    from its three vectors.  (normal (3,), C (3, 3))"""
    from oracle import orc

    _, v = orc.eigen_sym3(np.asarray(cov, dtype=np.float64), 0)
    n0 = v[:, 0] / np.linalg.norm(v[:, 0])
    org = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    if float(np.dot(np.asarray(point, dtype=np.float64) + org, n0)) > 0:
        n0 = -n0
    C = v @ np.diag([1e-3, 1.0, 1.0]) @ v.T
    return n0, C

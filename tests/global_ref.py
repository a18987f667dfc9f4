"""tests/global_ref.py — the definitions of the global registration (include/small_gicp_amd.h: sga_cloud_fpfh, sga_features_match,
sga_ransac_correspondences) restated in numpy float64.  Nothing here goes through the library.

Every restatement also marks its BAND: the points, rows, pairs or hypotheses whose result an ulp of double arithmetic can change, so
that a comparison can be exact everywhere else.
  FPFH      a bin coordinate within 1e-9 of an integer 1 .. 10 (0 and 11 are clamped: both sides give the same bin); | |a1| - |a2| | <
            1e-12 between normals that are neither equal nor opposite (those give |a1| == |a2| exactly: neighbours with the same
            neighbourhood have the same normal, and there are many); |v| < 1e-9; a k'-th / (k' + 1)-th neighbour distance gap below 1e-6 relative (the search orders fp32 squared distances);
            and every point with such a point among its neighbours (its SPFH enters the sum).
  matching  the best and the best DIFFERENT row (rows that are bytewise equal tie exactly: the lowest index wins on the device too)
            within 64 D eps relative; with mutual, also a winner whose reverse search is in the band.
  RANSAC    per hypothesis, the pairs with | |r| - max_distance | < 1e-9; an edge or degeneracy test within 1e-12 (relative to the lengths
            compared) of its limit.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
FPFH_DIM = 33


# ---- neighbours ---------------------------------------------------------------------------------------------------------------------------
def neighbours(records, k, chunk=1024):
    """(idx (n, k') int64: the k' = min(k, n - 1) nearest OTHER records of every fp32 record by brute force, ascending by (squared
    distance in double, index); d2 (n, k'); close (n,) bool: the k'-th and the (k' + 1)-th distance differ by less than 1e-6 relative)."""
    p = np.asarray(records, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = len(p)
    kp = min(int(k), n - 1)
    idx = np.zeros((n, max(kp, 0)), np.int64)
    d2 = np.zeros((n, max(kp, 0)))
    close = np.zeros(n, bool)
    if kp <= 0:
        return idx, d2, close
    for a in range(0, n, chunk):
        q = p[a:a + chunk]
        dx, dy, dz = q[:, None, 0] - p[None, :, 0], q[:, None, 1] - p[None, :, 1], q[:, None, 2] - p[None, :, 2]
        m = dx * dx + dy * dy + dz * dz
        m[np.arange(len(q)), a + np.arange(len(q))] = -1.0  # the record itself sorts first and is dropped
        take = min(kp + 2, n)  # the record itself, its k' neighbours and the next one
        part = np.argpartition(m, take - 1, axis=1)[:, :take] if take < n else np.broadcast_to(np.arange(n), (len(q), n))
        pd = np.take_along_axis(m, part, axis=1)
        order = np.take_along_axis(part, np.lexsort((part, pd), axis=1), axis=1)[:, 1:]  # by distance, then by index
        dd = np.take_along_axis(m, order, axis=1)
        idx[a:a + chunk] = order[:, :kp]
        d2[a:a + chunk] = dd[:, :kp]
        if dd.shape[1] > kp:
            last, nxt = np.sqrt(dd[:, kp - 1]), np.sqrt(dd[:, kp])
            close[a:a + chunk] = (nxt - last) < 1e-6 * nxt
    return idx, d2, close


# ---- FPFH ---------------------------------------------------------------------------------------------------------------------------------
def oriented_normals(points, normals, viewpoint):
    n = np.asarray(normals, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    if viewpoint is None:
        return n
    s = np.einsum("ij,ij->i", n, np.asarray(viewpoint, dtype=np.float64)[None, :] - points)
    return np.where((s < 0.0)[:, None], -n, n)


def pair_features(pi, ni, pj, nj):
    """(counted, theta, alpha, phi, shaky) for the pairs (i, j), every argument (..., 3) float64"""
    d = pj - pi
    ln = np.sqrt(np.einsum("...i,...i->...", d, d))
    ok = ln > 0.0
    safe = np.where(ok, ln, 1.0)
    a1 = np.einsum("...i,...i->...", ni, d) / safe
    a2 = np.einsum("...i,...i->...", nj, d) / safe
    swap = np.abs(a1) < np.abs(a2)
    n1 = np.where(swap[..., None], nj, ni)
    n2 = np.where(swap[..., None], ni, nj)
    d = np.where(swap[..., None], -d, d)
    phi = np.where(swap, -a2, a1)
    v = np.cross(d / safe[..., None], n1)
    vn = np.sqrt(np.einsum("...i,...i->...", v, v))
    counted = ok & (vn > 0.0)
    v = v / np.where(vn > 0.0, vn, 1.0)[..., None]
    w = np.cross(n1, v)
    alpha = np.einsum("...i,...i->...", v, n2)
    theta = np.arctan2(np.einsum("...i,...i->...", w, n2), np.einsum("...i,...i->...", n1, n2))
    # (equal or opposite normals give |a1| == |a2| exactly, in any arithmetic that treats the two alike: no swap, and nothing hangs on an ulp)
    alike = np.all(ni == nj, axis=-1) | np.all(ni == -nj, axis=-1)
    shaky = ok & (((np.abs(np.abs(a1) - np.abs(a2)) < 1e-12) & ~alike) | (vn < 1e-9))
    return counted, theta, alpha, phi, shaky


def bin_coordinates(theta, alpha, phi):
    return 11.0 * (theta + np.pi) / (2.0 * np.pi), 11.0 * (alpha + 1.0) / 2.0, 11.0 * (phi + 1.0) / 2.0


def bins(x):
    return np.clip(np.floor(x), 0, 10).astype(np.int64)


def near_bin_edge(x):
    r = np.round(x)
    return (np.abs(x - r) < 1e-9) & (r >= 1) & (r <= 10)


def fpfh(records, normals, k, viewpoint=None, origin=(0.0, 0.0, 0.0)):
    """{"rows" (n, 33) float64 before the one rounding to fp32, "spfh" (n, 33), "band" (n,) bool, "nbr" (n, k')} of the fp32 records (device
    frame at `origin`) and fp32 normals; viewpoint in the caller's frame, or None."""
    rec = np.asarray(records, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n = len(rec)
    rows, spfh, band = np.zeros((n, FPFH_DIM)), np.zeros((n, FPFH_DIM)), np.zeros(n, bool)
    if n < 2:
        return {"rows": rows, "spfh": spfh, "band": band, "nbr": np.zeros((n, 0), np.int64)}
    nbr, d2, close = neighbours(records, k)
    kp = nbr.shape[1]
    vp = None if viewpoint is None else np.asarray(viewpoint, dtype=np.float64) - np.asarray(origin, dtype=np.float64)
    nrm = oriented_normals(rec, normals, vp)
    pi, ni = rec[:, None, :], nrm[:, None, :]
    counted, theta, alpha, phi, shaky = pair_features(np.broadcast_to(pi, (n, kp, 3)), np.broadcast_to(ni, (n, kp, 3)), rec[nbr], nrm[nbr])
    ct, ca, cp = bin_coordinates(theta, alpha, phi)
    own_band = close | np.any(shaky | (counted & (near_bin_edge(ct) | near_bin_edge(ca) | near_bin_edge(cp))), axis=1)
    pairs = counted.sum(axis=1)
    rows_i = np.repeat(np.arange(n), kp).reshape(n, kp)
    hist = np.zeros((n, FPFH_DIM))
    for off, c in ((0, ct), (11, ca), (22, cp)):
        np.add.at(hist, (rows_i[counted], off + bins(c)[counted]), 1.0)
    spfh = hist * np.where(pairs > 0, 100.0 / np.maximum(pairs, 1), 0.0)[:, None]
    w = np.where(d2 > 0.0, 1.0 / np.where(d2 > 0.0, d2, 1.0), 0.0)
    acc = np.zeros((n, FPFH_DIM))
    for j in range(kp):  # the list's order
        acc += w[:, j, None] * spfh[nbr[:, j]]
    rows = spfh + acc / float(kp)
    for off in (0, 11, 22):
        total = np.zeros(n)
        for t in range(11):
            total += rows[:, off + t]
        rows[:, off:off + 11] *= np.where(total != 0.0, 100.0 / np.where(total != 0.0, total, 1.0), 1.0)[:, None]
    band = own_band | np.any(own_band[nbr], axis=1)
    return {"rows": rows, "spfh": spfh, "band": band, "nbr": nbr}


# ---- matching -----------------------------------------------------------------------------------------------------------------------------
def _exact_d2(q, rows):
    """squared distances of q (c, D) to rows (c, K, D), the bins summed in order"""
    d = np.zeros(rows.shape[:2])
    for b in range(q.shape[1]):
        x = q[:, b, None] - rows[:, :, b]
        d += x * x
    return d


def _judge(d, ids, rowid, tol):
    """winner (the least distance, the lowest index among equals), its distance and the band flag among the candidates ids (c, K)"""
    order = np.lexsort((ids, d), axis=1)  # by distance, then by index
    r = np.arange(len(d))
    j = ids[r, order[:, 0]]
    dj = d[r, order[:, 0]]
    other = np.where(rowid[ids] == rowid[j][:, None], np.inf, d).min(axis=1)
    return j, dj, (dj < np.inf) & np.isfinite(other) & (other - dj <= tol * other)


def _nearest_rows(A, B, chunk=256, screen=None):
    """for every row of A: (winner in B, its squared distance, band flag).  Large problems (screen; default: more than 4096 rows of B) are
    screened first: |a|^2 + |b|^2 - 2 a.b in double picks eight candidates per row, which are then measured by the definition; a row
    whose ninth-best screened value does not clear its winner by a million times the screen's own error is measured against all of B."""
    A = np.asarray(A, dtype=np.float32).astype(np.float64)
    B = np.asarray(B, dtype=np.float32).astype(np.float64)
    n, m, D = len(A), len(B), A.shape[1]
    win, best, band = np.full(n, -1, np.int64), np.full(n, np.inf), np.zeros(n, bool)
    if m == 0 or n == 0:
        return win, best, band
    _, rowid = np.unique(np.asarray(B, dtype=np.float32), axis=0, return_inverse=True)
    rowid = rowid.reshape(-1)
    tol = 64.0 * D * EPS
    screen = (m > 4096) if screen is None else screen
    K = 8
    b2 = np.einsum("ij,ij->i", B, B)
    everyone = np.broadcast_to(np.arange(m), (1, m))
    for a in range(0, n, chunk):
        q = A[a:a + chunk]
        c = len(q)
        full = np.ones(c, bool)
        if screen and m > K + 1:
            approx = np.einsum("ij,ij->i", q, q)[:, None] + b2[None, :] - 2.0 * (q @ B.T)
            part = np.argpartition(approx, K, axis=1)[:, :K + 1]
            vals = np.take_along_axis(approx, part, axis=1)
            ninth = vals.max(axis=1)
            ids = np.sort(np.take_along_axis(part, np.argsort(vals, axis=1)[:, :K], axis=1), axis=1)
            j, dj, bd = _judge(_exact_d2(q, B[ids]), ids, rowid, tol)
            err = 1e-9 * (np.einsum("ij,ij->i", q, q) + b2.max())  # a million times the rounding of the screen
            full = ~(ninth - err > dj * (1.0 + 1e-9) + err)
            win[a:a + chunk], best[a:a + chunk], band[a:a + chunk] = np.where(dj < np.inf, j, -1), dj, bd
        rows = np.flatnonzero(full)
        if len(rows):
            ids = np.broadcast_to(everyone, (len(rows), m))
            j, dj, bd = _judge(_exact_d2(q[rows], np.broadcast_to(B[None], (len(rows), m, D))), ids, rowid, tol)
            win[a + rows], best[a + rows], band[a + rows] = np.where(dj < np.inf, j, -1), dj, bd
    return win, best, band


def match(A, B, mutual):
    """{"match" (n,) int64 (-1: none), "dist" (n,) float64 (+inf for -1), "band" (n,) bool} of the rows of A against the rows of B"""
    win, best, band = _nearest_rows(A, B)
    if mutual and len(B) > 0 and len(A) > 0:
        back, _, back_band = _nearest_rows(B, A)
        has = win >= 0
        j = np.where(has, win, 0)
        band = band | (has & back_band[j])
        win = np.where(has & (back[j] == np.arange(len(win))), win, -1)
    dist = np.where(win >= 0, np.sqrt(best), np.inf)
    return {"match": win, "dist": dist, "band": band}


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def mix64(x):
    z = (int(x) + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw(seed, h, M):
    """the three distinct pair numbers of hypothesis h (plain integers)"""
    u = [mix64(int(seed) ^ mix64(4 * int(h) + j)) for j in range(3)]
    idx = lambda v, R: ((v >> 32) * R) >> 32  # noqa: E731
    i0 = idx(u[0], M)
    i1 = idx(u[1], M - 1)
    i1 += i1 >= i0
    i2 = idx(u[2], M - 2)
    i2 += i2 >= min(i0, i1)
    i2 += i2 >= max(i0, i1)
    return int(i0), int(i1), int(i2)


def _mix64_np(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def draws(seed, hs, M):
    """draw() for an array of hypotheses: (len(hs), 3) int64"""
    hs = np.asarray(hs, dtype=np.uint64)
    seed = np.uint64(int(seed) & _M64)
    with np.errstate(over="ignore"):
        u = [_mix64_np(seed ^ _mix64_np(np.uint64(4) * hs + np.uint64(j))) for j in range(3)]
        idx = lambda v, R: ((v >> np.uint64(32)) * np.uint64(R)) >> np.uint64(32)  # noqa: E731
        i0 = idx(u[0], M).astype(np.int64)
        i1 = idx(u[1], M - 1).astype(np.int64)
        i1 = i1 + (i1 >= i0)
        i2 = idx(u[2], M - 2).astype(np.int64)
        i2 = i2 + (i2 >= np.minimum(i0, i1))
        i2 = i2 + (i2 >= np.maximum(i0, i1))
    return np.stack([i0, i1, i2], axis=1)


def _norm(v):
    return np.sqrt(np.einsum("...i,...i->...", v, v))


def triangle_frames(a, b, c):
    """(F (..., 3, 3) with the columns e1 e2 e3, ok, shaky) of the triangles a b c (..., 3)"""
    ab, ac = b - a, c - a
    lab, lac = _norm(ab), _norm(ac)
    e1 = ab / np.where(lab > 0, lab, 1.0)[..., None]
    nn = np.cross(e1, ac)
    ln = _norm(nn)
    ok = (lab > 0) & (ln > 0) & ~(ln < 1e-9 * lac)
    shaky = np.abs(ln - 1e-9 * lac) < 1e-12 * np.maximum(lac, 1e-300)
    e3 = nn / np.where(ln > 0, ln, 1.0)[..., None]
    e2 = np.cross(e3, e1)
    return np.stack([e1, e2, e3], axis=-1), ok, shaky


def pose_from_triangles(s, t):
    """(R (..., 3, 3), tr (..., 3), ok, shaky): s, t (..., 3 points, 3)"""
    Fs, oks, shs = triangle_frames(s[..., 0, :], s[..., 1, :], s[..., 2, :])
    Ft, okt, sht = triangle_frames(t[..., 0, :], t[..., 1, :], t[..., 2, :])
    R = Ft @ np.swapaxes(Fs, -1, -2)
    cs = ((s[..., 0, :] + s[..., 1, :]) + s[..., 2, :]) / 3.0
    ct = ((t[..., 0, :] + t[..., 1, :]) + t[..., 2, :]) / 3.0
    return R, ct - np.einsum("...ij,...j->...i", R, cs), oks & okt, shs | sht


def ransac(ps, pt, max_distance=1.0, iterations=20000, seed=0, edge_similarity=0.9, min_edge=0.0, chunk=512):
    """Every hypothesis of sga_ransac_correspondences over the M pairs' points ps, pt (M, 3) float64:
    {"valid" (H,) bool, "score" (H,) int64 (0 where not valid), "band" (H,) int64: pairs within 1e-9 of max_distance (of the valid and the shaky hypotheses), "shaky" (H,) bool: an
    edge or degeneracy test at its limit, "R" (H, 3, 3), "t" (H, 3), "triple" (H, 3), "best": the winner or -1}"""
    ps, pt = np.asarray(ps, dtype=np.float64), np.asarray(pt, dtype=np.float64)
    M, H = len(ps), int(iterations)
    out = {"valid": np.zeros(H, bool), "score": np.zeros(H, np.int64), "band": np.zeros(H, np.int64), "shaky": np.zeros(H, bool), "R": np.zeros((H, 3, 3)), "t": np.zeros((H, 3)),
           "triple": np.zeros((H, 3), np.int64), "best": -1}
    if M < 3:
        return out
    for a in range(0, H, chunk):
        hs = np.arange(a, min(a + chunk, H))
        tri = draws(seed, hs, M)
        s, t = ps[tri], pt[tri]  # (h, 3, 3)
        ok, shaky = np.ones(len(hs), bool), np.zeros(len(hs), bool)
        for e in range(3):
            ls, lt = _norm(s[:, (e + 1) % 3] - s[:, e]), _norm(t[:, (e + 1) % 3] - t[:, e])
            lo, hi = np.minimum(ls, lt), np.maximum(ls, lt)
            ok &= (lo >= edge_similarity * hi) & (lo >= min_edge)
            shaky |= (np.abs(lo - edge_similarity * hi) < 1e-12 * np.maximum(hi, 1e-300)) | (np.abs(lo - min_edge) < 1e-12 * np.maximum(hi, 1e-300))
        R, tr, okf, shf = pose_from_triangles(s, t)
        ok &= okf
        shaky |= shf
        out["valid"][hs] = ok
        live = np.flatnonzero(ok | shaky)  # the others score nothing, whatever an ulp does
        if len(live):
            moved = np.matmul(R[live], ps.T[None]) + tr[live][:, :, None] - pt.T[None]  # (h, 3, M)
            r = np.sqrt(moved[:, 0] ** 2 + moved[:, 1] ** 2 + moved[:, 2] ** 2)
            out["score"][hs[live]] = np.where(ok[live], (r <= max_distance).sum(axis=1), 0)
            out["band"][hs[live]] = (np.abs(r - max_distance) < 1e-9).sum(axis=1)
        out["shaky"][hs] = shaky
        out["R"][hs], out["t"][hs], out["triple"][hs] = R, tr, tri
    if out["valid"].any():
        score = np.where(out["valid"], out["score"], -1)
        out["best"] = int(np.argmax(score))  # the first of equal scores: the lowest h
    return out


def kabsch(ps, pt):
    """the least-squares rigid motion pt ~ R ps + t by numpy's SVD: 4x4"""
    ps, pt = np.asarray(ps, dtype=np.float64), np.asarray(pt, dtype=np.float64)
    ms, mt = ps.mean(axis=0), pt.mean(axis=0)
    U, _, Vt = np.linalg.svd((ps - ms).T @ (pt - mt))
    S = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T))])
    T = np.eye(4)
    T[:3, :3] = Vt.T @ S @ U.T
    T[:3, 3] = mt - T[:3, :3] @ ms
    return T


def pose_error(T, T_ref):
    """(translation error in metres, rotation error in radians) of T against T_ref"""
    E = np.linalg.inv(T_ref) @ T
    return float(np.linalg.norm(E[:3, 3])), float(2.0 * np.arcsin(min(1.0, np.linalg.norm(E[:3, :3] - np.eye(3)) / (2.0 * np.sqrt(2.0)))))  # |R - I|_F = 2 sqrt 2 |sin(angle / 2)|

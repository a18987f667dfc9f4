"""The rule of the place recognition (include/small_gicp_amd.h: Scan Context and the shift-aligned search)
restated in numpy float64, with its band.  Nothing here goes through the library.

Descriptor: p = (record + origin) - center in double; a record with a non-finite component is skipped; rho = sqrt(px^2 + py^2), skipped
if rho >= L; ring = min(floor(rho / L * R), R - 1); theta = atan2(py, px), plus 2 pi when negative; sector = min(floor(theta / (2 pi) *
S), S - 1); v = float32(max(pz + height, 0)); D[ring][sector] = the greatest v of the cell, 0 for an empty one.

Distance: n[j] = sqrt(sum_r img[r][j]^2), rings ascending; d(s) = 1 - (1 / count) sum_j (sum_r q[r][j] c[r][(j + s) mod S]) / (n_q[j]
n_c[(j + s) mod S]) over the pairs with both norms > 0, j ascending; count == 0: 1; d = min_s d(s), ties to the lowest s.

Band.  A record is a band point when rho / L * R lies within 1e-9 of an integer in 1 .. R, or theta / (2 pi) * S within 1e-9 of an
integer in 0 .. S, or pz + height within 1e-12 of 0: another correctly working evaluation of sqrt, atan2 or the quotients may put it
into the neighbouring ring or sector, or skip it, or give it the value 0 instead of a value below 1e-12.  A cell is a band cell when a
band point could enter or leave it: every (ring, sector) the point reaches when its two coordinates move by the band's width.  A
decision (the best shift of an entry, the order of two neighbours of the ranking) is in band when the two restated distances it
separates differ by less than 2e-12 (twice the tolerance of a distance)."""
import numpy as np

RING_BAND = 1e-9
SECTOR_BAND = 1e-9
HEIGHT_BAND = 1e-12
DECISION_BAND = 2e-12
DISTANCE_TOL = 1e-12  # R + S + 8 roundings of 2^-53 on terms <= 1 are 4e-14 at (16, 256): 25 x over that


def _polar(records, origin, center, R, S, L, height):
    rec = np.asarray(records, dtype=np.float32).reshape(-1, 3)
    o = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    c = np.zeros(3) if center is None else np.asarray(center, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (rec.astype(np.float64) + o) - c
        fin = np.isfinite(p).all(axis=1)
        p = p[fin]
        rho = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
    near = rho < L
    p, rho = p[near], rho[near]
    t = rho / L * R
    theta = np.arctan2(p[:, 1], p[:, 0])
    theta = np.where(theta < 0.0, theta + 2.0 * np.pi, theta)
    u = theta / (2.0 * np.pi) * S
    h = p[:, 2] + height
    return p, t, u, h, (rho, fin, near)


def descriptor(records, origin=None, center=None, R=20, S=60, L=80.0, height=2.0, return_band=False):
    """records (n, 3) float32: the device's records -> D (R, S) float32 [, band (R, S) bool: the band cells]"""
    p, t, u, h, _ = _polar(records, origin, center, R, S, L, height)
    ring = np.minimum(np.floor(t), R - 1).astype(np.int64)
    sector = np.minimum(np.floor(u), S - 1).astype(np.int64)
    with np.errstate(over="ignore"):
        v = np.where(h > 0.0, h, 0.0).astype(np.float32)
    D = np.zeros((R, S), np.float32)
    np.maximum.at(D, (ring, sector), v)
    if not return_band:
        return D
    return D, band_cells(records, origin, center, R, S, L, height)


def band_cells(records, origin=None, center=None, R=20, S=60, L=80.0, height=2.0):
    """(R, S) bool: the cells a band point could enter or leave.  Points just beyond L (skipped by the rule) count as well."""
    rec = np.asarray(records, dtype=np.float32).reshape(-1, 3)
    o = np.zeros(3) if origin is None else np.asarray(origin, dtype=np.float64)
    c = np.zeros(3) if center is None else np.asarray(center, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        p = (rec.astype(np.float64) + o) - c
        p = p[np.isfinite(p).all(axis=1)]
        rho = np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1])
    t = rho / L * R
    keep = t < R + RING_BAND
    p, t = p[keep], t[keep]
    theta = np.arctan2(p[:, 1], p[:, 0])
    theta = np.where(theta < 0.0, theta + 2.0 * np.pi, theta)
    u = theta / (2.0 * np.pi) * S
    h = p[:, 2] + height
    tn, un = np.rint(t), np.rint(u)
    ring_band = (np.abs(t - tn) <= RING_BAND) & (tn >= 1) & (tn <= R)
    sector_band = (np.abs(u - un) <= SECTOR_BAND) & (un >= 0) & (un <= S)
    height_band = np.abs(h) <= HEIGHT_BAND
    band = np.zeros((R, S), bool)
    for i in np.nonzero(ring_band | sector_band | height_band)[0]:
        rings = {int(np.clip(np.floor(t[i] + e), 0, R - 1)) for e in (-RING_BAND, 0.0, RING_BAND)}
        sectors = set()
        for e in (-SECTOR_BAND, 0.0, SECTOR_BAND):
            f = int(np.floor(u[i] + e))
            sectors.update({int(np.clip(f, 0, S - 1)), f % S})  # (the rule clamps at S; a neighbouring evaluation may wrap to 0)
        for r in rings:
            for s in sectors:
                band[r, s] = True
    return band


def column_norms(img):
    """(S,) float64: sqrt of the sum of squares of a column, rings ascending.  img (R, S) or (N, R, S)"""
    a = np.asarray(img, dtype=np.float32).astype(np.float64)
    s = np.zeros(a.shape[:-2] + a.shape[-1:])
    for r in range(a.shape[-2]):
        s = s + a[..., r, :] * a[..., r, :]
    return np.sqrt(s)


def shift_distances(q, entries):
    """d(s) of the query image q (R, S) against every entry (N, R, S): (N, S) float64"""
    q = np.asarray(q, dtype=np.float32).astype(np.float64)
    e = np.asarray(entries, dtype=np.float32).astype(np.float64)
    if e.ndim == 2:
        e = e[None]
    N, R, S = e.shape
    assert q.shape == (R, S)
    nq, ne = column_norms(q), column_norms(e)  # (S,), (N, S)
    idx = (np.arange(S)[None, :] + np.arange(S)[:, None]) % S  # idx[s][j] = (j + s) mod S
    dot = np.zeros((N, S, S))
    for r in range(R):
        dot = dot + q[r][None, None, :] * e[:, r, :][:, idx]
    ns = ne[:, idx]  # (N, S, S): n_c[(j + s) mod S]
    ok = (nq[None, None, :] > 0.0) & (ns > 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        term = np.where(ok, dot / (nq[None, None, :] * ns), 0.0)
    total = np.zeros((N, S))
    for j in range(S):  # j ascending (a term of 0.0 changes nothing)
        total = total + term[:, :, j]
    count = ok.sum(axis=2)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(count > 0, 1.0 - (1.0 / np.maximum(count, 1)) * total, 1.0)
    return d


def best_shifts(q, entries):
    """per entry: (d (N,), shift (N,) int, in_band (N,) bool: the least and the next d(s) lie closer than DECISION_BAND)"""
    ds = shift_distances(q, entries)
    shift = np.argmin(ds, axis=1)  # (the first of equals: the lowest s)
    d = ds[np.arange(len(ds)), shift]
    if ds.shape[1] > 1:
        rest = ds.copy()
        rest[np.arange(len(ds)), shift] = np.inf
        in_band = rest.min(axis=1) - d < DECISION_BAND
    else:
        in_band = np.zeros(len(ds), bool)
    return d, shift.astype(np.int64), in_band


def query(q, entries, first=0, count=None, k=1):
    """The k best of entries[first : first + count] by ascending (d, index): a dict with index (m,), shift (m,), distance (m,), the
    decisions' band flags — shift_band (m,), order_band (m,): entry t and the next candidate of the ranking (taken or not) lie closer
    than DECISION_BAND — and all_distance / all_shift / all_shift_band over the candidates."""
    entries = np.asarray(entries, dtype=np.float32)
    count = len(entries) - first if count is None else count
    cand = entries[first : first + count]
    if count == 0:
        z = np.zeros(0)
        return {"index": z.astype(np.int64), "shift": z.astype(np.int64), "distance": z, "shift_band": z.astype(bool), "order_band": z.astype(bool), "all_distance": z, "all_shift": z.astype(np.int64),
                "all_shift_band": z.astype(bool)}
    d, shift, sband = best_shifts(q, cand)
    order = np.lexsort((np.arange(count), d))
    m = min(k, count)
    top = order[:m]
    ds = d[order]
    gap = np.full(count, np.inf)
    gap[:-1] = ds[1:] - ds[:-1]
    return {"index": top + first, "shift": shift[top], "distance": d[top], "shift_band": sband[top], "order_band": gap[:m] < DECISION_BAND, "all_distance": d, "all_shift": shift, "all_shift_band": sband}


def distance(q, c):
    """(d, shift) of two images"""
    d, s, _ = best_shifts(q, np.asarray(c)[None])
    return float(d[0]), int(s[0])


def turned(img, shift):
    """The image a sensor turned by shift sectors (yaw = shift 2 pi / S) sees where `img` was seen: its column j is img's column
    (j + shift) mod S, so that distance(turned, img) is 0 at `shift`."""
    return np.roll(np.asarray(img), -int(shift), axis=1)


def expected_shift(yaw, S):
    """round(yaw / (2 pi / S)) mod S"""
    return int(np.rint(yaw / (2.0 * np.pi / S))) % S

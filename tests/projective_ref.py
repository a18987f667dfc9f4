"""Test helper: the reference's ProjectiveSearch restated in numpy (ann/projective_search.hpp), over the fp32 records the device holds.

  projection  :13-27    |p|^2 < 1e-3 -> (0.5, 0.5); otherwise b = p / |p|, lat = -asin(b.y), lon = atan2(b.x, b.z),
                        uv = (lon / 2 pi + 0.5, lat / pi + 0.5).  y is vertical, z points forward (a camera convention)
  pixel       :56-58    u = int(uv.x W), v = int(uv.y H), truncated toward zero
  build       :49-62    every pixel invalid (0xFFFFFFFF); points in index order, a pixel out of range is skipped (u == W), a later
                        point overwrites an earlier one: the highest index owns a pixel.  Non-finite points: skipped (undefined there)
  borders     :30-39    BorderRepeat wraps once (x < 0 -> x + W, x >= W -> x - W); BorderClamp returns x unchanged, so an out-of-range
                        row or column is skipped
  search      :107-140  du = -h..h outer, dv = -v..v inner; every valid pixel is pushed into KnnResult (knn_result.hpp:80-100): only if
                        d < worst (strict), inserted behind the entries it does not beat — i.e. the k smallest by (distance, scan
                        position); a column visited twice (W < 2 h + 1) pushes its points twice

Arithmetic as the device does it: the projection in float64 on (record + origin) — the records are fl32(p - origin) — with
|p|^2 = (x^2 + y^2) + z^2; squared distances (pt - q) in the pair arithmetic (float64 or float32) as (dx^2 + dy^2) + dz^2 on the
device-frame query.  libm's asin / atan2 may differ from the device's by an ulp: a projection whose u W or v H lies within AMBIG of an
integer is flagged AMBIGUOUS, and tests leave such points out of exact comparisons (and check that they are rare).
"""
import numpy as np

INVALID = 0xFFFFFFFF
AMBIG = 1e-9
_CHUNK = 1 << 14  # queries per block of the (queries x window) arrays


def caller_frame(rec, origin):
    """Device-frame records (float64) + origin as the device adds it: a zero origin leaves a coordinate as it is (keeps -0.0)."""
    o = np.asarray(origin, dtype=np.float64)
    return np.where(o == 0.0, rec, rec + o)


def project(p):
    """EquirectangularProjection of every row of p (float64, caller's frame): (pu, pv) float64 and a finite mask."""
    p = np.asarray(p, dtype=np.float64)
    finite = np.isfinite(p).all(1)
    x, y, z = (np.where(finite, p[:, a], 0.0) for a in range(3))
    n2 = (x * x + y * y) + z * z
    near = n2 < 1e-3
    nrm = np.sqrt(np.where(near, 1.0, n2))
    with np.errstate(invalid="ignore"):
        lat = -np.arcsin(y / nrm)
        lon = np.arctan2(x / nrm, z / nrm)
    pu = np.where(near, 0.5, lon / (2.0 * np.pi) + 0.5)
    pv = np.where(near, 0.5, lat / np.pi + 0.5)
    finite &= np.isfinite(pu) & np.isfinite(pv)  # |y| / |p| rounded past 1: NaN, not projected (the device's rule)
    pu, pv = np.where(finite, pu, 0.0), np.where(finite, pv, 0.0)
    return pu, pv, finite


def pixel(p, W, H):
    """(u, v, finite, ambiguous) of every row of p: the reference's int truncation; ambiguous = u W or v H within AMBIG of an integer,
    unless the angle is exact on every platform: asin(0) = 0, atan2(x, 0) = +-pi/2, atan2(0, z) = 0 or +-pi (a coordinate 0, or below
    1e-9 of the range: the angle then rounds to the same double everywhere), and the (0.5, 0.5) of a point near the origin."""
    pu, pv, finite = project(p)
    p = np.where(np.isfinite(p), p, 1.0)
    su, sv = pu * W, pv * H
    u = np.trunc(su).astype(np.int64)
    v = np.trunc(sv).astype(np.int64)
    near = ((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) < 1e-3
    ax, ay, az = np.abs(p[:, 0]), np.abs(p[:, 1]), np.abs(p[:, 2])
    tiny = 1e-9 * np.sqrt(ax * ax + ay * ay + az * az)  # asin(t) = t, atan2(t, z) = 0 or +-pi, atan2(x, t) = +-pi/2 to the last bit
    exact_u = near | (ax <= tiny) | (az <= tiny)
    exact_v = near | (ay <= tiny)
    amb = finite & (((np.abs(su - np.round(su)) < AMBIG) & ~exact_u) | ((np.abs(sv - np.round(sv)) < AMBIG) & ~exact_v))
    return u, v, finite, amb


def build(records, origin, W, H):
    """index_map (H, W) uint32 of the records (n, 3) fp32 device frame + origin (3,), and the ambiguous points' mask."""
    rec = np.asarray(records, dtype=np.float32).astype(np.float64)[:, :3]
    u, v, finite, amb = pixel(caller_frame(rec, origin), W, H)
    ok = finite & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    img = np.full(W * H, -1, dtype=np.int64)
    idx = np.flatnonzero(ok)
    np.maximum.at(img, v[idx] * W + u[idx], idx)  # the highest index wins
    out = np.where(img < 0, INVALID, img).astype(np.uint32).reshape(H, W)
    return out, amb


def ambiguous_pixels(records, origin, W, H):
    """Pixels an ambiguous point may land in on the device (its pixel and the neighbours across the near boundary): (H, W) bool."""
    rec = np.asarray(records, dtype=np.float32).astype(np.float64)[:, :3]
    u, v, _, amb = pixel(caller_frame(rec, origin), W, H)
    mask = np.zeros((H, W), bool)
    for du in (-1, 0, 1):
        for dv in (-1, 0, 1):
            uu, vv = u[amb] + du, v[amb] + dv
            ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
            mask[vv[ok], uu[ok]] = True
    return mask


def window(u, v, W, H, wh, wv, repeat_h=True, repeat_v=False):
    """Flat pixel numbers v * W + u of every query's window in scan order (m, (2 wh + 1)(2 wv + 1)); -1 where the pixel is skipped."""
    du = np.repeat(np.arange(-wh, wh + 1), 2 * wv + 1)
    dv = np.tile(np.arange(-wv, wv + 1), 2 * wh + 1)
    uu = u[:, None] + du[None]
    vv = v[:, None] + dv[None]
    if repeat_h:
        uu = np.where(uu < 0, uu + W, np.where(uu >= W, uu - W, uu))
    if repeat_v:
        vv = np.where(vv < 0, vv + H, np.where(vv >= H, vv - H, vv))
    ok = (uu >= 0) & (uu < W) & (vv >= 0) & (vv < H)
    return np.where(ok, vv * W + uu, -1)


def knn(index_map, records, origin, queries_dev, k, wh=10, wv=5, repeat_h=True, repeat_v=False, dtype=np.float64, max_sq=None):
    """The k-NN of every device-frame query (m, 3): (idx (m, k) int64, d2 (m, k) dtype, ambiguous (m,) bool); -1 / inf = none.
    max_sq: the filter of sga_index_knn (reject iff d2 > max_sq).  dtype: the pair arithmetic (float64, or float32 for fp32 passes)."""
    H, W = index_map.shape
    img = index_map.reshape(-1).astype(np.int64)
    img = np.where(img == INVALID, -1, img)
    rec = np.asarray(records, dtype=np.float32)[:, :3].astype(dtype)
    q = np.asarray(queries_dev, dtype=dtype)[:, :3]
    m = len(q)
    u, v, finite, amb = pixel(caller_frame(q.astype(np.float64), origin), W, H)
    worst0 = np.finfo(dtype).max
    out_i = np.full((m, k), -1, np.int64)
    out_d = np.full((m, k), np.inf, dtype)
    for lo in range(0, m, _CHUNK):
        hi = min(m, lo + _CHUNK)
        px = window(u[lo:hi], v[lo:hi], W, H, wh, wv, repeat_h, repeat_v)
        cand = np.where(px >= 0, img[np.maximum(px, 0)], -1)
        cand[~finite[lo:hi]] = -1
        t = rec[np.maximum(cand, 0)]
        dx = t[..., 0] - q[lo:hi, None, 0]
        dy = t[..., 1] - q[lo:hi, None, 1]
        dz = t[..., 2] - q[lo:hi, None, 2]
        d = (dx * dx + dy * dy) + dz * dz
        valid = (cand >= 0) & (d < worst0)
        d = np.where(valid, d, np.inf)
        order = np.argsort(d, axis=1, kind="stable")[:, :k]  # k smallest by (distance, scan position)
        di = np.take_along_axis(d, order, 1)
        ci = np.take_along_axis(cand, order, 1)
        ok = np.isfinite(di)
        if max_sq is not None and max_sq >= 0:
            ok &= ~(di > max_sq)
        kk = order.shape[1]
        out_i[lo:hi, :kk] = np.where(ok, ci, -1)
        out_d[lo:hi, :kk] = np.where(ok, di, np.inf)
    return out_i, out_d, amb


def nearest(index_map, records, origin, queries_dev, wh=10, wv=5, repeat_h=True, repeat_v=False, dtype=np.float64):
    """1-NN (idx (m,), d2 (m,), ambiguous (m,)): knn with k = 1 (KnnResult<1>: the first in scan order wins a tie)."""
    i, d, amb = knn(index_map, records, origin, queries_dev, 1, wh, wv, repeat_h, repeat_v, dtype)
    return i[:, 0], d[:, 0], amb


def pairs(index_map, records, origin, src_dev, T_dev, max_sq, wh=10, wv=5, repeat_h=True, repeat_v=False, dtype=np.float64):
    """The correspondences of one linearization: the source records (device frame of the source) moved by T_dev (the pose between the
    two device frames) in dtype, searched, and rejected iff d2 > max_sq (rejector.hpp:19-28).  (corr (n,) -1 = none, ambiguous (n,))."""
    T = np.asarray(T_dev, dtype=np.float64)
    p = np.asarray(src_dev, dtype=np.float32)[:, :3].astype(dtype)
    q = p @ T[:3, :3].T.astype(dtype) + T[:3, 3].astype(dtype)
    i, d, amb = nearest(index_map, records, origin, q, wh, wv, repeat_h, repeat_v, dtype)
    if max_sq is not None and max_sq >= 0:
        i = np.where(d > max_sq, -1, i)
    return i, amb

"""sga_cloud_visibility (include/small_gicp_amd.h) restated in numpy float64.  No device and no project code.

Sensor frame: x forward, y left, z up.  Projection of a point s, every operation rounded on its own:
    rho = sqrt((sx^2 + sy^2) + sz^2), az = atan2(sy, sx), el = asin(sz / rho),
    su = (az / (2 pi) + 0.5) * width,  u = (int)su, u == width -> 0,
    sv = (fov_up - el) / (fov_up - fov_down) * height,  v = floor(sv);
s is in the image iff rho > 0, everything is finite, 0 <= sv and v < height.
Range image of the scan (fp32 record + the cloud's origin): a cell holds the least rho over the returns that are finite, in the image and
have rho >= min_range; an empty cell holds +inf.
Map point i (fp32 record r, device frame at o_m; T = [R t] maps the scan's sensor frame into the map's frame, None: the identity):
    w = r + (o_m - t),  s_k = (R[0][k] w0 + R[1][k] w1) + R[2][k] w2,  rho_i = |s|.
Window of (u, v): du in -window_h .. window_h wrapping in azimuth, dv in -window_v .. window_v, rows outside the image skipped; m_i / M_i
the least / greatest finite cell.  tol_i = margin + margin_ratio rho_i.  State 0 (unobserved): s not finite, not in the image, rho_i <
min_range, rho_i > max_range, or no return in the window; 3 (seen through): rho_i + tol_i < m_i; 2 (occluded): rho_i - tol_i > M_i; 1
(consistent) otherwise.  Clearance m_i - rho_i for the states 1 .. 3, NaN for state 0.

libm's atan2 / asin may differ from the device's by an ulp: a projection is AMBIGUOUS when su or sv lies within AMBIG of an integer
(projective_ref's idea) — but for su within AMBIG of 0 or of width: both sides of that seam give u = 0."""
import numpy as np

EPS64 = float(np.finfo(np.float64).eps)
AMBIG = 1e-9
UNOBSERVED, CONSISTENT, OCCLUDED, SEEN_THROUGH = 0, 1, 2, 3
DEFAULTS = dict(width=1024, height=64, fov_up=3.0 * np.pi / 180.0, fov_down=-25.0 * np.pi / 180.0, min_range=0.5, max_range=60.0, margin=0.2, margin_ratio=0.01, window_h=1, window_v=1)


def parameters(**kw):
    p = dict(DEFAULTS)
    for name in kw:
        if name not in p:
            raise TypeError(name)
    p.update(kw)
    return p


def project(s, width, height, fov_up, fov_down):
    """-> dict: rho, su, sv (n,) float64, u, v (n,) int64 (0 where not inside), inside (n,) bool, ambiguous (n,) bool"""
    s = np.asarray(s, dtype=np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fin = np.isfinite(s).all(1)
        x, y, z = (np.where(fin, s[:, k], 0.0) for k in range(3))
        rho = np.sqrt((x * x + y * y) + z * z)
        ok = fin & (rho > 0) & np.isfinite(rho)
        safe = np.where(ok, rho, 1.0)
        az = np.arctan2(y, x)
        el = np.arcsin(z / safe)
        su = (az / (2.0 * np.pi) + 0.5) * float(width)
        sv = (fov_up - el) / (fov_up - fov_down) * float(height)
        ok &= np.isfinite(su) & np.isfinite(sv)
        su, sv = np.where(ok, su, 0.0), np.where(ok, sv, -1.0)
        u = su.astype(np.int64)  # truncation; su >= 0
        u[u == width] = 0
        vf = np.floor(sv)
        inside = ok & (sv >= 0.0) & (vf < height)
        v = np.where(inside, vf, 0.0).astype(np.int64)
        u = np.where(inside, u, 0)
        near_u = (np.abs(su - np.round(su)) < AMBIG) & ~((su < AMBIG) | (su > width - AMBIG))
        near_v = (np.abs(sv - np.round(sv)) < AMBIG) & (sv > -AMBIG) & (sv < height + AMBIG)
        amb = ok & (near_v | (near_u & (sv > -AMBIG) & (sv < height + AMBIG)))
    return {"rho": np.where(fin, rho, np.nan), "su": su, "sv": sv, "u": u, "v": v, "inside": inside, "ambiguous": amb}


def range_image(scan_rel, o_s=(0.0, 0.0, 0.0), **kw):
    """-> (image (height, width) float64 with +inf where empty, the projection of the scan's returns, unsure (height, width) bool: the
    cells an ambiguous return may land in)"""
    p = parameters(**kw)
    W, H = p["width"], p["height"]
    pts = np.asarray(scan_rel, dtype=np.float32).astype(np.float64).reshape(-1, 3) + np.asarray(o_s, dtype=np.float64)
    pr = project(pts, W, H, p["fov_up"], p["fov_down"])
    with np.errstate(invalid="ignore"):
        use = pr["inside"] & (pr["rho"] >= p["min_range"])
    img = np.full(H * W, np.inf)
    np.minimum.at(img, pr["v"][use] * W + pr["u"][use], pr["rho"][use])
    unsure = np.zeros((H, W), bool)
    with np.errstate(invalid="ignore"):
        amb = np.nonzero(pr["ambiguous"] & ~(pr["rho"] < p["min_range"] * (1 - 64 * EPS64)))[0]
    for i in amb:
        for su in (pr["su"][i] - AMBIG, pr["su"][i] + AMBIG):
            for sv in (pr["sv"][i] - AMBIG, pr["sv"][i] + AMBIG):
                u, v = int(np.floor(su)) % W, int(np.floor(sv))
                if 0 <= v < H:
                    unsure[v, u] = True
    pr["used"] = use
    return img.reshape(H, W), pr, unsure


def sensor_points(map_rel, o_m=(0.0, 0.0, 0.0), T=None):
    """-> (s (n, 3), mag (n,)): the map points in the scan's sensor frame, and the magnitudes that enter them (the 1-norm over the axes)"""
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64).reshape(4, 4)
    R, d = T[:3, :3], np.asarray(o_m, dtype=np.float64) - T[:3, 3]
    r = np.asarray(map_rel, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        w = r + d
        s = np.stack([(R[0, k] * w[:, 0] + R[1, k] * w[:, 1]) + R[2, k] * w[:, 2] for k in range(3)], axis=1)
        aw = np.abs(r) + np.abs(d)
        mag = sum(np.abs(R[j, k]) * aw[:, j] for j in range(3) for k in range(3))
    return s, mag


def window_cells(img, u, v, window_h, window_v):
    """-> (n, cells) float64: the cells of every point's window, +inf for the rows outside the image"""
    H, W = img.shape
    du = np.arange(-window_h, window_h + 1)
    dv = np.arange(-window_v, window_v + 1)
    vv = v[:, None, None] + dv[None, :, None]
    uu = (u[:, None, None] + du[None, None, :]) % W
    rows = (vv >= 0) & (vv < H)
    cells = np.where(rows, img[np.clip(vv, 0, H - 1), uu], np.inf)
    return cells.reshape(len(u), -1)


def restate(map_rel, scan_rel, o_m=(0.0, 0.0, 0.0), T=None, o_s=(0.0, 0.0, 0.0), **kw):
    """-> dict: state (n,) uint8, clearance (n,), image (H, W), counts {name: number}, finite (n,: the RECORD is finite), rho, m, M, tol,
    B (n,: the comparison band), band (indices: the points the device may state otherwise), ambiguous_scan (number of ambiguous returns)"""
    p = parameters(**kw)
    W, H = p["width"], p["height"]
    img, spr, unsure = range_image(scan_rel, o_s, **p)
    rec = np.asarray(map_rel, dtype=np.float32).reshape(-1, 3)
    n = len(rec)
    s, mag = sensor_points(rec, o_m, T)
    pr = project(s, W, H, p["fov_up"], p["fov_down"])
    rho = pr["rho"]
    with np.errstate(invalid="ignore"):
        in_range = pr["inside"] & (rho >= p["min_range"]) & (rho <= p["max_range"])
    cells = window_cells(img, pr["u"], pr["v"], p["window_h"], p["window_v"]) if n else np.zeros((0, 1))
    finite_cells = np.isfinite(cells)
    any_cell = finite_cells.any(axis=1) if n else np.zeros(0, bool)
    m = cells.min(axis=1) if n else np.zeros(0)
    M = np.where(finite_cells, cells, -np.inf).max(axis=1) if n else np.zeros(0)
    observed = in_range & any_cell
    with np.errstate(invalid="ignore"):
        tol = p["margin"] + p["margin_ratio"] * rho
        seen = observed & (rho + tol < m)
        occluded = observed & ~seen & (rho - tol > M)
    state = np.zeros(n, np.uint8)
    state[observed] = CONSISTENT
    state[occluded] = OCCLUDED
    state[seen] = SEEN_THROUGH
    with np.errstate(invalid="ignore"):
        clearance = np.where(observed, m - rho, np.nan)
    # the band: where one ulp of the device's arithmetic may decide otherwise
    with np.errstate(invalid="ignore"):
        B = 64 * EPS64 * (np.where(np.isfinite(mag), mag, 0.0) + np.where(np.isfinite(rho), rho, 0.0) + np.where(any_cell, M, 0.0))
        fin_s = np.isfinite(s).all(1)
        edge = fin_s & (np.abs(rho - p["min_range"]) <= B)
        if np.isfinite(p["max_range"]):
            edge |= fin_s & (np.abs(rho - p["max_range"]) <= B)
        edge |= in_range & any_cell & ((np.abs((m - rho) - tol) <= B) | (np.abs((rho - M) - tol) <= B))
        edge |= pr["ambiguous"]
    if n and unsure.any():
        edge |= pr["inside"] & window_cells(unsure.astype(np.float64), pr["u"], pr["v"], p["window_h"], p["window_v"]).astype(bool).any(axis=1)
    names = ("unobserved", "consistent", "occluded", "seen_through")
    return {
        "state": state, "clearance": clearance, "image": img, "counts": {name: int((state == k).sum()) for k, name in enumerate(names)}, "finite": np.isfinite(rec).all(1), "rho": rho, "m": m, "M": M,
        "tol": tol, "B": B, "band": np.nonzero(edge)[0], "ambiguous_scan": int(spr["ambiguous"].sum()), "s": s, "u": pr["u"], "v": pr["v"],
        "inside": pr["inside"], "n": n,
    }


def kept(want, keep):
    """the indices of the output cloud: keep "seen_through" | "rest", finite records only"""
    sel = (want["state"] == SEEN_THROUGH) if keep == "seen_through" else (want["state"] != SEEN_THROUGH)
    return np.nonzero(sel & want["finite"])[0]

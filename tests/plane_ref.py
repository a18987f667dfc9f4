"""tests/plane_ref.py — the rule of sga_cloud_segment_plane (include/small_gicp_amd.h) restated in numpy float64.
Nothing here goes through the library.  The draws are global_ref.draws, the generator of the correspondence RANSAC.

The restatement also marks its BAND, as cluster_ref.py does, so that a comparison can be exact everywhere else:
  scores      per hypothesis, the records i with | |dist| - threshold | <= 1e-12 max(1, |r_i - a|): an ulp of double arithmetic (the
              device fuses products into sums) can move them across the threshold;
  shaky       hypotheses whose collinearity test (|m| against 1e-9 |u| |v|) or angle test (s / |axis| against cos(max_angle)) hangs
              within 1e-12 of its limit; the refitted normal's angle test likewise ("refit_shaky");
  final       the records within 1e-9 max(1, |r_i - anchor|) of the threshold about the FINAL plane (the refitted normal carries the
              solver's error, 1e-10 rad over up to 100 m).
Sums follow the header's order where a value depends on it: |w| = sqrt((wx wx + wy wy) + wz wz), dist = (nx dx + ny dy) + nz dz.
"""
import math

import numpy as np

from global_ref import draws

DROPPED = 0xFFFFFFFF


def _norm(v):
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def _dot(n, d):
    return (n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2]


def _axis(axis):
    ax = np.zeros(3) if axis is None else np.asarray(axis, dtype=np.float64).reshape(3)
    return ax, bool(np.any(ax != 0.0))


def orient(n, axis=None, max_angle=0.0):
    """(the normals n (..., 3) turned by the rule, ok (...,): the axis constraint holds, shaky (...,): it hangs within 1e-12)"""
    n = np.array(n, dtype=np.float64)
    ax, has = _axis(axis)
    if has:
        s = _dot(n, ax)
        flip = s < 0.0
        n = np.where(flip[..., None], -n, n)
        s = np.where(flip, -s, s)
        ratio = s / _norm(ax)
        lim = math.cos(float(max_angle))
        return n, ratio >= lim, np.abs(ratio - lim) <= 1e-12
    lead = np.where(n[..., 2] != 0.0, n[..., 2], np.where(n[..., 1] != 0.0, n[..., 1], n[..., 0]))
    n = np.where((lead < 0.0)[..., None], -n, n)
    return n, np.ones(n.shape[:-1], bool), np.zeros(n.shape[:-1], bool)


def hypotheses(records, iterations, seed=0, axis=None, max_angle=0.0):
    """{"triple" (H, 3), "nhat" (H, 3), "a" (H, 3), "valid" (H,), "shaky" (H,)} of the fp32 records (n >= 3)"""
    r = np.asarray(records, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    H = int(iterations)
    tri = draws(seed, np.arange(H), len(r))
    with np.errstate(all="ignore"):
        a, b, c = r[tri[:, 0]], r[tri[:, 1]], r[tri[:, 2]]
        u, v = b - a, c - a
        m = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)
        lm, lim = _norm(m), 1e-9 * _norm(u) * _norm(v)
        dropped = ~(lm > 0.0) | (lm < lim) | ~(lm < np.inf)
        # within 1e-12 of |u| |v|; u = 0 or v = 0 gives m = 0 exactly in any arithmetic: dropped, and nothing hangs on an ulp
        shaky = np.isfinite(lm) & np.isfinite(lim) & (lim > 0.0) & (np.abs(lm - lim) <= 1e-12 * (1e9 * lim))
        nhat = m / np.where(dropped, 1.0, lm)[:, None]
        nhat, ok, edge = orient(nhat, axis, max_angle)
    valid = ~dropped & ok
    shaky = shaky | (~dropped & edge)
    nhat = np.where(valid[:, None], nhat, 0.0)
    return {"triple": tri, "nhat": nhat, "a": a, "valid": valid, "shaky": shaky}


def distances(r, nhat, a):
    """dist (h, n) of the records r (n, 3) from the planes (nhat, a) (h, 3), and |r_i - a| (h, n)"""
    with np.errstate(all="ignore"):
        dx, dy, dz = r[None, :, 0] - a[:, 0, None], r[None, :, 1] - a[:, 1, None], r[None, :, 2] - a[:, 2, None]
        dist = (nhat[:, 0, None] * dx + nhat[:, 1, None] * dy) + nhat[:, 2, None] * dz
        far = np.sqrt((dx * dx + dy * dy) + dz * dz)
    return dist, far


def score(r, hyp, threshold, cells=1 << 22):
    """(scores (H,) uint32 with DROPPED for a dropped hypothesis, band (H,) int64) by a chunked H x N product"""
    H, n = len(hyp["valid"]), len(r)
    scores, band = np.full(H, DROPPED, np.uint32), np.zeros(H, np.int64)
    live = np.flatnonzero(hyp["valid"] | hyp["shaky"])
    step = max(1, cells // max(n, 1))
    for s in range(0, len(live), step):
        hs = live[s:s + step]
        dist, far = distances(r, hyp["nhat"][hs], hyp["a"][hs])
        with np.errstate(all="ignore"):
            ad = np.abs(dist)
            inl = (ad <= threshold).sum(axis=1)
            near = (np.isfinite(far) & (np.abs(ad - threshold) <= 1e-12 * np.maximum(1.0, far))).sum(axis=1)  # (a non-finite record is no inlier, whatever an ulp does)
        scores[hs] = np.where(hyp["valid"][hs], inl, DROPPED).astype(np.uint32)
        band[hs] = near
    return scores, band


def segment_plane(records, distance_threshold=0.1, iterations=1000, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, origin=(0.0, 0.0, 0.0)):
    """The whole rule over the fp32 records (device frame at `origin`):
    {"scores" (H,) uint32, "band" (H,) int64, "shaky" (H,) bool, "scored", "best_hypothesis" (-1: none), "hypothesis_inliers",
     "found" bool, "plane" (4,), "normal", "anchor", "inliers", "inlier_mask" (n,) bool, "rmse", "refit" 0 | 1, "refit_shaky" bool,
     "final_band" int: records within 1e-9 of the threshold about the final plane, "records64": the records as doubles}"""
    r = np.asarray(records, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    n, H = len(r), int(iterations)
    out = {"scores": np.full(H, DROPPED, np.uint32), "band": np.zeros(H, np.int64), "shaky": np.zeros(H, bool), "scored": 0, "best_hypothesis": -1, "hypothesis_inliers": 0, "found": False,
           "plane": np.zeros(4), "normal": np.zeros(3), "anchor": np.zeros(3), "inliers": 0, "inlier_mask": np.zeros(n, bool), "rmse": 0.0, "refit": 0, "refit_shaky": False, "final_band": 0, "records64": r}
    if n < 3:
        return out
    hyp = hypotheses(r, H, seed, axis, max_angle)
    out["scores"], out["band"] = score(r, hyp, distance_threshold)
    out["shaky"] = hyp["shaky"]
    out["scored"] = int(hyp["valid"].sum())
    if out["scored"] == 0:
        return out
    best = int(np.argmax(np.where(hyp["valid"], out["scores"].astype(np.int64), -1)))  # the first of equal scores: the lowest h
    out["best_hypothesis"], out["hypothesis_inliers"] = best, int(out["scores"][best])
    if out["hypothesis_inliers"] < int(min_inliers):
        return out
    out["found"] = True
    normal, anchor = hyp["nhat"][best], hyp["a"][best]
    dist, _ = distances(r, normal[None], anchor[None])
    with np.errstate(all="ignore"):
        inl = np.abs(dist[0]) <= distance_threshold
    if refit:
        x = r[inl] - anchor
        k = len(x)
        if k >= 3:
            mean = x.sum(axis=0) / k
            y = x - mean
            w, V = np.linalg.eigh(y.T @ y)
            if w[1] - w[0] > 1e-12 * w[2]:
                nf, ok, edge = orient(V[:, 0] / _norm(V[:, 0]), axis, max_angle)
                out["refit_shaky"] = bool(edge)
                if ok:
                    normal, anchor = nf, anchor + mean
                    out["refit"] = 1
    dist, far = distances(r, normal[None], anchor[None])
    with np.errstate(all="ignore"):
        ad = np.abs(dist[0])
        mask = ad <= distance_threshold
        out["final_band"] = int((np.isfinite(far[0]) & (np.abs(ad - distance_threshold) <= 1e-9 * np.maximum(1.0, far[0]))).sum())
    out["normal"], out["anchor"], out["inlier_mask"], out["inliers"] = normal, anchor, mask, int(mask.sum())
    out["rmse"] = float(np.sqrt(np.mean(dist[0][mask] ** 2))) if mask.any() else 0.0
    o = np.asarray(origin, dtype=np.float64)
    out["plane"] = np.array([normal[0], normal[1], normal[2], -_dot(normal, anchor + o)])
    return out


def segment_planes(records, max_planes, distance_threshold=0.1, iterations=1000, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, origin=(0.0, 0.0, 0.0)):
    """The host loop: round r runs the rule with seed + r on what round r - 1 left.  {"labels" (n,) int32, "planes": the rounds' results,
    "rest_indices", "clean": no round had a score band, a shaky hypothesis or a final band}"""
    r = np.asarray(records, dtype=np.float32).reshape(-1, 3)
    index = np.arange(len(r), dtype=np.int64)
    labels = np.full(len(r), -1, np.int32)
    planes, clean = [], True
    for rnd in range(int(max_planes)):
        res = segment_plane(r[index], distance_threshold, iterations, (int(seed) + rnd) & 0xFFFFFFFFFFFFFFFF, axis, max_angle, min_inliers, refit, origin)
        clean = clean and int(res["band"].sum()) == 0 and not res["shaky"].any() and res["final_band"] == 0 and not res["refit_shaky"]
        if not res["found"] or res["inliers"] < int(min_inliers):
            break
        labels[index[res["inlier_mask"]]] = rnd
        index = index[~res["inlier_mask"]]
        planes.append(res)
    return {"labels": labels, "planes": planes, "rest_indices": index, "clean": clean}


def plane_error(plane, ref, at=(0.0, 0.0, 0.0)):
    """(angle between the normals in radians, |difference of the signed distances of the point `at`| in metres)"""
    n, m = np.asarray(plane[:3], dtype=np.float64), np.asarray(ref[:3], dtype=np.float64)
    p = np.asarray(at, dtype=np.float64)
    return float(np.arctan2(_norm(np.cross(n, m)), float(n @ m))), float(abs((n @ p + plane[3]) - (m @ p + ref[3])))

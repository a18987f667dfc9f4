"""The ISS keypoint rule of DESIGN.md section 3.28 (include/small_gicp_amd.h: sga_cloud_iss_keypoints) restated in numpy float64 and
scipy's cKDTree, never through the library.

Records are the fp32 values the device holds (a cloud's points minus its origin).  For point i, with x_j = r_j - r_i in double:
  1  N_i(r) = { j : d2(i, j) <= r r }, d2 = ((dx dx) + (dy dy)) + (dz dz); i is a member.  The tree only proposes candidates (a ball a
     little wider than r); every candidate is then held against the exact predicate, as cluster_ref.neighbours recomputes it.
  2  s = sum x_j, S = sum x_j x_j^T over N_i(salient_radius); C = S / c - (s / c)(s / c)^T; l1 >= l2 >= l3 from numpy.linalg.eigvalsh.
  3  sal_i = l3 when c >= min_neighbors, l1 > 0, l2 < gamma_21 l1, l3 < gamma_32 l2 and l3 > 1e-9 l1; else 0.
  4  i is a keypoint iff sal_i > 0, |N_i(non_max_radius)| >= min_neighbors, and no j != i of that window has sal_j > sal_i, or sal_j ==
     sal_i with j < i.

THE BAND holds the points whose result an implementation that sums in another order, or solves the eigenproblem another way, may decide
differently: a neighbour within 1e-12 max(1, r^2) of either radius (in d2); a test of rule 3 within 1e-12 l1 of its limit; a window
neighbour whose saliency lies within 2e-12 max(l1_i, l1_j) of the point's own without being bytewise equal to it; and every point with
such a point in its window."""
import numpy as np
from scipy.spatial import cKDTree

BAND = 1e-12
FLOOR = 1e-9


def bumpy_surface(n, seed, side=10.0, spacing=0.1):
    """n random points (float32) of a bumpy surface over a side x side square: z = six Gaussians + 0.02 m of noise.  xy is drawn
    uniformly; a draw closer than `spacing` (in xy) to an earlier point is drawn again.  Why: the covariance of rule 2 does not depend
    on the query, so two points with the SAME neighbour set — likely for two points a centimetre apart — tie up to rounding, and a
    cloud with a dozen such pairs has a tenth of its points in the band."""
    g = np.random.default_rng(seed)
    xy = np.zeros((0, 2))
    while len(xy) < n:
        c = g.uniform(0.0, side, 2)
        if len(xy) == 0 or ((xy - c) ** 2).sum(axis=1).min() >= spacing * spacing:
            xy = np.vstack([xy, c])
    z = np.zeros(n)
    for _ in range(6):
        c, h, w = g.uniform(0.0, side, 2), g.uniform(-1.0, 1.0), g.uniform(0.5, 1.5)
        z += h * np.exp(-((xy - c) ** 2).sum(axis=1) / (2.0 * w * w))
    z += 0.02 * g.standard_normal(n)
    return np.ascontiguousarray(np.column_stack([xy, z]), dtype=np.float32)


def neighbourhoods(rec64, tree, radius):
    """-> (lists, near): lists[i] = the indices j (ascending) with d2(i, j) <= radius^2; near[i] = some candidate's d2 lies within
    1e-12 max(1, radius^2) of radius^2"""
    r2 = float(radius) * float(radius)
    slack = BAND * max(1.0, r2)
    cand = tree.query_ball_point(rec64, float(radius) * (1.0 + 1e-9) + 1e-9, return_sorted=True) if len(rec64) else []
    lists, near = [], np.zeros(len(rec64), bool)
    for i, c in enumerate(cand):
        c = np.asarray(c, np.int64)
        d = rec64[c] - rec64[i]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        lists.append(c[d2 <= r2])
        near[i] = bool((np.abs(d2 - r2) <= slack).any())
    return lists, near


def iss(records, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5):
    """The keypoints of the fp32 records (n,3).  Returns a dict: indices (int64, ascending), saliency, l1, l2, l3 (float64 per point; the
    eigenvalues are 0 where the point has fewer than min_neighbors neighbours), count_salient / count_window (the sizes of the two
    neighbourhoods), keypoint (bool per point), band (bool per point) and ties: the salient points with a bytewise-equal saliency in
    their window (exact ties: expected of duplicated points and of lattices, whose sums are exact, and an accident elsewhere)."""
    rec32 = np.asarray(records, np.float32).reshape(-1, 3)
    rec = rec32.astype(np.float64)
    n = len(rec)
    tree = cKDTree(rec) if n else None
    sal_lists, near_s = neighbourhoods(rec, tree, salient_radius)
    win_lists, near_w = neighbourhoods(rec, tree, non_max_radius)
    sal, l1s, l2s, l3s = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    shaky = near_s | near_w
    cs = np.array([len(v) for v in sal_lists], np.int64).reshape(n)
    cw = np.array([len(v) for v in win_lists], np.int64).reshape(n)
    for i in range(n):
        c = cs[i]
        if c < min_neighbors:
            continue
        x = rec[sal_lists[i]] - rec[i]
        m = x.sum(axis=0) / c
        cov = (x.T @ x) / c - np.outer(m, m)
        l3, l2, l1 = np.linalg.eigvalsh(cov)
        l1s[i], l2s[i], l3s[i] = l1, l2, l3
        tests = (l1 > 0.0, l2 < gamma_21 * l1, l3 < gamma_32 * l2, l3 > FLOOR * l1)
        margins = (l1, gamma_21 * l1 - l2, gamma_32 * l2 - l3, l3 - FLOOR * l1)
        if l1 > 0.0 and any(abs(v) <= BAND * l1 for v in margins[1:]):
            shaky[i] = True
        if all(tests):
            sal[i] = l3
    keypoint = np.zeros(n, bool)
    close = np.zeros(n, bool)
    ties = 0
    for i in range(n):
        w = win_lists[i]
        w = w[w != i]
        if len(w):
            scale = np.maximum(l1s[i], l1s[w])
            near = (np.abs(sal[w] - sal[i]) <= 2.0 * BAND * scale) & (sal[w] != sal[i]) & (scale > 0.0)
            close[i] = bool(near.any())
            ties += int(sal[i] > 0.0 and (sal[w] == sal[i]).any())
        if sal[i] > 0.0 and cw[i] >= min_neighbors:
            keypoint[i] = not bool(((sal[w] > sal[i]) | ((sal[w] == sal[i]) & (w < i))).any())
    shaky |= close
    band = shaky.copy()
    for i in range(n):
        if shaky[win_lists[i]].any():
            band[i] = True
    return {"indices": np.flatnonzero(keypoint).astype(np.int64), "saliency": sal, "l1": l1s, "l2": l2s, "l3": l3s, "count_salient": cs, "count_window": cw, "keypoint": keypoint, "band": band, "ties": ties}

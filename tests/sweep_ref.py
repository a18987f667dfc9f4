"""Sweep registration restated in numpy float64: the pose of every point by a 30-term series of the exponential,
the left Jacobian of SE(3) by a 30-term series, brute-force nearest neighbours, the three factors, H / b / e over GIVEN pairs, and the
LM loop in 12 dimensions.  Twists are rotation first ([rx ry rz tx ty tz]); T is target <- sensor at ref_time; point i has the pose
exp((times[i] - ref_time) xi).  Nothing here is fast; everything is meant to be read next to the header's statement of the model."""
import numpy as np

ICP, PLANE_ICP, GICP = 0, 1, 2
TERMS = 30


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def hat(x):
    X = np.zeros((4, 4))
    X[:3, :3] = skew(x[:3])
    X[:3, 3] = x[3:]
    return X


def ad(x):
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = skew(x[:3])
    A[3:, :3] = skew(x[3:])
    return A


def _power_series(X, scales, first_factorial):
    """sum_k scales^k X^k / (k + first_factorial)! for every scale: (n, d, d)"""
    d = X.shape[0]
    scales = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    out = np.zeros((len(scales), d, d))
    P = np.eye(d)
    c = np.ones(len(scales))
    for k in range(1, first_factorial + 1):
        c = c / k
    for k in range(TERMS + 1):
        out += c[:, None, None] * P
        P = P @ X
        c = c * scales / (k + 1 + first_factorial)
    return out


def se3_exp(x, a=1.0):
    """exp(a x) for every a: (n, 4, 4), or (4, 4) for a number"""
    E = _power_series(hat(np.asarray(x, dtype=np.float64)), a, 0)
    return E[0] if np.ndim(a) == 0 else E


def left_jacobian(x, a=1.0):
    """J_l(a x) = sum_k ad(a x)^k / (k + 1)!"""
    Jl = _power_series(ad(np.asarray(x, dtype=np.float64)), a, 1)
    return Jl[0] if np.ndim(a) == 0 else Jl


def posed(points, times, T, xi, ref_time):
    """(p'_i = E_i p_i, q_i = T p'_i, R_Ei, a_i) of points (n, 3)"""
    a = np.asarray(times, dtype=np.float32).astype(np.float64) - ref_time
    E = se3_exp(xi, a)
    pp = np.einsum("nij,nj->ni", E[:, :3, :3], points) + E[:, :3, 3]
    q = pp @ T[:3, :3].T + T[:3, 3]
    return pp, q, E[:, :3, :3], a


def _sq_distances(q, target):
    """|q_i - t_j|^2 from the differences themselves (no |q|^2 + |t|^2 - 2 q.t, which cancels): (len(q), len(target))"""
    D = (q[:, 0:1] - target[None, :, 0]) ** 2
    D += (q[:, 1:2] - target[None, :, 1]) ** 2
    D += (q[:, 2:3] - target[None, :, 2]) ** 2
    return D


def nearest(target, q, chunk=512):
    """brute force: (index of the nearest target point, squared distance, the runner-up's squared distance) per query"""
    idx, d2, second = np.full(len(q), -1, np.int64), np.full(len(q), np.inf), np.full(len(q), np.inf)
    if len(target) == 0:
        return idx, d2, second
    for s in range(0, len(q), chunk):
        D = _sq_distances(q[s : s + chunk], target)
        j = D.argmin(1)
        idx[s : s + chunk], d2[s : s + chunk] = j, D[np.arange(len(j)), j]
        if target.shape[0] > 1:
            D[np.arange(len(j)), j] = np.inf
            second[s : s + chunk] = D.min(1)
    return idx, d2, second


def pairs(target, points, times, T, xi, ref_time, max_dist_sq):
    """the pair of every point (-1: none) at a state"""
    _, q, _, _ = posed(points, times, T, xi, ref_time)
    idx, d2, _ = nearest(target, q)
    ok = np.isfinite(q).all(1) & (idx >= 0)
    if max_dist_sq >= 0:
        ok &= d2 <= max_dist_sq
    return np.where(ok, idx, -1)


def weights(kind, T, RE, j, target_normals=None, target_covs=None, source_covs=None):
    """M of every pair (n, 3, 3); rows without a pair hold zeros"""
    n = len(j)
    M = np.zeros((n, 3, 3))
    ok = j >= 0
    if kind == ICP:
        M[ok] = np.eye(3)
    elif kind == PLANE_ICP:
        nn = target_normals[j[ok]]
        M[ok] = np.einsum("ni,ij->nij", nn * nn, np.eye(3))
    else:
        R = T[:3, :3] @ RE[ok]
        S = target_covs[j[ok]] + R @ source_covs[ok] @ np.transpose(R, (0, 2, 1))
        M[ok] = np.linalg.inv(S)
    return M


def residual_and_jacobian(target, points, times, T, xi, ref_time, j):
    """(r (n, 3), J (n, 3, 12), RE) over given pairs; rows without a pair hold zeros"""
    pp, q, RE, a = posed(points, times, T, xi, ref_time)
    n = len(points)
    ok = j >= 0
    r = np.zeros((n, 3))
    r[ok] = target[j[ok]] - q[ok]
    R = T[:3, :3]
    J = np.zeros((n, 3, 12))
    A = a[:, None, None] * left_jacobian(xi, a)
    S = np.zeros((n, 3, 3))  # skew(p'_i)
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0], S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -pp[:, 2], pp[:, 1], pp[:, 2], -pp[:, 0], -pp[:, 1], pp[:, 0]
    J[ok, :, :3] = (R @ S)[ok]
    J[ok, :, 3:6] = -R
    J[ok, :, 6:] = (J[:, :, :6] @ A)[ok]
    return r, J, RE


def per_pair(kind, target, points, times, T, xi, ref_time, j, M=None, target_normals=None, target_covs=None, source_covs=None):
    """H_i (n, 12, 12), b_i (n, 12), e_i (n,) and the M used, over given pairs (and a given M, when there is one)"""
    r, J, RE = residual_and_jacobian(target, points, times, T, xi, ref_time, j)
    if M is None:
        M = weights(kind, T, RE, j, target_normals, target_covs, source_covs)
    MJ = M @ J
    H = np.transpose(J, (0, 2, 1)) @ MJ
    b = np.einsum("nij,ni->nj", MJ, r)
    e = 0.5 * np.einsum("ni,nij,nj->n", r, M, r)
    return H, b, e, M


def magnitudes(target, points, times, T, xi, ref_time, j, M):
    """The absolute contributions to every entry, per pair: |J|^T |M| |J| (n, 12, 12), |J|^T |M| |r| (n, 12) and |r|^T |M| |r| / 2 (n,) —
    every product that enters an entry, taken absolutely (tests/factor_ref.py's Hmag and bmag).  An entry that cancels within a pair —
    R^T R's off-diagonals under ICP are zero but for rounding — has no scale of its own; its products have."""
    r, J, _ = residual_and_jacobian(target, points, times, T, xi, ref_time, j)
    aJ, aM, ar = np.abs(J), np.abs(M), np.abs(r)
    return np.einsum("nki,nkl,nlj->nij", aJ, aM, aJ), np.einsum("nki,nkl,nl->ni", aJ, aM, ar), 0.5 * np.einsum("nk,nkl,nl->n", ar, aM, ar)


def sums(H, b, e):
    """(H, b, e) summed over the pairs"""
    return H.sum(0), b.sum(0), e.sum()


def estimate_covariances(points, k=10):
    """the reference's covariances: k nearest neighbours (the point itself among them), eigenvalues replaced by (1e-3, 1, 1)"""
    n = len(points)
    out = np.zeros((n, 3, 3))
    for s in range(0, n, 512):
        D = _sq_distances(points[s : s + 512], points)
        nn = np.argpartition(D, min(k, n - 1), axis=1)[:, :k]
        P = points[nn]  # (c, k, 3)
        X = P - P.mean(1, keepdims=True)
        C = np.transpose(X, (0, 2, 1)) @ X / (k - 1)
        _, V = np.linalg.eigh(C)
        out[s : s + 512] = V @ np.diag([1e-3, 1.0, 1.0]) @ np.transpose(V, (0, 2, 1))
    return out


class Result:
    pass


def lm(kind, target, points, times, max_dist_sq=1.0, T=None, xi=None, ref_time=1.0, twist_prior=None, twist_information=None, hold_twist=False, target_normals=None, target_covs=None, source_covs=None,
       max_iterations=20, max_inner_iterations=10, init_lambda=1e-3, lambda_factor=10.0, rotation_eps=0.1 * np.pi / 180.0, translation_eps=1e-3):
    """optimizer.hpp:83-149 in 12 dimensions (hold_twist: in the 6 of the pose, the twist kept as given)"""
    T = np.eye(4) if T is None else np.array(T, dtype=np.float64)
    xi = np.zeros(6) if xi is None else np.array(xi, dtype=np.float64)
    x0 = np.zeros(6) if twist_prior is None else np.asarray(twist_prior, dtype=np.float64)
    L = np.zeros((6, 6)) if twist_information is None else np.asarray(twist_information, dtype=np.float64)
    dim = 6 if hold_twist else 12
    kw = dict(target_normals=target_normals, target_covs=target_covs, source_covs=source_covs)
    res = Result()
    res.converged, res.iterations = False, 0
    lam = init_lambda
    for it in range(max_iterations):
        if res.converged:
            break
        j = pairs(target, points, times, T, xi, ref_time, max_dist_sq)
        Hs, bs, es, M = per_pair(kind, target, points, times, T, xi, ref_time, j, **kw)
        H, b, e = Hs.sum(0), bs.sum(0), es.sum()
        H[6:, 6:] += L
        b[6:] += L @ (xi - x0)
        e += 0.5 * (xi - x0) @ L @ (xi - x0)
        success = False
        for _ in range(max_inner_iterations):
            delta = np.zeros(12)
            delta[:dim] = np.linalg.solve(H[:dim, :dim] + lam * np.eye(dim), -b[:dim])
            new_T, new_xi = T @ se3_exp(delta[:6]), xi + delta[6:]
            new_e = per_pair(kind, target, points, times, new_T, new_xi, ref_time, j, M=M)[2].sum() + 0.5 * (new_xi - x0) @ L @ (new_xi - x0)
            if new_e <= e:
                d = delta
                res.converged = bool(
                    np.linalg.norm(d[:3]) <= rotation_eps and np.linalg.norm(d[3:6]) <= translation_eps and np.linalg.norm(d[6:9]) <= rotation_eps and np.linalg.norm(d[9:]) <= translation_eps
                )
                T, xi, e = new_T, new_xi, new_e
                lam /= lambda_factor
                success = True
                break
            lam *= lambda_factor
        res.iterations = it
        res.H, res.b, res.error = H, b, e
        if not success:
            break
    res.T_target_source, res.twist, res.num_inliers = T, xi, int((j >= 0).sum())
    return res


def pose_error(T, T_true):
    """(translation error in metres, rotation error in radians)"""
    E = np.linalg.inv(T_true) @ T
    return float(np.linalg.norm(E[:3, 3])), float(np.arccos(np.clip((np.trace(E[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))

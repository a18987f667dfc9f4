"""Test helper: the linearization sums of the three factors restated in float64 over a GIVEN set of correspondences.

The GPU passes pick their own pairs; the sums over exactly those pairs are what this module computes, so a test can separate "the pairs
are right" (checked with an independent nearest-neighbour search) from "the sums over the pairs are right" (checked here).  Every number
is accumulated in float64 from the fp32 values the device stores.  Written from the reference's factors:

  ICP        factors/icp_factor.hpp:43-51        r = t - T p,  J = [R skew(p) | -R],  H = J^T J,  b = J^T r,  e = 1/2 |r|^2
  PLANE_ICP  factors/plane_icp_factor.hpp:45-54  err = n * r (element-wise), J = diag(n) [R skew(p) | -R],  H = J^T J,  b = J^T err,
                                                 e = 1/2 |err|^2
  GICP       factors/gicp_factor.hpp:59-70       M = (C_t + R C_s R^T)^-1,  H = J^T M J,  b = J^T M r,  e = 1/2 r^T M r
  robust     factors/robust_kernel.hpp:24-27, 47, 85-88: w = weight(sqrt(e)) scales H, b and e; Huber: 1 if s < c else c / s,
             Cauchy: c / (c + s^2)
  rejector   registration/rejector.hpp:23-24: a pair is rejected iff sq_dist > max_dist_sq (double)
  error      factors/*_factor.hpp error(): the stale correspondence (and GICP's stale mahalanobis) at a trial pose, robustified as
             robust_kernel.hpp:95-97; summed as registration/reduction_omp.hpp:62-67 does.

per_pair() is linearize() before its sum — H_i, b_i, e_i and M_i of every pair, with the magnitudes that bound their rounding — for the
outputs a pass leaves per pair (tests/test_pass_outputs_gpu.py); tests/test_factor_ref.py holds its sums to linearize().

Kinds and robust kinds use the C-ABI numbering: ICP 0, PLANE_ICP 1, GICP 2; none 0, Huber 1, Cauchy 2.
"""
import numpy as np

ICP, PLANE_ICP, GICP = 0, 1, 2
ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY = 0, 1, 2
_CHUNK = 1 << 17  # pairs per block of the per-pair arrays (bounded memory at a million points)


def skew(p):
    z = np.zeros(len(p))
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], -1), np.stack([p[:, 2], z, -p[:, 0]], -1), np.stack([-p[:, 1], p[:, 0], z], -1)], 1)


def robust_weight(kind, c, e):
    """robust_kernel.hpp:24-27 (Huber) and :47 (Cauchy), evaluated at sqrt(e) as RobustFactor does (:85, :97)."""
    s = np.sqrt(e)
    if kind == ROBUST_HUBER:
        return np.where(s < c, 1.0, c / np.where(s > 0, s, 1.0))
    if kind == ROBUST_CAUCHY:
        return c / (c + s * s)
    return np.ones_like(e)


def _cov3(c):
    c = np.asarray(c, dtype=np.float64)
    return c[:, :3, :3] if c.ndim == 3 else c.reshape(-1, 3, 3)


def transform(T, p):
    """T p for every row of p, in float64."""
    T = np.asarray(T, dtype=np.float64)
    return np.asarray(p, dtype=np.float64) @ T[:3, :3].T + T[:3, 3]


def sq_dist(src, tgt, corr, T):
    """|t_corr[i] - T p_i|^2 in float64 for the pairs corr[i] >= 0; inf elsewhere."""
    corr = np.asarray(corr)
    ok = corr >= 0
    d2 = np.full(len(corr), np.inf)
    r = np.asarray(tgt, dtype=np.float64)[corr[ok]] - transform(T, np.asarray(src)[ok])
    d2[ok] = (r * r).sum(1)
    return d2


def mahalanobis(kind, T, src_cov=None, tgt_cov=None, tgt_nrm=None, src_idx=None, tgt_idx=None):
    """The per-pair M of the factor: identity (ICP), diag(n^2) (PLANE_ICP: err = n * r, so 1/2 |err|^2 = 1/2 r^T diag(n^2) r), or the
    fused GICP precision (gicp_factor.hpp:59-60)."""
    m = len(src_idx)
    if kind == GICP:
        R = np.asarray(T, dtype=np.float64)[:3, :3]
        Cs, Ct = _cov3(src_cov)[src_idx], _cov3(tgt_cov)[tgt_idx]
        return np.linalg.inv(Ct + R @ Cs @ R.T)
    if kind == PLANE_ICP:
        n = np.asarray(tgt_nrm, dtype=np.float64)[tgt_idx][:, :3]
        M = np.zeros((m, 3, 3))
        M[:, [0, 1, 2], [0, 1, 2]] = n * n
        return M
    return np.broadcast_to(np.eye(3), (m, 3, 3))


class Sums:
    """H (6, 6), b (6,), e, the inlier count, and (GICP) the mahalanobis matrix of every source point (zeros for an outlier)."""

    def __init__(self, H, b, e, inliers, maha):
        self.H, self.b, self.e, self.inliers, self.maha = H, b, e, inliers, maha


def linearize(src, tgt, corr, T, kind, robust=ROBUST_NONE, c=1.0, src_cov=None, tgt_cov=None, tgt_nrm=None):
    """The sums of one linearization at pose T over the pairs (i, corr[i]) with corr[i] >= 0 (corr: target index in the caller's
    order, -1 = no pair).  Every given pair counts; the caller decides which pairs a rejector keeps."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    corr = np.asarray(corr)
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    n = len(corr)
    H, b, e = np.zeros((6, 6)), np.zeros(6), 0.0
    maha = np.zeros((n, 3, 3))
    inl = np.flatnonzero(corr >= 0)
    for lo in range(0, len(inl), _CHUNK):
        si = inl[lo:lo + _CHUNK]
        ti = corr[si]
        p = src[si][:, :3]
        r = tgt[ti][:, :3] - (p @ R.T + T[:3, 3])
        M = mahalanobis(kind, T, src_cov, tgt_cov, tgt_nrm, si, ti)
        if kind == GICP:
            maha[si] = M
        J = np.zeros((len(si), 3, 6))
        J[:, :, :3] = R[None] @ skew(p)
        J[:, :, 3:] = -R[None]
        MJ = M @ J
        Mr = np.einsum("nij,nj->ni", M, r)
        ei = 0.5 * np.einsum("ni,ni->n", r, Mr)
        w = robust_weight(robust, c, ei)
        H += np.einsum("n,nki,nkj->ij", w, J, MJ)
        b += np.einsum("n,nki,nk->i", w, J, Mr)
        e += float((w * ei).sum())
    H = np.triu(H) + np.triu(H, 1).T  # one value per entry pair, as the engine's 21-value upper triangle
    return Sums(H, b, e, len(inl), maha)


class Pairs:
    """What per_pair returns, one row per pair (i, corr[i]) with corr[i] >= 0, in the order of idx (the source indices): H (m, 6, 6),
    b (m, 6), e (m,) with the robust weight applied, M (m, 3, 3) the factor's own matrix (no weight), and the magnitudes
    Hmag = w |J|^T |M| |J| and bmag = w |J|^T |M| |r|, which bound what rounding each product once can do to H and b."""

    def __init__(self, idx, H, b, e, M, Hmag, bmag):
        self.idx, self.H, self.b, self.e, self.M, self.Hmag, self.bmag = idx, H, b, e, M, Hmag, bmag


def per_pair(src, tgt, corr, T, kind, robust=ROBUST_NONE, c=1.0, src_cov=None, tgt_cov=None, tgt_nrm=None):
    """linearize() before its sum: the system of every pair (i, corr[i]) with corr[i] >= 0 at pose T, in float64, by the formulas of the
    header (H_i = w J^T M J, b_i = w J^T M r, e_i = w 1/2 r^T M r, w the robust weight at sqrt(1/2 r^T M r))."""
    T = np.asarray(T, dtype=np.float64)
    R = T[:3, :3]
    corr = np.asarray(corr)
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    si = np.flatnonzero(corr >= 0)
    ti = corr[si]
    p = src[si][:, :3]
    # the residual alone is formed in extended precision (64-bit mantissa where numpy has it) and then rounded: in float64 the rounding of
    # q = R p + t, 1e-14 m at 50 m, is 1e-9 of a point-to-plane residual of 1e-5 m, ten times the bound this restatement is used with
    L = np.longdouble
    r = (tgt[ti][:, :3].astype(L) - ((p.astype(L)[:, None, :] * R.astype(L)[None]).sum(2) + T[:3, 3].astype(L))).astype(np.float64)
    M = np.array(mahalanobis(kind, T, src_cov, tgt_cov, tgt_nrm, si, ti))
    J = np.zeros((len(si), 3, 6))
    J[:, :, :3] = R[None] @ skew(p)
    J[:, :, 3:] = -R[None]
    Mr = np.einsum("nij,nj->ni", M, r)
    e0 = 0.5 * np.einsum("ni,ni->n", r, Mr)
    w = robust_weight(robust, c, e0)
    H = w[:, None, None] * np.einsum("nki,nkl,nlj->nij", J, M, J)
    b = w[:, None] * np.einsum("nki,nk->ni", J, Mr)
    aJ, aM = np.abs(J), np.abs(M)
    Hmag = w[:, None, None] * np.einsum("nki,nkl,nlj->nij", aJ, aM, aJ)
    bmag = w[:, None] * np.einsum("nki,nkl,nl->ni", aJ, aM, np.abs(r))
    return Pairs(si, H, b, w * e0, M, Hmag, bmag)


def error(src, tgt, corr, T, kind, robust=ROBUST_NONE, c=1.0, maha=None, tgt_nrm=None):
    """Reduction::error at a trial pose T: the stale pairs corr of the last linearization and, for GICP, the mahalanobis matrices it
    cached (maha, (n, 3, 3) by source point — Sums.maha)."""
    T = np.asarray(T, dtype=np.float64)
    corr = np.asarray(corr)
    src, tgt = np.asarray(src, dtype=np.float64), np.asarray(tgt, dtype=np.float64)
    inl = np.flatnonzero(corr >= 0)
    total = 0.0
    for lo in range(0, len(inl), _CHUNK):
        si = inl[lo:lo + _CHUNK]
        ti = corr[si]
        r = tgt[ti][:, :3] - transform(T, src[si][:, :3])
        if kind == GICP:
            M = np.asarray(maha, dtype=np.float64)[si]
        else:
            M = mahalanobis(kind, T, None, None, tgt_nrm, si, ti)
        ei = 0.5 * np.einsum("ni,nij,nj->n", r, M, r)
        total += float((robust_weight(robust, c, ei) * ei).sum())
    return total

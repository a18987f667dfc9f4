"""tests/factor_ref.py — the float64 restatement the route matrix (test_route_matrix.py) measures every GPU pass against — pinned to the
CPU oracle on config C1 over the oracle's own correspondences: every factor kind, no robust kernel / Huber / Cauchy, the three poses of
test_gpu_parity.py, linearization and the error at a trial pose with the stale pairs and mahalanobis matrices."""
import numpy as np
import pytest

import factor_ref as fr

C = 0.7
POSES = [
    np.eye(4),
    (0.1, 0.2, 1.0, 0.7, (0.49, 0.12, -0.02)),
    (1.0, -1.0, 0.3, 5.0, (-0.4, 0.3, 0.2)),
]


def se3(axis, deg, t):
    a = np.asarray(axis, dtype=np.float64)
    k = a / np.linalg.norm(a)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    ang = np.deg2rad(deg)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K
    T[:3, 3] = t
    return T


def pose(p):
    return p if isinstance(p, np.ndarray) else se3(p[:3], p[3], p[4])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("robust", [fr.ROBUST_NONE, fr.ROBUST_HUBER, fr.ROBUST_CAUCHY])
@pytest.mark.parametrize("kind", [fr.ICP, fr.PLANE_ICP, fr.GICP])
def test_factor_ref_matches_oracle_c1(orc, c1_f32, kind, robust):
    d = c1_f32
    otc, osc = d["otc"], d["osc"]
    st = orc.default_setting(factor_kind=kind, robust_kind=robust, robust_c=C, num_threads=4)
    for k, P in enumerate(POSES):
        T = pose(P)
        f = orc.Factors(len(osc))
        Ho, bo, eo, no = orc.linearize(otc, osc, st, T, f)
        ti, om = f.get()
        assert (ti >= 0).sum() == no > 1000
        s = fr.linearize(d["sp"], d["tp"], ti, T, kind, robust, C, d["sc"], d["tc"], d["tn"])
        assert s.inliers == no
        assert rel(s.H, Ho) <= 1e-12 and rel(s.b, bo) <= 1e-12 and abs(s.e - eo) <= 1e-12 * abs(eo), (k, rel(s.H, Ho), rel(s.b, bo), s.e, eo)
        assert np.array_equal(s.H, s.H.T)
        if kind == fr.GICP:  # the cached mahalanobis matrices are the oracle's
            ok = ti >= 0
            assert np.abs(s.maha[ok] - om[ok]).max() <= 1e-12 * np.abs(om[ok]).max()
        # the error at the linearization pose and at a trial pose: stale pairs, stale mahalanobis (gicp_factor.hpp:80-89)
        for Tq in (T, T @ se3([0.3, -1.0, 0.2], 0.4, [0.02, -0.01, 0.03])):
            eq = fr.error(d["sp"], d["tp"], ti, Tq, kind, robust, C, s.maha, d["tn"])
            eoq = orc.error(otc, osc, st, Tq, f)
            assert abs(eq - eoq) <= 1e-12 * abs(eoq), (k, eq, eoq)


@pytest.mark.parametrize("robust", [fr.ROBUST_NONE, fr.ROBUST_HUBER, fr.ROBUST_CAUCHY])
@pytest.mark.parametrize("kind", [fr.ICP, fr.PLANE_ICP, fr.GICP])
def test_per_pair_sums_to_linearize_c1(orc, c1_f32, kind, robust):
    """per_pair (the restatement the per-pair outputs of a pass are measured against) summed over its pairs is linearize — both float64,
    in another order — so the pins of linearize to the oracle above hold it too; its M is the matrix linearize caches."""
    d = c1_f32
    otc, osc = d["otc"], d["osc"]
    st = orc.default_setting(factor_kind=kind, robust_kind=robust, robust_c=C, num_threads=4)
    for k, P in enumerate(POSES):
        T = pose(P)
        f = orc.Factors(len(osc))
        orc.linearize(otc, osc, st, T, f)
        ti, _ = f.get()
        s = fr.linearize(d["sp"], d["tp"], ti, T, kind, robust, C, d["sc"], d["tc"], d["tn"])
        pp = fr.per_pair(d["sp"], d["tp"], ti, T, kind, robust, C, d["sc"], d["tc"], d["tn"])
        assert np.array_equal(pp.idx, np.flatnonzero(ti >= 0)) and len(pp.idx) == s.inliers > 1000
        assert pp.H.shape == (s.inliers, 6, 6) and pp.b.shape == (s.inliers, 6) and pp.e.shape == (s.inliers,) and pp.M.shape == (s.inliers, 3, 3)
        H = pp.H.sum(0)
        assert rel(H, s.H) <= 1e-13 and rel(pp.b.sum(0), s.b) <= 1e-13 and abs(pp.e.sum() - s.e) <= 1e-13 * abs(s.e), (k, rel(H, s.H), rel(pp.b.sum(0), s.b), pp.e.sum(), s.e)
        assert np.abs(pp.H - pp.H.transpose(0, 2, 1)).max() <= 1e-13 * np.abs(pp.H).max()
        if kind == fr.GICP:
            assert np.array_equal(pp.M, s.maha[pp.idx])
        # the magnitudes dominate what they bound, entry by entry
        assert (np.abs(pp.H) <= pp.Hmag * (1 + 1e-12)).all() and (np.abs(pp.b) <= pp.bmag * (1 + 1e-12)).all() and (pp.e >= 0).all()


def test_factor_ref_rejector_is_strict():
    """A pair exactly at max_dist_sq is kept (rejector.hpp:24: reject iff sq_dist > max_dist_sq); sq_dist is float64 from fp32 points."""
    tgt = np.zeros((1, 3), np.float32)
    src = np.array([[0.1, 0, 0], [0.0999999, 0, 0], [0.1000001, 0, 0]], np.float32)
    d2 = fr.sq_dist(src, tgt, np.zeros(3, np.int64), np.eye(4))
    assert d2[0] == np.float64(np.float32(0.1)) ** 2
    assert list(d2 <= np.float64(np.float32(0.1)) ** 2) == [True, True, False]

"""tests/search_ref.py — the float64 kNN and normal / covariance restatements test_search_matrix.py measures the GPU against — pinned to the
CPU oracle (the reference's kd-tree and normal estimation, in double) on config C1: kNN at several k from queries fp32 cannot hold, and
normals / covariances at k = 10 and 20 on every neighbourhood outside the tie band."""
import numpy as np
import pytest

import search_ref as sr


@pytest.fixture(scope="module")
def c1_target32(orc, c1_raw):
    return orc.voxelgrid_sampling(c1_raw[0], 0.25).astype(np.float32)


@pytest.mark.parametrize("k", [1, 5, 20, 64])
def test_knn_ref_matches_oracle_c1(orc, c1_target32, k):
    p = c1_target32
    rng = np.random.default_rng(k)
    q = p[rng.choice(len(p), 400, replace=False)].astype(np.float64) + rng.normal(scale=0.3, size=(400, 3))
    idx, d2, band, _ = sr.knn_ref(p, q, k)
    oi, od = orc.Cloud(p.astype(np.float64)).knn(q, k)
    assert band.sum() <= 4, band.sum()
    assert (idx[~band] == oi[~band]).all()
    assert np.abs(d2 - od).max() <= 4 * sr.EPS64 * od.max()
    # the threshold: kept iff d2 <= max_sq, the rest -1 / inf as a trailing run
    ms = float(np.median(d2[:, -1]))
    ti, td, _, _ = sr.knn_ref(p, q, k, ms)
    keep = d2 <= ms
    assert (ti == np.where(keep, idx, -1)).all() and (td == np.where(keep, d2, np.inf)).all()


def test_tie_band_flags_equidistant_rows():
    p = np.array([[1, 0, 0], [-1, 0, 0], [0, 3, 0]], np.float32)
    _, _, band, _ = sr.knn_ref(p, np.zeros((1, 3)), 1)
    assert band.all()
    _, _, band, _ = sr.knn_ref(p, np.array([[0.5, 0.0, 0.0]]), 1)
    assert not band.any()


@pytest.mark.parametrize("k", [10, 20])
def test_features_ref_matches_oracle_c1(orc, c1_target32, k):
    p = c1_target32
    ref = sr.features_ref(p, k)
    oc = orc.Cloud(p.astype(np.float64))
    oc.estimate_normals_covariances(k, 1)
    _, on, ocv = oc.get()
    good = ref["sep"] & ~ref["band"] & ~ref["sign_amb"]
    assert good.sum() >= 0.95 * len(p), (good.sum(), len(p))
    # a smallest eigenvector with relative gap g moves by ~ (covariance error) / g: the one-pass sums of the oracle, |p|^2 eps64 / lam2
    gap = (ref["lam"][:, 1] - ref["lam"][:, 0]) / ref["lam"][:, 2]
    tol = 1e-12 + 50 * ref["dev_err"] / gap
    dn = np.abs(on - ref["normals"]).max(axis=1)
    dc = np.abs(ocv - ref["covs"]).reshape(len(p), 9).max(axis=1)
    print("k=%d: %d of %d neighbourhoods compared; normals to %.1e, covariances to %.1e (largest bound %.1e)" % (k, good.sum(), len(p), dn[good].max(), dc[good].max(), tol[good].max()))
    assert (dn[good] <= tol[good]).all() and (dc[good] <= tol[good]).all()
    # the sign rule and the computeDirect restatement agree with the oracle where eigh's vector is not unique as well
    for i in np.flatnonzero(~ref["sep"] & ~ref["band"])[:20]:
        n0, C = sr.compute_direct(ref["cov"][i], p[i])
        assert np.abs(n0 - on[i]).max() < 1e-6 and np.abs(C - ocv[i]).max() < 1e-6


def test_features_ref_degenerate_neighbourhoods(orc):
    """Fewer than 5 points: zero normal, identity; all points equal: computeDirect's identity branch (normal -+e_x by the sign rule)."""
    few = sr.features_ref(np.zeros((4, 3), np.float32) + [1, 2, 3], 10)
    assert (few["normals"] == 0).all() and (few["covs"] == np.eye(3)).all()
    same = np.tile(np.array([[2.0, -1.0, 0.5]], np.float32), (6, 1))
    r = sr.features_ref(same, 6)
    assert (r["cov"] == 0).all()
    n0, C = sr.compute_direct(r["cov"][0], same[0])
    assert (n0 == [-1, 0, 0]).all() and (C == np.diag([1e-3, 1, 1])).all()
    oc = orc.Cloud(same.astype(np.float64))
    oc.estimate_normals_covariances(6, 1)
    _, on, ocv = oc.get()
    assert (on == n0).all() and (ocv == C).all()

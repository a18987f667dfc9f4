"""The standalone kd-tree kNN (csrc/problem.hip: knn_kernel, entry points sga_index_knn and sga_index_knn_f64) and normal / covariance
estimation (csrc/preprocess.hip: sga_estimate_normals_covariances) against the float64 restatements of tests/search_ref.py.

kNN: both entry points at every k class the LDS list sweeps (below, at and above each multiple of 4, up to the limit 116), target sizes
around k, the leaf and the batch, a deep tree, queries on points, near, far outside the box and not representable in fp32, through a plain
and a framed (shifted) index.  Then pairs placed at (1 +- delta) max_sq from queries fp32 cannot hold: the double entry point finds a pair
iff its double distance is <= max_sq, exactly.

Features: every route (one wave per query; one lane per query with the list in registers, k = 10 / 20, or in LDS, any k up to 112) at
k from 1 to 112 and sizes around k, on a random scene and on designed isolated clusters of exactly k points whose spectra are prescribed
(separated, a disk, line-like, collinear, all points equal), on both sides of the origin and 1e5 m away from it.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import search_ref as sr
import small_gicp_amd as sga
from conftest import ROOT

gpu = pytest.mark.gpu  # every test here but the last (a CPU check of the feature matrix's coverage)

KS = [1, 2, 3, 4, 5, 7, 8, 20, 21, 33, 64, 65, 100, 115, 116]
SHIFT = np.array([4.0e5, -3.0e5, 120.0])  # a framed index: the host moves the queries to its device frame (index_knn_impl)
WAVE_DEFAULT = 81920
EPS32, EPS64 = sr.EPS32, sr.EPS64
WORST = {}  # worst residual per assertion class, printed with -s


def note(key, v):
    WORST[key] = max(WORST.get(key, 0.0), float(v))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for k in sorted(WORST):
        print("worst %-32s %.3e" % (k, WORST[k]))


def knn32(tree, q32, k, max_sq=-1.0):
    """sga_index_knn: fp32 queries, fp32 distances, float(max_sq) against the float distance."""
    q = np.ascontiguousarray(q32, dtype=np.float32)
    idx = np.empty((len(q), k), np.int64)
    d2 = np.empty((len(q), k), np.float32)
    sga._lib.check(sga.load().sga_index_knn(tree.ctx.h, tree.h, q.ctypes.data_as(C.POINTER(C.c_float)), len(q), int(k), float(max_sq), idx.ctypes.data_as(C.POINTER(C.c_int64)), d2.ctypes.data_as(C.POINTER(C.c_float))))
    return idx, d2


def random_scene(n, seed, scale=20.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-scale, scale, size=(n, 3))).astype(np.float32)


def make_queries(p32, seed, m=192):
    """on points (d = 0), near points, far outside the box; doubles that fp32 cannot hold"""
    rng = np.random.default_rng(seed)
    n = len(p32)
    on = p32[rng.integers(0, n, m // 3)].astype(np.float64)
    near = p32[rng.integers(0, n, m // 3)].astype(np.float64) + rng.normal(scale=0.05, size=(m // 3, 3))
    lo, hi = p32.min(0).astype(np.float64), p32.max(0).astype(np.float64)
    far = hi + 50.0 + rng.uniform(0, 200, size=(m - 2 * (m // 3), 3))
    far[::2] = lo - 50.0 - rng.uniform(0, 200, size=(len(far[::2]), 3))
    q = np.concatenate([on, near, far])
    q[len(on):] += rng.uniform(-1, 1, size=q[len(on):].shape) * 1e-9  # off the fp32 grid
    return q


def framed(p32, shift):
    """(caller's double points, the device-frame records the cloud will hold, origin): the cloud chooses its origin from its box"""
    P = p32.astype(np.float64) + shift
    cloud = sga.PointCloud(P)
    o = cloud.origin()
    return cloud, (P - o).astype(np.float32), o


def check_rows(label, idx, d2, ref_idx, ref_d2, band, e, n, k, f64, unbounded):
    m = len(idx)
    found = idx >= 0
    # -1 / inf only as a trailing run; distances non-decreasing
    assert (found[:, :-1] >= found[:, 1:]).all(), (label, "hole in a row")
    assert (np.isinf(d2) == ~found).all(), label
    dd = np.where(found, d2, np.inf)
    assert (np.diff(dd, axis=1)[found[:, 1:]] >= 0).all(), (label, "row not ascending")
    if unbounded:
        assert (found.sum(1) == min(n, k)).all(), (label, found.sum(1), n, k)
    assert (found.sum(1) == (ref_idx >= 0).sum(1))[~band].all(), label
    ok = ~band
    assert (idx[ok] == ref_idx[ok]).all(), (label, np.flatnonzero((idx != ref_idx).any(1) & ok)[:5])
    fin = np.isfinite(ref_d2)
    if f64:  # double distances of the same records: a few ulps
        r = np.abs(d2[ok] - ref_d2[ok])[fin[ok]]
        tol = 8 * EPS64 * np.maximum(ref_d2[ok][fin[ok]], 1e-300) + 1e-300
        note("knn64 distance (ulps of d2)", (r / (2 * EPS64 * np.maximum(ref_d2[ok][fin[ok]], 1e-300))).max(initial=0))
        assert (r <= tol).all(), (label, r.max())
    else:  # the float distance from the rounded query: within delta of the double one
        B = sr.tie_bound(ref_d2, e[:, None]) / 2
        r = np.abs(d2.astype(np.float64) - ref_d2)[fin & ok[:, None]]
        note("knn32 distance / B", (r / B[fin & ok[:, None]]).max(initial=0))
        assert (r <= B[fin & ok[:, None]]).all(), label
    # inside the band: the distance multisets agree within B
    for i in np.flatnonzero(band):
        a, b = np.sort(d2[i][found[i]]), np.sort(ref_d2[i][ref_idx[i] >= 0])
        assert len(a) == len(b), (label, i)
        assert (np.abs(a - b) <= sr.tie_bound(b, e[i]) + 1e-300).all(), (label, i, a, b)
    note("knn band rows (fraction)", band.mean() if m else 0)


def sizes_for(k):
    return sorted({s for s in (1, 4, k - 1, k, k + 1, 63, 64, 65, 4097) if s >= 1})


@gpu
@pytest.mark.parametrize("k", KS)
def test_knn_matrix(k):
    for n in sizes_for(k) + [200_000]:
        p32 = random_scene(n, 1000 + n, scale=20.0 if n > 100 else 2.0)
        q = make_queries(p32, k * 7 + n, m=96 if n > 100_000 else 192)
        for shift in (None, SHIFT):
            if shift is None:
                cloud, rec, o = sga.PointCloud(p32), p32, np.zeros(3)
                qq = q
            else:
                cloud, rec, o = framed(p32, shift)
                qq = q + shift
            tree = sga.KdTree(cloud)
            label = "k=%d n=%d %s" % (k, n, "framed" if shift is not None else "plain")
            for max_sq in (-1.0, 0.5):
                ri, rd, band, e = sr.knn_ref(rec, qq, k, max_sq, origin=o)
                idx, d2 = tree.batch_knn_search(qq, k, max_sq_dist=max_sq)
                check_rows(label + " f64 max_sq=%g" % max_sq, idx, d2, ri, rd, band, e, n, k, True, max_sq < 0)
            # the fp32 entry point: queries fp32 holds in the caller's frame
            q32 = qq.astype(np.float32)
            ri, rd, band, e = sr.knn_ref(rec, q32.astype(np.float64), k, -1.0, origin=o)
            idx, d2 = knn32(tree, q32, k)
            check_rows(label + " f32", idx, d2, ri, rd, band, e, n, k, False, True)


@gpu
@pytest.mark.parametrize("k", [1, 20, 116])
def test_knn_deep_tree(k):
    n = 1_100_000
    p32 = random_scene(n, 77, scale=60.0)
    q = make_queries(p32, 78, m=96)
    tree = sga.KdTree(sga.PointCloud(p32))
    ri, rd, band, e = sr.knn_ref(p32, q, k)
    idx, d2 = tree.batch_knn_search(q, k)
    check_rows("deep k=%d" % k, idx, d2, ri, rd, band, e, n, k, True, True)


@gpu
def test_knn_k_limits():
    p32 = random_scene(500, 5)
    tree = sga.KdTree(sga.PointCloud(p32))
    q = p32[:4].astype(np.float64)
    for bad in (0, 117):
        with pytest.raises(sga.SgaError):
            tree.batch_knn_search(q, bad)
    vm = sga.IncrementalVoxelMap(1.0)
    vm.insert(sga.PointCloud(p32))
    idx, _ = vm.batch_knn_search(q, 128)
    assert idx.shape == (4, 128)
    with pytest.raises(sga.SgaError):
        vm.batch_knn_search(q, 129)


# ---- threshold edges ----------------------------------------------------------------------------------------------------------------
def edge_scene(R, max_sq, seed, dup=False):
    """Isolated targets at |p| >= R (~R unless the reach forces them apart) and one double query per target at d^2 = (1 + delta) max_sq: (targets fp32 (t, 3), queries (t, 3))."""
    rng = np.random.default_rng(seed)
    deltas = np.array([-1e-5, -1e-7, -1e-9, 1e-9, 1e-7, 1e-5])
    reps = 12
    t = len(deltas) * reps
    d = np.sqrt(max_sq) if max_sq > 0 else 0.0
    gap = max(10.0 * d, 1.0)
    # targets on a ring of radius R (|p| ~ R), spaced by more than 2 gap
    ang = np.arange(t) * max(2.5 * gap / R, 2 * np.pi / t)
    z = np.arange(t) // max(1, int(2 * np.pi * R / (2.5 * gap))) * 2.5 * gap
    g = 2.0**-20  # on a 2^-20 grid: fp32 holds the records, and records shifted by whole metres, exactly
    P = (np.round(np.stack([R * np.cos(ang), R * np.sin(ang), z], 1) / g) * g).astype(np.float32)
    u = rng.normal(size=(t, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dl = np.tile(deltas, reps)
    q = P.astype(np.float64) + u * (d * np.sqrt(1 + dl))[:, None]
    if dup:  # max_sq = 0: two copies of every target; every other query on it, the rest 1e-7 m off (fp32 may round them back onto it)
        q[1::2] += 1e-7
        P = np.concatenate([P, P])
    return P, q


@gpu
@pytest.mark.parametrize("R", [1.0, 40.0, 4000.0])
@pytest.mark.parametrize("max_sq", [0.0, 1e-4, 0.01, 1.0, 4.0])
def test_knn_threshold_is_double(R, max_sq):
    for shift in (None, SHIFT):
        P, q = edge_scene(R, max_sq, int(R) + int(1e4 * max_sq), dup=max_sq == 0.0)
        if shift is None:  # (an fp32 cloud far from the origin gets a device frame of its own as well: the records the index holds)
            cloud = sga.PointCloud(P)
            o = cloud.origin()
            rec = (P.astype(np.float64) - o).astype(np.float32)
        else:
            cloud, rec, o = framed(P, shift)
        if shift is not None:
            # the same offsets from the records the index holds, on the caller's double grid near 4e5 m (2^-34 m): q - o is then exact
            # in double (the host's shift).  That grid moves d2 by up to ~2 d 2^-34 sqrt(3): at max_sq <= 0.01 more than the designed
            # 1e-9 max_sq, so there the framed cells are pairs near the threshold rather than at a prescribed offset; the verdict is
            # still checked exactly against knn_ref on the queries as sent.
            g = 2.0**-34
            qd = np.round((rec[: len(q)].astype(np.float64) + (q - P[: len(q)].astype(np.float64))) / g) * g
            q = o + qd
        tree = sga.KdTree(cloud)
        k = 2 if max_sq == 0.0 else 1
        ri, rd, _, _ = sr.knn_ref(rec, q, k, max_sq, origin=o)
        idx, d2 = tree.batch_knn_search(q, k, max_sq_dist=max_sq)
        want = ri[:, 0] >= 0
        got = idx[:, 0] >= 0
        assert 0 < want.sum() < len(q) or max_sq == 0.0
        assert (got == want).all(), (R, max_sq, shift, np.flatnonzero(got != want)[:8], (rd[:, 0] / max(max_sq, 1e-300) - 1)[got != want][:8])
        # (max_sq = 0: the two copies of a target tie at d2 = 0; the kernel orders them by kd position, knn_ref by index: a set)
        assert (np.sort(idx[want], 1) == np.sort(ri[want], 1)).all()
        r = np.abs(d2[want, 0] - rd[want, 0]) / (2 * EPS64 * max(max_sq, 1e-300))
        note("threshold d64 (ulps of max_sq)", r.max(initial=0))
        assert r.max(initial=0) <= 4, (R, max_sq, shift, r.max())
        if max_sq == 0.0:  # exact duplicates: both copies at distance 0, nothing for the queries off them
            assert want[::2].all() and not want[1::2].any()
            assert (idx[want] >= 0).all() and (d2[want] == 0).all()


# ---- features -----------------------------------------------------------------------------------------------------------------------
FEAT_KS = [1, 4, 5, 6, 10, 11, 20, 21, 33, 64, 65, 100, 112]


def route_of(n, k, wave_max):
    """preprocess.hip: sga_estimate_normals_covariances's dispatch, restated"""
    if n <= wave_max and k <= 64:
        return "wave"
    return {10: "K10", 20: "K20"}.get(k, "K0")


def k_class(k):
    return "k<5" if k < 5 else ("k<=64" if k <= 64 else "k>64")


def estimate(pts, k, wave, flags=3, tree=False, normals=None, covs=None):
    lib = sga.load()
    lib.sga_set_knn_wave_max(1 << 40 if wave else 0)
    try:
        c = sga.PointCloud(pts, normals=normals, covs=covs)
        t = sga.KdTree(c) if tree else None
        sga.api._estimate(c, t, k, flags)
        return (c, t) if tree else c
    finally:
        lib.sga_set_knn_wave_max(WAVE_DEFAULT)


def feat_tol(ref):
    """fp32 output rounding (a few ulps of unit-size entries) plus the conditioning of the smallest eigenvector: (the device's one-pass
    covariance error + computeDirect's, relative to lam2) / the relative gap lam1 - lam0"""
    lam = ref["lam"]
    gap = np.maximum((lam[:, 1] - lam[:, 0]) / np.maximum(lam[:, 2], 1e-300), 1e-300)
    return 4 * EPS32 + 16 * (ref["dev_err"] + 64 * EPS64) / gap


def check_features(label, c, ref, origin=None):
    nrm, cov = c.normals()[:, :3], c.covs()[:, :3, :3]
    n = len(nrm)
    few = ref["found"] < 5
    assert (nrm[few] == 0).all() and (cov[few] == np.eye(3)).all(), label
    good = ~few & ref["sep"] & ~ref["band"] & ~ref["sign_amb"]
    tol = feat_tol(ref)
    dn = np.abs(nrm - ref["normals"]).max(1)
    dc = np.abs(cov - ref["covs"]).reshape(n, 9).max(1)
    if good.any():
        note("feature normal / 4eps32", (dn[good] / (4 * EPS32)).max())
        note("feature C / 4eps32", (dc[good] / (4 * EPS32)).max())
        assert (dn[good] <= tol[good]).all(), (label, np.flatnonzero(dn > tol)[:5], dn[good].max())
        assert (dc[good] <= tol[good]).all(), (label, dc[good].max())
    # every neighbourhood: a unit normal, C = I - (1 - 1e-3) n n^T, exactly symmetric
    some = ~few
    assert np.abs(np.linalg.norm(nrm[some], axis=1) - 1).max(initial=0) < 1e-6, label
    cn = np.eye(3) - (1 - 1e-3) * np.einsum("ri,rj->rij", nrm[some], nrm[some])
    note("feature C vs I-(1-1e-3)nn^T", np.abs(cov[some] - cn).max(initial=0))
    assert np.abs(cov[some] - cn).max(initial=0) < 2e-6, label
    assert (cov == np.swapaxes(cov, 1, 2)).all(), label
    return nrm, cov


@gpu
@pytest.mark.parametrize("k", FEAT_KS)
@pytest.mark.parametrize("wave", [True, False])
def test_features_random_scene(k, wave):
    for n in sorted({s for s in (1, 4, 5, k - 1, k, k + 1, 64, 65, 4097) if s >= 1}):
        p32 = random_scene(n, 3 * n + k, scale=3.0 if n < 100 else 12.0)
        c = estimate(p32, k, wave)
        check_features("k=%d n=%d wave=%s" % (k, n, wave), c, sr.features_ref(p32, k))


def cluster(kind, k, rng):
    """k points around 0 with a prescribed spectrum: (points (k, 3) float64 offsets, the defined direction(s) of the normal)"""
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if kind == "separated":
        s = rng.normal(size=(k, 3))
        s -= s.mean(0)
        # whiten, then scale: the spectrum is exactly (0.01, 0.09, 0.25) up to the rounding of the points
        L = np.linalg.cholesky(s.T @ s / k)
        s = np.linalg.solve(L, s.T).T * [0.5, 0.3, 0.1]
        return s @ R.T, ("normal", R[:, 2])
    if kind == "disk":  # a ring: lam1 = lam2, lam0 = 0; the normal is the plane's
        a = 2 * np.pi * np.arange(k) / k
        s = np.stack([0.5 * np.cos(a), 0.5 * np.sin(a), np.zeros(k)], 1)
        return s @ R.T, ("normal", R[:, 2])
    if kind == "line":  # lam0 ~ lam1 << lam2: the normal is any direction orthogonal to the line
        s = rng.normal(size=(k, 3)) * [0.5, 1e-3, 1e-3]
        return s @ R.T, ("orth", R[:, 0])
    if kind == "collinear":  # exactly on the x axis
        s = np.zeros((k, 3))
        s[:, 0] = np.linspace(-0.5, 0.5, k)
        return s, ("orth", np.array([1.0, 0, 0]))
    return np.zeros((k, 3)), ("identity", None)  # all points equal


CLUSTER_KINDS = ["separated", "disk", "line", "collinear", "equal"]


@gpu
@pytest.mark.parametrize("k,wave", [(k, w) for k in (5, 6, 10, 20, 33, 64, 65, 112) for w in (True, False) if w is False or k <= 64])  # k > 64: no wave route
@pytest.mark.parametrize("far", [False, True])
def test_features_designed_clusters(k, wave, far):
    """Isolated clusters of exactly k points, 40 m apart: each point's k neighbours are its cluster.  Centres on both sides of the
    origin; far = the whole scene ~1e5 m away (a framed cloud: the sign rule must use the caller's frame)."""
    rng = np.random.default_rng(k + 1000 * far)
    blocks, meta = [], []
    spots = [np.array([sx * 40.0 * (j + 1), sy * 40.0, 15.0 * j]) for j in range(3) for sx in (-1, 1) for sy in (-1, 1)]
    ci = 0
    for kind in CLUSTER_KINDS:
        for _ in range(2):
            off, what = cluster(kind, k, rng)
            ctr = spots[ci % len(spots)] + [0, 0, 300.0 * (ci // len(spots))]
            ci += 1
            blocks.append(ctr + off)
            meta += [(kind, what)] * k
    P = np.concatenate(blocks)
    shift = np.array([1.0e5, -1.0e5, 20.0]) if far else np.zeros(3)
    if far:
        cl = sga.PointCloud(P + shift)
        o = cl.origin()
        rec = (P + shift - o).astype(np.float32)
    else:
        o = np.zeros(3)
        rec = P.astype(np.float32)
    lib = sga.load()
    lib.sga_set_knn_wave_max(1 << 40 if wave else 0)
    try:
        cl = sga.PointCloud(rec.astype(np.float64) + o if far else rec)
        assert (cl.origin() == o).all()
        sga.api._estimate(cl, None, k, 3)
    finally:
        lib.sga_set_knn_wave_max(WAVE_DEFAULT)
    ref = sr.features_ref(rec, k, origin=o)
    assert (ref["found"] == k).all() and not ref["band"][np.array([m[0] != "equal" for m in meta])].any()
    nrm, cov = check_features("clusters k=%d wave=%s far=%s" % (k, wave, far), cl, ref, o)
    caller = rec.astype(np.float64) + o
    for i, (kind, (what, v)) in enumerate(meta):
        if what == "normal":  # the defined normal, turned away from the caller's origin
            sgn = -1.0 if np.dot(caller[i], v) > 0 else 1.0
            note("cluster normal (%s)" % kind, np.abs(nrm[i] - sgn * v).max())
            assert np.abs(nrm[i] - sgn * v).max() < 2e-5, (kind, i, nrm[i], sgn * v)
        elif what == "orth":  # orthogonal to the sample's own line (the top eigenvector, well separated)
            v = np.linalg.eigh(ref["cov"][i])[1][:, 2]
            note("cluster |n . dir| (%s)" % kind, abs(np.dot(nrm[i], v)))
            assert abs(np.dot(nrm[i], v)) < 1e-5, (kind, i, nrm[i], v)
        else:  # zero covariance: computeDirect's identity branch, normal -+e_x by the sign rule, C = diag(1e-3, 1, 1)
            ex = np.array([-1.0, 0, 0]) if caller[i, 0] > 0 else np.array([1.0, 0, 0])
            assert (nrm[i] == ex).all() and (cov[i] == np.diag([1e-3, 1.0, 1.0]).astype(np.float32)).all(), (i, nrm[i], cov[i])


@gpu
@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("wave", [True, False])
def test_features_flags_keep_the_other_attribute(flags, wave):
    p32 = random_scene(3000, 11, scale=10.0)
    rng = np.random.default_rng(12)
    n0 = rng.normal(size=(3000, 3)).astype(np.float32)
    c60 = rng.normal(size=(3000, 6)).astype(np.float32)
    c, tree = estimate(p32, 20, wave, flags=flags, tree=True, normals=n0, covs=c60)
    ref = sr.features_ref(p32, 20)
    nrm, cov = c.normals()[:, :3], c.covs()[:, :3, :3]
    if flags & 1:
        good = ref["sep"] & ~ref["band"] & ~ref["sign_amb"]
        assert (np.abs(nrm - ref["normals"]).max(1)[good] <= feat_tol(ref)[good]).all()
    else:
        assert (nrm == n0).all()
    if flags & 2:
        good = ref["sep"] & ~ref["band"] & ~ref["sign_amb"]
        assert (np.abs(cov - ref["covs"]).reshape(-1, 9).max(1)[good] <= feat_tol(ref)[good]).all()
    else:
        assert (cov == sga.api.mats_from_sym6(c60.astype(np.float64))).all()
    # the index's kd-ordered copies, written by the kernel, equal the cloud's: a pass that reads them (PLANE_ICP: target normals, GICP:
    # target covariances) gives bit for bit the same system before and after refresh_attributes() pulls the cloud's into the index
    src = sga.PointCloud(p32[::3] + np.float32(0.02), covs=np.tile(np.eye(3) * 1e-2, (len(p32[::3]), 1, 1)))
    T = np.eye(4)
    T[:3, 3] = [0.01, -0.02, 0.015]
    kinds = [k for f, k in ((1, "PLANE_ICP"), (2, "GICP")) if flags & f]

    def systems():
        return [sga.Problem(tree, src).linearize(sga.make_setting(kind, max_correspondence_distance=1.0).factor, T) for kind in kinds]

    before = systems()
    tree.refresh_attributes()
    after = systems()
    for kind, (H0, b0, e0, n0_), (H1, b1, e1, n1) in zip(kinds, before, after):
        assert n0_ == n1 > 0 and (H0 == H1).all() and (b0 == b1).all() and e0 == e1, kind


@gpu
def test_features_default_knob_large_cloud():
    """~90k points at the default knob: above SGA_KNN_WAVE_MAX, the one-lane-per-query kernels"""
    p32 = random_scene(90_000, 21, scale=30.0)
    for k in (10, 20, 21):
        c = sga.PointCloud(p32)
        sga.api._estimate(c, None, k, 3)
        check_features("90k k=%d" % k, c, sr.features_ref(p32, k))


@gpu
def test_features_k_limit():
    c = sga.PointCloud(random_scene(200, 3))
    sga.api._estimate(c, None, 112, 3)
    for bad in (0, 113):
        with pytest.raises(sga.SgaError):
            sga.api._estimate(c, None, bad, 3)


def test_feature_matrix_covers_every_route_and_k_class():
    """(CPU) every (route, k class) cell the dispatch can reach has a case above, and the dispatch is still the one restated here"""
    src = open(os.path.join(ROOT, "small_gicp_amd", "csrc", "preprocess.hip")).read()
    assert "n <= static_cast<size_t>(g_knn_wave_max) && k <= 64" in src
    assert re.search(r"else if \(k == 20\)\s*hipLaunchKernelGGL\(\(local_features_kernel<20>\)", src)
    assert re.search(r"else if \(k == 10\)\s*hipLaunchKernelGGL\(\(local_features_kernel<10>\)", src)
    cells = set()
    for k in FEAT_KS:
        for wave in (True, False):
            for n in (1, 4, 5, k - 1, k, k + 1, 64, 65, 4097):
                if n >= 1:
                    cells.add((route_of(n, k, (1 << 40) if wave else 0), k_class(k)))
    for k in (10, 20, 21):
        cells.add((route_of(90_000, k, WAVE_DEFAULT), k_class(k)))
    want = {("wave", "k<5"), ("wave", "k<=64"), ("K10", "k<=64"), ("K20", "k<=64"), ("K0", "k<5"), ("K0", "k<=64"), ("K0", "k>64")}
    assert want <= cells, want - cells
    assert max(FEAT_KS) == 112 and 64 in FEAT_KS and 65 in FEAT_KS

"""Flat voxel maps of every kind of contents (IncrementalVoxelMap<FlatContainer<HasNormals, HasCovs>>, ann/flat_container.hpp:18-58) and
point-to-plane ICP against the maps that keep normals.

The oracle has only the covariance flat map.  Its points and correspondences are the same for every kind of contents; the point-to-plane
algebra is checked against a numpy restatement of plane_icp_factor.hpp:35-73 (+ robust_kernel.hpp:68-90), itself pinned to the oracle
over a kd-tree target by the first (CPU) test."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, pose_error

POSE_TOL_T, POSE_TOL_R = 1e-4, 1e-4


def rot(axis, ang):
    a = np.asarray(axis, dtype=np.float64)
    k = a / np.linalg.norm(a)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K


def se3(axis, ang, t):
    T = np.eye(4)
    T[:3, :3] = rot(axis, ang)
    T[:3, 3] = t
    return T


def skew(p):
    z = np.zeros(len(p))
    return np.stack([np.stack([z, -p[:, 2], p[:, 1]], -1), np.stack([p[:, 2], z, -p[:, 0]], -1), np.stack([-p[:, 1], p[:, 0], z], -1)], 1)


def robust_weight(kind, c, e):
    s = np.sqrt(e)
    if kind == "HUBER":
        return np.where(s < c, 1.0, c / np.where(s > 0, s, 1.0))
    if kind == "CAUCHY":
        return c / (c + s * s)
    return np.ones_like(e)


def plane_terms(src, tgt, nrm, T, robust=None, c=1.0):
    """plane_icp_factor.hpp:35-73 per pair (src[i] matched with tgt[i], normal nrm[i]), robustified like RobustFactor: H (m,6,6), b (m,6), e (m,)."""
    R, t = T[:3, :3], T[:3, 3]
    q = src @ R.T + t
    err = nrm * (tgt - q)
    J = np.zeros((len(src), 3, 6))
    J[:, :, :3] = nrm[:, :, None] * (R[None] @ skew(src))
    J[:, :, 3:] = -nrm[:, :, None] * R[None]
    H = np.einsum("mki,mkj->mij", J, J)
    b = np.einsum("mki,mk->mi", J, err)
    e = 0.5 * (err * err).sum(1)
    w = robust_weight(robust, c, e)
    return H * w[:, None, None], b * w[:, None], e * w


def plane_error(src, tgt, nrm, T, robust=None, c=1.0):
    R, t = T[:3, :3], T[:3, 3]
    err = nrm * (tgt - (src @ R.T + t))
    e = 0.5 * (err * err).sum(1)
    return float((robust_weight(robust, c, e) * e).sum())


def plane_sums(src, tgt, nrm, T, robust=None, c=1.0):
    H, b, e = plane_terms(src, tgt, nrm, T, robust, c)
    return H.sum(0), b.sum(0), float(e.sum())


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


ROBUST = [(None, 1.0), ("HUBER", 0.05), ("CAUCHY", 0.05)]
ROBUST_KIND = {None: 0, "HUBER": 1, "CAUCHY": 2}


# ---- 1. the restatement, pinned to the oracle (CPU) -------------------------------------------------------------------------------
@pytest.mark.parametrize("robust,c", ROBUST)
def test_plane_restatement_matches_oracle(orc, c1_oracle_clouds, robust, c):
    tc, sc = c1_oracle_clouds
    tp, tn, _ = tc.get()
    sp, _, _ = sc.get()
    T = se3([0.1, 0.2, 1.0], np.deg2rad(0.7), [0.49, 0.12, -0.02])
    st = orc.default_setting(factor_kind=orc.PLANE_ICP, robust_kind=ROBUST_KIND[robust], robust_c=c, num_threads=1)
    f = orc.Factors(len(sp))
    Ho, bo, eo, no = orc.linearize(tc, sc, st, T, f)
    ti = f.get()[0]
    ok = ti >= 0
    assert ok.sum() == no > 1000
    H, b, e = plane_sums(sp[ok], tp[ti[ok]], tn[ti[ok]], T, robust, c)
    assert rel(H, Ho) <= 1e-12 and rel(b, bo) <= 1e-12 and abs(e - eo) <= 1e-12 * abs(eo), (rel(H, Ho), rel(b, bo), e, eo)
    T2 = se3([1, -1, 0.3], np.deg2rad(0.3), [0.45, 0.1, 0.0])
    e2 = orc.error(tc, sc, st, T2, f)
    assert abs(plane_error(sp[ok], tp[ti[ok]], tn[ti[ok]], T2, robust, c) - e2) <= 1e-12 * abs(e2)


# ---- surfaces without a device ------------------------------------------------------------------------------------------------------
def test_drop_in_module_exposes_the_four_flat_maps():
    import small_gicp

    for name in ("IncrementalVoxelMap", "IncrementalVoxelMapNormal", "IncrementalVoxelMapCov", "IncrementalVoxelMapNormalCov"):
        cls = getattr(small_gicp, name)
        assert name in small_gicp.__all__
        for m in ("insert", "set_lru", "size", "__len__", "voxel_points", "set_setting", "set_search_offsets", "knn_search", "batch_knn_search", "download", "from_voxels"):
            assert hasattr(cls, m), (name, m)
        assert hasattr(cls, "voxel_normals") == ("Normal" in name), name
        assert hasattr(cls, "voxel_covs") == ("Cov" in name), name


def test_new_entry_points_are_declared():
    from small_gicp_amd._lib import FLAT_COVS, FLAT_NORMALS, SYMBOLS

    names = {s[0] for s in SYMBOLS}
    for n in ("sga_flatmap_create_contents", "sga_flatmap_get_contents", "sga_flatmap_download_contents", "sga_index_create_flatmap_from_voxels_contents"):
        assert n in names
    hdr = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    assert "SGA_FLAT_NORMALS = %d" % FLAT_NORMALS in hdr and "SGA_FLAT_COVS = %d" % FLAT_COVS in hdr


def test_odometry_refuses_plane_icp_without_a_flat_model():
    from small_gicp_amd.odometry import ModelOdometry

    with pytest.raises(ValueError):
        ModelOdometry(model="gaussian", factor="PLANE_ICP")
    with pytest.raises(ValueError):
        ModelOdometry(model="flat", factor="VGICP")


# ---- device tests ---------------------------------------------------------------------------------------------------------------------
KINDS = ["IncrementalVoxelMap", "IncrementalVoxelMapNormal", "IncrementalVoxelMapCov", "IncrementalVoxelMapNormalCov"]


def _clouds_for(sga, d, prefix, kind):
    """the device cloud with exactly the attributes a kind needs"""
    p, n, c = d[prefix + "p"], d[prefix + "n"], d[prefix + "c"]
    return sga.PointCloud(p, n if "Normal" in kind else None, c if "Cov" in kind else None)


def _poses():
    return [se3([0.1, 0.2, 1.0], 0.02 * step, [5.0 * step, -2.0 * step, 0.1 * step]) for step in range(7)]


def _build(sga, d, kind, offsets):
    m = getattr(sga, kind)(1.0)
    m.set_lru(2, 3)
    m.set_search_offsets(offsets)
    clouds = [_clouds_for(sga, d, "t", kind), _clouds_for(sga, d, "s", kind)]
    for step, T in enumerate(_poses()):
        m.insert(clouds[step % 2], T)
    return m


def _orc_map(orc, d, offsets):
    ot, os_ = orc.Cloud(d["tp"], d["tn"], d["tc"]), orc.Cloud(d["sp"], d["sn"], d["sc"])
    ov = orc.FlatMap(1.0)
    ov.set_lru(2, 3)
    ov.set_search_offsets(offsets)
    for step, T in enumerate(_poses()):
        ov.insert(ot if step % 2 == 0 else os_, T)
    return ov, os_


def _slot_rows(idx, counts):
    """(voxel << 32) | point -> row of the voxel-major point list (download / orc get); -1 stays -1"""
    offs = np.concatenate([[0], np.cumsum(counts.astype(np.int64))[:-1]])
    out = np.full(len(idx), -1, np.int64)
    ok = idx >= 0
    out[ok] = offs[idx[ok] >> 32] + (idx[ok] & 0xFFFFFFFF)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [1, 7, 27])
def test_insert_parity_every_kind(orc, c1_f32, offsets):
    import small_gicp_amd as sga
    from scipy.spatial import cKDTree

    d = c1_f32
    ov, _ = _orc_map(orc, d, offsets)
    oc, on, op, ocv = ov.get()
    maps = {k: _build(sga, d, k, offsets) for k in KINDS}
    scale = max(1.0, float(np.abs(op).max()))
    ref_pts = None
    for k, m in maps.items():
        got = m.download()
        gc, gn, gp = got[:3]
        assert len(m) == len(ov) and (gc == oc).all() and (gn == on).all(), k
        assert np.abs(gp - op).max() <= 2e-7 * scale, k
        if ref_pts is None:
            ref_pts = gp
        assert (gp == ref_pts).all(), k  # the accept / reject rule reads the points alone
        assert m.voxel_points().shape == (len(gp), 4)
    g6 = maps["IncrementalVoxelMapNormalCov"].download()[4]
    assert np.abs(sga.api.mats_from_sym6(g6.astype(np.float64)) - ocv).max() <= 2e-7
    assert (g6 == maps["IncrementalVoxelMapCov"].download()[3]).all()
    # normals: R n of the source point each slot kept, found by position among everything inserted
    cand_p, cand_n = [], []
    for step, T in enumerate(_poses()):
        pfx = "t" if step % 2 == 0 else "s"
        p, n = d[pfx + "p"].astype(np.float64), d[pfx + "n"].astype(np.float64)
        cand_p.append(p @ T[:3, :3].T + T[:3, 3])
        cand_n.append(n @ T[:3, :3].T)
    cand_p, cand_n = np.concatenate(cand_p), np.concatenate(cand_n)
    dist, j = cKDTree(cand_p).query(ref_pts.astype(np.float64))
    assert dist.max() <= 2e-7 * scale * 4
    for k in ("IncrementalVoxelMapNormal", "IncrementalVoxelMapNormalCov"):
        vn = maps[k].voxel_normals()
        assert vn.shape == (len(ref_pts), 4) and (vn[:, 3] == 0).all()
        assert np.abs(vn[:, :3] - cand_n[j]).max() <= 2e-7, k
    assert (maps["IncrementalVoxelMapNormal"].download()[3] == maps["IncrementalVoxelMapNormalCov"].download()[3]).all()


@pytest.mark.gpu
def test_insert_argument_checks(c1_f32):
    import small_gicp_amd as sga

    d = c1_f32
    bare = sga.PointCloud(d["tp"])
    pts_map = sga.IncrementalVoxelMap(1.0)
    pts_map.insert(bare)  # neither normals nor covariances needed
    assert len(pts_map) > 0 and len(pts_map.download()) == 3
    for kind, cloud in (("IncrementalVoxelMapNormal", sga.PointCloud(d["tp"], None, d["tc"])), ("IncrementalVoxelMapNormalCov", sga.PointCloud(d["tp"], d["tn"], None)),
                        ("IncrementalVoxelMapCov", sga.PointCloud(d["tp"], d["tn"], None))):
        with pytest.raises(sga.SgaError, match="error 1: .*(normals|covariances)"):  # SGA_ERR_INVALID
            getattr(sga, kind)(1.0).insert(cloud)
    lib = sga._lib.load()
    import ctypes as C

    h = C.c_void_p()
    assert lib.sga_flatmap_create_contents(sga.default_context().h, 1.0, 4, C.byref(h)) == 1  # SGA_ERR_INVALID
    contents = C.c_int()
    for kind, want in zip(KINDS, (0, 1, 2, 3)):
        m = getattr(sga, kind)(1.0)
        assert lib.sga_flatmap_get_contents(m.h, C.byref(contents)) == 0 and contents.value == want
    # a download of what a map does not keep is refused
    nrm = np.empty((len(pts_map), 16, 3), np.float32)
    assert lib.sga_flatmap_download_contents(sga.default_context().h, pts_map.h, None, None, None, sga.api._fp(nrm), None) == 1


def _fixed_T():
    return se3([0.1, 0.2, 1.0], 0.02 * 6 + 0.004, [30.0 + 0.1, -12.0 - 0.05, 0.6])


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [1, 7, 27])
@pytest.mark.parametrize("mode", ["fp32", "fp64"])
@pytest.mark.parametrize("robust,c", ROBUST)
def test_plane_linearize_over_normal_map(orc, c1_f32, offsets, mode, robust, c):
    import small_gicp_amd as sga

    d = c1_f32
    nm = _build(sga, d, "IncrementalVoxelMapNormal", offsets)
    src = sga.PointCloud(d["sp"])
    T0 = _fixed_T()
    st = sga.make_setting("PLANE_ICP", robust_kernel=robust, robust_c=c, math_mode=mode)
    pb = sga.Problem(nm, src, T0)
    H, b, e, n = pb.linearize(st.factor, T0)
    gi = pb.factors()[0]
    # correspondences: the oracle's search over the same inserts
    ov, os_ = _orc_map(orc, d, offsets)
    fac = orc.Factors(len(d["sp"]))
    orc.linearize(ov, os_, orc.default_setting(factor_kind=orc.ICP, num_threads=1), T0, fac)
    oi = fac.get(2)[0]
    assert (gi == oi).mean() > 0.999 and n > 1000
    # H, b, e over the map's own fp32 records
    coords, counts, mp, mn = nm.download()
    rows = _slot_rows(gi, counts)
    ok = rows >= 0
    assert ok.sum() == n
    sp = d["sp"].astype(np.float64)
    Hn, bn, en = plane_sums(sp[ok], mp[rows[ok]].astype(np.float64), mn[rows[ok]].astype(np.float64), T0, robust, c)
    tol = 1e-9 if mode == "fp64" else 1e-5
    assert rel(H, Hn) <= tol and rel(b, bn) <= tol and abs(e - en) <= tol * abs(en), (rel(H, Hn), rel(b, bn), e, en)
    # against the oracle's doubles and correspondences
    _, ocnt, opts, _ = ov.get()
    orows = _slot_rows(oi, ocnt)
    ook = orows >= 0
    Ho, bo, eo = plane_sums(sp[ook], opts[orows[ook]], mn[orows[ook]].astype(np.float64), T0, robust, c)
    assert rel(H, Ho) <= 1e-4 and rel(b, bo) <= 1e-4 and abs(e - eo) <= 1e-4 * abs(eo)
    # error() over the stale correspondences at three trial poses
    for k, dT in enumerate([se3([0, 0, 1], 1e-3, [0.01, 0, 0]), se3([1, 0, 0], -2e-3, [0, -0.02, 0.01]), se3([0.3, 1, 0], 5e-3, [0.05, 0.02, -0.03])]):
        Tk = T0 @ dT
        ek = pb.error(st.factor, Tk)
        en_k = plane_error(sp[ok], mp[rows[ok]].astype(np.float64), mn[rows[ok]].astype(np.float64), Tk, robust, c)
        assert abs(ek - en_k) <= tol * abs(en_k), (k, ek, en_k)
    # per-point systems sum to the linearization (the export runs in fp64)
    inl, Hp, bp, ep = pb.linearize_per_point(st.factor, T0)
    H64, b64, e64, n64 = pb.linearize(sga.make_setting("PLANE_ICP", robust_kernel=robust, robust_c=c, math_mode="fp64").factor, T0)
    assert inl.sum() == n64 and rel(Hp.sum(0), H64) <= 1e-9 and rel(bp.sum(0), b64) <= 1e-9 and abs(ep.sum() - e64) <= 1e-9 * abs(e64)
    Hq, bq, eq = plane_terms(sp[inl], mp[_slot_rows(pb.factors()[0], counts)[inl]].astype(np.float64), mn[_slot_rows(pb.factors()[0], counts)[inl]].astype(np.float64), T0, robust, c)
    assert rel(Hp[inl], Hq) <= 1e-9 and rel(bp[inl], bq) <= 1e-9


def _host_plane_lm(sga, orc, ov, os_, sp, normals, setting, T0, robust=None, c=1.0):
    """sga_optimize over numpy callbacks: the restatement over the oracle's search; error() reuses the correspondences of the last linearize."""
    _, cnt, opts, _ = ov.get()
    state = {}

    def lin(T):
        fac = orc.Factors(len(sp))
        orc.linearize(ov, os_, orc.default_setting(factor_kind=orc.ICP, max_dist_sq=setting.factor.max_dist_sq, num_threads=1), T, fac)
        rows = _slot_rows(fac.get(2)[0], cnt)
        ok = rows >= 0
        state["ok"], state["rows"] = ok, rows[ok]
        H, b, e = plane_sums(sp[ok], opts[rows[ok]], normals[rows[ok]], T, robust, c)
        return H, b, e, int(ok.sum())

    def err(T):
        return plane_error(sp[state["ok"]], opts[state["rows"]], normals[state["rows"]], T, robust, c)

    return sga.optimize(setting, T0, lin, err)


@pytest.mark.gpu
def test_plane_align_over_normal_map_matches_host_lm(orc, c1_f32):
    import small_gicp_amd as sga

    d = c1_f32
    nm = _build(sga, d, "IncrementalVoxelMapNormal", 7)
    ov, os_ = _orc_map(orc, d, 7)
    src = sga.PointCloud(d["sp"])
    T0 = _fixed_T()
    st = sga.make_setting("PLANE_ICP")
    res = sga.Problem(nm, src, T0).align(st, T0)
    nrm = nm.download()[3].astype(np.float64)
    ref = _host_plane_lm(sga, orc, ov, os_, d["sp"].astype(np.float64), nrm, st, T0)
    dt, dr = pose_error(res.T_target_source, ref.T_target_source)
    assert res.iterations == ref.iterations and dt < POSE_TOL_T and dr < POSE_TOL_R, (res.iterations, ref.iterations, dt, dr)
    assert res.converged and abs(int(res.num_inliers) - int(ref.num_inliers)) <= 2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "fp64"])
def test_same_points_same_answers(c1_f32, mode):
    import small_gicp_amd as sga

    d = c1_f32
    src_c = sga.PointCloud(d["sp"], None, d["sc"])
    T0 = _fixed_T()
    cov = _build(sga, d, "IncrementalVoxelMapCov", 7)
    nc = _build(sga, d, "IncrementalVoxelMapNormalCov", 7)
    pts = _build(sga, d, "IncrementalVoxelMap", 7)
    g = sga.make_setting("GICP", math_mode=mode)
    a, b = sga.Problem(cov, src_c, T0), sga.Problem(nc, src_c, T0)
    ra, rb = a.linearize(g.factor, T0), b.linearize(g.factor, T0)
    assert (ra[0] == rb[0]).all() and (ra[1] == rb[1]).all() and ra[2] == rb[2] and ra[3] == rb[3]
    assert (a.factors()[0] == b.factors()[0]).all()
    assert (a.align(g, T0).T_target_source == b.align(g, T0).T_target_source).all()
    i = sga.make_setting("ICP", math_mode=mode)
    pa, pp = sga.Problem(cov, src_c, T0), sga.Problem(pts, sga.PointCloud(d["sp"]), T0)
    ra, rp = pa.linearize(i.factor, T0), pp.linearize(i.factor, T0)
    assert (ra[0] == rp[0]).all() and (ra[1] == rp[1]).all() and ra[2] == rp[2] and ra[3] == rp[3]
    assert (pa.align(i, T0).T_target_source == pp.align(i, T0).T_target_source).all()
    # a map rebuilt from its download: bit-identical point-to-plane linearize
    nm = _build(sga, d, "IncrementalVoxelMapNormal", 7)
    coords, counts, mp, mn = nm.download()
    rb_map = sga.IncrementalVoxelMapNormal.from_voxels(1.0, coords, counts, mp, search_offsets=7, normals=mn)
    pl = sga.make_setting("PLANE_ICP", math_mode=mode)
    src = sga.PointCloud(d["sp"])
    p1, p2 = sga.Problem(nm, src, T0), sga.Problem(rb_map, src, T0)
    r1, r2 = p1.linearize(pl.factor, T0), p2.linearize(pl.factor, T0)
    assert r1[3] > 1000 and (r1[0] == r2[0]).all() and (r1[1] == r2[1]).all() and r1[2] == r2[2] and r1[3] == r2[3]
    assert (p1.factors()[0] == p2.factors()[0]).all()
    assert (rb_map.voxel_normals() == nm.voxel_normals()).all()


@pytest.mark.gpu
def test_plane_icp_refusals_unchanged(c1_f32):
    import small_gicp_amd as sga

    d = c1_f32
    full = sga.PointCloud(d["tp"], d["tn"], d["tc"])
    src = sga.PointCloud(d["sp"], d["sn"], d["sc"])
    st = sga.make_setting("PLANE_ICP")
    gv = sga.GaussianVoxelMap(1.0)
    gv.insert(full)
    cv = sga.IncrementalVoxelMapCov(1.0)
    cv.insert(full)
    pv = sga.IncrementalVoxelMap(1.0)
    pv.insert(full)
    for m in (gv, cv, pv):
        with pytest.raises(sga.SgaError, match="error 4: PLANE_ICP needs a kd-tree index over a target with normals"):  # SGA_ERR_UNSUPPORTED
            sga.Problem(m, src).linearize(st.factor, np.eye(4))
    with pytest.raises(sga.SgaError, match="error 4: per-point factors need a kd-tree target"):  # SGA_ERR_UNSUPPORTED
        sga.Problem(gv, src).linearize_per_point(st.factor, np.eye(4))


@pytest.mark.gpu
def test_cpp_registration_against_normal_flat_map(tmp_path, c1_f32):
    """tests/cpp/test_cpp_flat_plane.cpp: Registration<PointToPlaneICPFactor, ParallelReductionHIP> against IncrementalVoxelMap<FlatContainerNormal>,
    compiled with g++ against include/ only, gives the pose of the Python path to 1e-9."""
    import small_gicp_amd as sga

    d = c1_f32
    exe = tmp_path / "test_cpp_flat_plane"
    libdir = os.path.dirname(sga.LIB_PATH)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_flat_plane.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    for k in ("tp", "tn", "sp"):
        (tmp_path / (k + ".f32")).write_bytes(np.ascontiguousarray(d[k], dtype=np.float32).tobytes())
    T0 = se3([0.1, 0.2, 1.0], 0.01, [0.3, -0.2, 0.05])
    (tmp_path / "init.f64").write_bytes(np.ascontiguousarray(T0.T, dtype=np.float64).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "tp.f32"), str(tmp_path / "tn.f32"), str(tmp_path / "sp.f32"), str(tmp_path / "init.f64")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("POSE")][0].split()
    iters = int(line[1])
    Tc = np.array([float(x) for x in line[2:18]]).reshape(4, 4).T
    nm = sga.IncrementalVoxelMapNormal(1.0)
    nm.set_search_offsets(7)
    nm.insert(sga.PointCloud(d["tp"], d["tn"]))
    res = sga.Problem(nm, sga.PointCloud(d["sp"]), T0).align(sga.make_setting("PLANE_ICP"), T0)
    assert iters == res.iterations and np.abs(Tc - res.T_target_source).max() <= 1e-9, (iters, res.iterations, np.abs(Tc - res.T_target_source).max())


@pytest.mark.gpu
def test_model_odometry_plane_icp_matches_host_chain(orc):
    """run_synthetic_model(model="flat", factor="PLANE_ICP") against a frame-by-frame chain: the same device preprocessing, the same map
    inserts, and every registration solved by the host LM over the oracle's search and the restatement."""
    import small_gicp_amd as sga
    from small_gicp_amd import synthetic
    from small_gicp_amd.odometry import run_synthetic_model

    frames = 6
    r = run_synthetic_model(frames, model="flat", factor="PLANE_ICP")
    st = sga.make_setting("PLANE_ICP")
    nm, ov = sga.IncrementalVoxelMapNormal(1.0), orc.FlatMap(1.0)
    T_world = np.eye(4)
    chain = []
    for f in range(frames):
        pts, _ = synthetic.kitti_like_scan(f)
        cloud = sga.voxelgrid_sampling(sga.PointCloud(pts), 0.25)
        sga.estimate_normals(cloud, None, 20)
        p64 = cloud.xyz().astype(np.float64)
        oc = orc.Cloud(p64, None, np.tile(np.eye(3), (len(p64), 1, 1)), tree=False)  # the oracle map is searched for points only
        if f > 0:
            nrm = nm.download()[3].astype(np.float64)
            T_world = _host_plane_lm(sga, orc, ov, oc, p64, nrm, st, T_world).T_target_source
        nm.insert(cloud, T_world)
        ov.insert(oc, T_world)
        chain.append(T_world.copy())
    worst = max(np.abs(a - b).max() for a, b in zip(r["estimated"], chain))
    assert worst < 2e-4, worst
    assert r["num_voxels"] == len(nm)

"""ProjectiveSearch on the GPU (sga_index_build_projective; ann/projective_search.hpp) against tests/projective_ref.py, the numpy
restatement of the reference, and the factor sums against tests/factor_ref.py over the GPU's own pairs.

Clouds: the C1 pair, two kitti_like_scan frames turned into the camera convention (y down, z forward), the same two frames 1 km away
(a non-zero device origin: the projection adds it back in double), and a 1M-point synthetic.scene.  Projections within 1e-9 of a pixel
border (projective_ref.AMBIG: libm and the device may differ by an ulp) are left out of exact comparisons and must be rare."""
import os

import numpy as np
import pytest

import factor_ref as fr
import projective_ref as pr
from conftest import GOLDEN, pose_error

pytestmark = pytest.mark.gpu

SIZES = [(2048, 512), (1024, 64), (16, 8)]
SHIFT = np.array([1000.0, 250.0, 1000.0])
CAM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])  # sensor (x forward, z up) -> camera (y down, z forward)
MAX_SQ = 1.0
N_QUERIES = 20000


def _cam_scan(frame):
    from small_gicp_amd import synthetic

    pts, Tws = synthetic.kitti_like_scan(frame)
    return (pts.astype(np.float64) @ CAM.T).astype(np.float32), Tws


def _cam_pose(T_sensor):
    C4 = np.eye(4)
    C4[:3, :3] = CAM
    return C4 @ T_sensor @ np.linalg.inv(C4)


def _shift_pose(T, s):
    S = np.eye(4)
    S[:3, 3] = s
    return S @ T @ np.linalg.inv(S)


class Case:
    def __init__(self, name, tgt, src, T):
        self.name, self.tgt, self.src, self.T = name, tgt, src, T
        self.t_origin, self.s_origin = tgt.origin(), src.origin()
        self.t_rec = (tgt.xyz64() - self.t_origin).astype(np.float32)  # the device records fl32(p - origin), exactly
        self.s_rec = (src.xyz64() - self.s_origin).astype(np.float32)

    def T_dev(self, T):
        """The pose between the two device frames (pose_to_device): R o_s + t - o_t."""
        Td = np.array(T, dtype=np.float64)
        Td[:3, 3] = Td[:3, :3] @ self.s_origin + Td[:3, 3] - self.t_origin
        return Td


@pytest.fixture(scope="session")
def cases():
    import small_gicp_amd as sga

    out = {}
    d = np.load(os.path.join(GOLDEN, "c1_points.npz"))
    t, _ = sga.preprocess_points(d["target"], 0.25, 10)
    s, _ = sga.preprocess_points(d["source"], 0.25, 10)
    T = np.array(d["T_target_source"], dtype=np.float64)
    U, _, Vt = np.linalg.svd(T[:3, :3])
    T[:3, :3] = U @ Vt  # a rotation to the last bit: the quadratic error model of sga_error assumes R^T R = I
    out["c1"] = Case("c1", t, s, T)
    (p0, T0), (p1, T1) = _cam_scan(0), _cam_scan(1)
    T = _cam_pose(np.linalg.inv(T0) @ T1)
    clouds = []
    for p in (p0, p1):
        c = sga.PointCloud(p)
        sga.estimate_normals_covariances(c)
        clouds.append(c)
    out["kitti"] = Case("kitti", clouds[0], clouds[1], T)
    shifted = []
    for p in (p0, p1):
        c = sga.PointCloud(p.astype(np.float64) + SHIFT)
        sga.estimate_normals_covariances(c)
        shifted.append(c)
    out["kitti_1km"] = Case("kitti_1km", shifted[0], shifted[1], _shift_pose(T, SHIFT))
    from small_gicp_amd import synthetic

    out["scene_1m"] = Case("scene_1m", sga.PointCloud(synthetic.scene(1_000_000, 1)), sga.PointCloud(synthetic.scene(N_QUERIES, 2)), np.eye(4))
    return out


def _rare(amb, n):
    return int(amb.sum()) <= max(2, int(1e-5 * n))  # measured: 0 on every cloud here


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["c1", "kitti", "kitti_1km", "scene_1m"])
def test_index_map_matches_restatement(cases, name, size):
    import small_gicp_amd as sga

    c = cases[name]
    W, H = size
    ps = sga.ProjectiveSearch(c.tgt, W, H)
    assert ps.size() == len(c.t_rec)
    assert np.array_equal(ps.origin(), c.t_origin)
    got = ps.index_map()
    ref, amb = pr.build(c.t_rec, c.t_origin, W, H)
    assert _rare(amb, len(c.t_rec)), int(amb.sum())
    keep = ~pr.ambiguous_pixels(c.t_rec, c.t_origin, W, H)
    assert np.array_equal(got[keep], ref[keep])
    if name == "kitti_1km":
        assert np.any(c.t_origin != 0.0)


def _queries(c):
    q = c.src.xyz64() @ np.asarray(c.T)[:3, :3].T + np.asarray(c.T)[:3, 3]  # the source at the (near-)true pose, caller's frame
    if len(q) > N_QUERIES:
        q = q[np.random.default_rng(5).choice(len(q), N_QUERIES, replace=False)]
    return q


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", ["c1", "kitti", "kitti_1km", "scene_1m"])
def test_knn_matches_restatement(cases, name, size):
    import small_gicp_amd as sga

    c = cases[name]
    W, H = size
    ps = sga.ProjectiveSearch(c.tgt, W, H)
    img = ps.index_map()
    q = _queries(c)
    nn = None
    for k in (1, 5):
        gi, gd = ps.batch_knn_search(q, k)
        nn = gi if k == 1 else nn
        ri, rd, amb = pr.knn(img, c.t_rec, c.t_origin, q - c.t_origin, k)
        assert _rare(amb, len(q)), int(amb.sum())
        ok = ~amb
        assert np.array_equal(gi[ok], ri[ok]), (k, np.flatnonzero((gi != ri).any(1) & ok)[:5])
        fin = np.isfinite(rd[ok])
        assert np.array_equal(np.isfinite(gd[ok]), fin)
        assert np.all(np.abs(gd[ok][fin] - rd[ok][fin]) <= 1e-12 * np.maximum(rd[ok][fin], 1e-300))
    if W < 21:  # a column visited more than once pushes its points again: duplicates are the reference's answer
        p4 = sga.ProjectiveSearch(c.tgt, 4, H)
        gi, _ = p4.batch_knn_search(q[:500], 8)
        ri, _, amb4 = pr.knn(p4.index_map(), c.t_rec, c.t_origin, q[:500] - c.t_origin, 8)
        assert np.array_equal(gi[~amb4], ri[~amb4])
        assert any(len(set(r[r >= 0])) < (r >= 0).sum() for r in gi)
    gi, gd = ps.batch_knn_search(q, 3, max_sq_dist=0.25)
    ri, rd, amb = pr.knn(img, c.t_rec, c.t_origin, q - c.t_origin, 3, max_sq=0.25)
    assert np.array_equal(gi[~amb], ri[~amb])
    n, i, d = ps.nearest_neighbor_search(q[0])
    assert i == nn[0, 0] and n == (1 if i >= 0 else 0)


def test_knn_k128_and_fp32_api(cases):
    import ctypes as C

    import small_gicp_amd as sga
    from small_gicp_amd._lib import load

    c = cases["kitti"]
    ps = sga.ProjectiveSearch(c.tgt, 1024, 64)
    q = _queries(c)[:2000]
    gi, gd = ps.batch_knn_search(q, 128)
    ri, rd, amb = pr.knn(ps.index_map(), c.t_rec, c.t_origin, q - c.t_origin, 128)
    assert np.array_equal(gi[~amb], ri[~amb])
    # sga_index_knn: the fp32 query, float distances
    qf = np.ascontiguousarray(q, dtype=np.float32)
    idx = np.empty((len(q), 4), np.int64)
    d2 = np.empty((len(q), 4), np.float32)
    sga.api.check(load().sga_index_knn(c.tgt.ctx.h, ps.h, qf.ctypes.data_as(C.POINTER(C.c_float)), len(q), 4, -1.0, idx.ctypes.data_as(C.POINTER(C.c_int64)), d2.ctypes.data_as(C.POINTER(C.c_float))))
    ri, rd, amb = pr.knn(ps.index_map(), c.t_rec, c.t_origin, qf.astype(np.float64), 4, dtype=np.float32)
    assert np.array_equal(idx[~amb], ri[~amb])
    assert np.array_equal(d2[~amb], rd[~amb])
    with pytest.raises(sga.SgaError):
        ps.batch_knn_search(q[:4], 129)


@pytest.fixture(scope="session")
def ref_pairs(cases):
    """Restated correspondences per (case, arithmetic) at the case's pose, 2048 x 512, the default window and borders."""
    out = {}
    for name in ("c1", "kitti", "kitti_1km"):
        c = cases[name]
        img, _ = pr.build(c.t_rec, c.t_origin, 2048, 512)
        for dt in (np.float64, np.float32):
            out[name, dt] = pr.pairs(img, c.t_rec, c.t_origin, c.s_rec, c.T_dev(c.T), MAX_SQ, dtype=dt)
    return out


KINDS = {"ICP": fr.ICP, "PLANE_ICP": fr.PLANE_ICP, "GICP": fr.GICP}
ROBUST = {None: fr.ROBUST_NONE, "HUBER": fr.ROBUST_HUBER, "CAUCHY": fr.ROBUST_CAUCHY}


def _close(a, b, tol):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.mark.parametrize("robust", [None, "HUBER", "CAUCHY"])
@pytest.mark.parametrize("kind", ["ICP", "PLANE_ICP", "GICP"])
@pytest.mark.parametrize("name", ["c1", "kitti", "kitti_1km"])
def test_linearize_fp64_pairs_and_sums(cases, ref_pairs, name, kind, robust):
    import small_gicp_amd as sga

    c = cases[name]
    ps = sga.ProjectiveSearch(c.tgt, 2048, 512)
    st = sga.make_setting(kind, np.sqrt(MAX_SQ), robust_kernel=robust, robust_c=0.5, math_mode="fp64")
    pb = sga.Problem(ps, c.src, c.T)
    H, b, e, n = pb.linearize(st.factor, c.T)
    assert pb.last_plan()["route"] == "factors" and pb.last_plan()["pts"] == 1
    corr, _ = pb.factors()
    rc, amb = ref_pairs[name, np.float64]
    assert _rare(amb, len(rc)), int(amb.sum())
    assert np.array_equal(corr[~amb], rc[~amb]), np.flatnonzero((corr != rc) & ~amb)[:5]
    assert n == int((corr >= 0).sum())
    if name == "kitti_1km":
        return  # the caller-frame sums of a cloud 1 km out are pinned by the unshifted twin (device frames: common.hpp)
    src, tgt = c.src.xyz64(), c.tgt.xyz64()
    ref = fr.linearize(src, tgt, corr, c.T, KINDS[kind], ROBUST[robust], 0.5, c.src.covs(), c.tgt.covs(), c.tgt.normals())
    assert n == ref.inliers
    assert _close(H, ref.H, 1e-10) and _close(b, ref.b, 1e-10), (np.abs(H - ref.H).max(), np.abs(b - ref.b).max())
    assert abs(e - ref.e) <= 1e-10 * abs(ref.e)
    Tq = c.T.copy()
    Tq[:3, 3] += [0.01, -0.02, 0.005]
    eg = pb.error(st.factor, Tq)
    er = fr.error(src, tgt, corr, Tq, KINDS[kind], ROBUST[robust], 0.5, ref.maha, c.tgt.normals())
    assert abs(eg - er) <= 1e-9 * abs(er), (eg, er)


@pytest.mark.parametrize("name", ["c1", "kitti"])
def test_linearize_fp32_pairs(cases, ref_pairs, name):
    import small_gicp_amd as sga

    c = cases[name]
    ps = sga.ProjectiveSearch(c.tgt, 2048, 512)
    st = sga.make_setting("GICP", np.sqrt(MAX_SQ))
    pb = sga.Problem(ps, c.src, c.T)
    _, _, _, n = pb.linearize(st.factor, c.T)
    corr, _ = pb.factors()
    rc, amb = ref_pairs[name, np.float32]
    differ = int(((corr != rc) & ~amb).sum())
    assert differ <= 1e-4 * len(rc), differ
    assert n == int((corr >= 0).sum())


def test_window_and_border_setters(cases):
    import small_gicp_amd as sga

    c = cases["kitti"]
    q = _queries(c)[:5000]
    for W, H, wh, wv, bh, bv in [(1024, 64, 3, 2, "repeat", "clamp"), (1024, 64, 0, 0, "clamp", "clamp"), (16, 8, 10, 5, "clamp", "repeat"), (16, 8, 12, 6, "repeat", "repeat")]:
        ps = sga.ProjectiveSearch(c.tgt, W, H, search_window_h=wh, search_window_v=wv, border_h=bh, border_v=bv)
        img = ps.index_map()
        gi, _ = ps.batch_knn_search(q, 3)
        ri, _, amb = pr.knn(img, c.t_rec, c.t_origin, q - c.t_origin, 3, wh, wv, bh == "repeat", bv == "repeat")
        assert np.array_equal(gi[~amb], ri[~amb]), (W, H, wh, wv, bh, bv)
        # the same index, parameters changed afterwards: read at each search, including a registration pass
        ps.set_search_window(1, 1)
        ps.set_border_modes("repeat", "clamp")
        gi, _ = ps.batch_knn_search(q, 1)
        ri, _, amb = pr.knn(img, c.t_rec, c.t_origin, q - c.t_origin, 1, 1, 1, True, False)
        assert np.array_equal(gi[~amb], ri[~amb])
        st = sga.make_setting("ICP", np.sqrt(MAX_SQ), math_mode="fp64")
        pb = sga.Problem(ps, c.src, c.T)
        pb.linearize(st.factor, c.T)
        rc, amb = pr.pairs(img, c.t_rec, c.t_origin, c.s_rec, c.T_dev(c.T), MAX_SQ, 1, 1, True, False)
        assert np.array_equal(pb.factors()[0][~amb], rc[~amb])
    with pytest.raises(sga.SgaError):
        ps.set_search_window(-1, 2)


def test_align_fp64_matches_host_lm(cases):
    import small_gicp_amd as sga

    c = cases["c1"]
    ps = sga.ProjectiveSearch(c.tgt, 2048, 512)
    img = ps.index_map()
    st = sga.make_setting("GICP", np.sqrt(MAX_SQ), math_mode="fp64")
    T0 = c.T.copy()
    T0[:3, 3] += [0.05, -0.03, 0.02]
    res = sga.Problem(ps, c.src, T0).align(st, T0)
    src, tgt, scov, tcov = c.src.xyz64(), c.tgt.xyz64(), c.src.covs(), c.tgt.covs()
    state = {}

    def lin(T):
        corr, _ = pr.pairs(img, c.t_rec, c.t_origin, c.s_rec, c.T_dev(T), MAX_SQ)
        s = fr.linearize(src, tgt, corr, T, fr.GICP, src_cov=scov, tgt_cov=tcov)
        state["corr"], state["maha"] = corr, s.maha
        return s.H, s.b, s.e, s.inliers

    def err(T):
        return fr.error(src, tgt, state["corr"], T, fr.GICP, maha=state["maha"])

    ref = sga.optimize(st, T0, lin, err)
    dt, dr = pose_error(res.T_target_source, ref.T_target_source)
    assert res.iterations == ref.iterations and dt < 1e-9 and dr < 1e-9, (res.iterations, ref.iterations, dt, dr)
    assert res.num_inliers == ref.num_inliers
    # align() with the projective search as the target tree
    res2 = sga.align(c.tgt, c.src, ps, T0, registration_type="GICP", max_correspondence_distance=1.0)
    assert res2.converged


def test_refusals(cases):
    import small_gicp_amd as sga
    from small_gicp_amd._lib import load

    c = cases["c1"]
    ps = sga.ProjectiveSearch(c.tgt, 1024, 64)
    pb = sga.Problem(ps, c.src, c.T)
    with pytest.raises(sga.SgaError, match="kd-tree"):
        pb.set_rejector(lambda T, idx, d2: np.zeros(len(idx), bool))
    with pytest.raises(sga.SgaError, match="kd-tree"):
        pb.linearize_per_point(sga.make_setting("ICP").factor, c.T)
    with pytest.raises(sga.SgaError, match="projective"):
        sga.Problem(sga.KdTree(c.tgt), ps, c.T)
    with pytest.raises(sga.SgaError, match="projective"):
        sga.estimate_covariances(c.tgt, tree=ps)
    with pytest.raises(sga.SgaError):
        sga.ProjectiveSearch(c.tgt, 0, 64)
    bare = sga.ProjectiveSearch(sga.PointCloud(c.tgt.xyz()), 1024, 64)
    with pytest.raises(sga.SgaError, match="normals"):
        sga.Problem(bare, c.src, c.T).linearize(sga.make_setting("PLANE_ICP").factor, c.T)
    assert load().sga_index_build_projective is not None


def test_clone_and_refresh(cases):
    import ctypes as C

    import small_gicp_amd as sga
    from small_gicp_amd._lib import load

    c = cases["kitti"]
    ps = sga.ProjectiveSearch(c.tgt, 1024, 64, search_window_h=4)
    h = C.c_void_p()
    sga.api.check(load().sga_index_clone(c.tgt.ctx.h, ps.h, C.byref(h)))
    try:
        params = (C.c_int * 6)()
        sga.api.check(load().sga_projective_get_params(h, params))
        assert list(params) == [1024, 64, 4, 5, 1, 0]
        out = np.empty((64, 1024), np.uint32)
        sga.api.check(load().sga_projective_download_map(c.tgt.ctx.h, h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        assert np.array_equal(out, ps.index_map())
    finally:
        load().sga_index_destroy(h)
    ps.refresh_attributes()
    st = sga.make_setting("PLANE_ICP", np.sqrt(MAX_SQ), math_mode="fp64")
    H, _, _, n = sga.Problem(ps, c.src, c.T).linearize(st.factor, c.T)
    assert n > 0.5 * c.src.size() and np.isfinite(H).all()


def test_cpp_registration_against_projective_search(tmp_path, cases):
    """tests/cpp/test_cpp_projective.cpp, compiled with g++ against include/ only: the NN / kNN of the C++ ProjectiveSearch and a
    point-to-plane Registration::align against it (window 8 x 3 set through the public members) give the Python path's answers."""
    import subprocess

    import small_gicp_amd as sga
    from conftest import ROOT

    c = cases["c1"]
    tp, tn, sp = c.tgt.xyz(), np.ascontiguousarray(c.tgt.normals()[:, :3], dtype=np.float32), c.src.xyz()
    exe = tmp_path / "test_cpp_projective"
    libdir = os.path.dirname(sga.LIB_PATH)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_projective.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    for k, a in (("tp", tp), ("tn", tn), ("sp", sp)):
        (tmp_path / (k + ".f32")).write_bytes(np.ascontiguousarray(a, dtype=np.float32).tobytes())
    T0 = np.asarray(c.T, dtype=np.float64)
    (tmp_path / "init.f64").write_bytes(np.ascontiguousarray(T0.T, dtype=np.float64).tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "tp.f32"), str(tmp_path / "tn.f32"), str(tmp_path / "sp.f32"), str(tmp_path / "init.f64")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {ln.split()[0]: ln.split()[1:] for ln in p.stdout.splitlines() if ln[:2] in ("NN", "KN", "PO")}
    ps = sga.ProjectiveSearch(sga.PointCloud(tp, tn), 1024, 64, search_window_h=8, search_window_v=3)
    q = sp[:1].astype(np.float64)
    gi, gd = ps.batch_knn_search(q, 5)
    assert int(out["NN"][0]) == gi[0, 0] and (gi[0, 0] < 0 or float(out["NN"][1]) == gd[0, 0])
    assert [int(x) for x in out["KNN"][1:]] == [int(x) for x in gi[0] if x >= 0]
    res = sga.Problem(ps, sga.PointCloud(sp), T0).align(sga.make_setting("PLANE_ICP"), T0)
    Tc = np.array([float(x) for x in out["POSE"][1:17]]).reshape(4, 4).T
    assert int(out["POSE"][0]) == res.iterations and np.abs(Tc - res.T_target_source).max() <= 1e-9, (out["POSE"][0], res.iterations)


def test_hand_built_cases_on_the_gpu():
    """The hand-built cases of tests/test_projective_ref.py through the device: the image, 1-NN / k-NN, and the pairs of an fp64 ICP pass
    (the source points are the queries, identity pose, no rejector)."""
    import small_gicp_amd as sga
    from test_projective_ref import at

    W, H = 16, 8
    cases_ = [
        # (target, queries, width, window h, window v, repeat_h, repeat_v)
        ([at(W - 1, 3), at(6, 3)], [at(0, 3)], W, 2, 1, True, False),  # seam wrap
        ([at(W - 1, 3), at(6, 3)], [at(0, 3)], W, 2, 1, False, False),  # no wrap when clamped
        ([at(4, 0)], [at(4, 0)], W, 0, 5, True, False),  # pole rows skipped, not clamped
        ([at(4, H - 1)], [at(4, 0)], W, 0, 2, True, True),  # vertical wrap
        ([at(5, 5, r=4.0), at(5, 5, r=9.0), at(5, 5, r=6.0)], [at(5, 5, r=4.0)], W, 10, 5, True, False),  # last index wins
        ([[1.0, 0.0, 3.0], [-1.0, 0.0, 3.0]], [[0.0, 0.0, 0.0], [0.0, 0.0, 0.01]], W, 10, 5, True, False),  # tie: first in scan order
        ([[1.0, -1.0, 3.0], [1.0, 1.0, 3.0]], [[1.0, 0.0, 3.0]], W, 10, 5, True, False),  # tie in one column: smaller v first
        ([[1.0, 1.0, 3.0], [1.0, -1.0, 3.0]], [[1.0, 0.0, 3.0]], W, 10, 5, True, False),
        ([at(1, 2, W=8)], [at(0, 2, W=8)], 8, 10, 0, True, False),  # a column visited three times
        ([[0.0, 0.0, -3.0], [-0.0, 0.0, -3.0], [0.01, -0.02, 0.0], [np.nan, 1.0, 1.0]], [[0.0, 0.0, -3.0], [0.0, 0.0, 0.0]], W, 1, 1, True, False),
    ]
    for tgt, qs, w, wh, wv, rh, rv in cases_:
        tgt = np.asarray(tgt, dtype=np.float32)
        qs = np.asarray(qs, dtype=np.float64)
        cloud = sga.PointCloud(tgt)
        ps = sga.ProjectiveSearch(cloud, w, H, wh, wv, "repeat" if rh else "clamp", "repeat" if rv else "clamp")
        ref_img, _ = pr.build(tgt, np.zeros(3), w, H)
        assert np.array_equal(ps.index_map(), ref_img)
        for k in (1, 4):
            gi, gd = ps.batch_knn_search(qs, k)
            ri, rd, _ = pr.knn(ref_img, tgt, np.zeros(3), qs, k, wh, wv, rh, rv)
            assert np.array_equal(gi, ri), (tgt.tolist(), qs.tolist(), gi, ri)
            assert np.array_equal(gd, rd)
        st = sga.make_setting("ICP", None, math_mode="fp64")
        pb = sga.Problem(ps, sga.PointCloud(qs.astype(np.float32)), np.eye(4))
        pb.linearize(st.factor, np.eye(4))
        ri, _, _ = pr.nearest(ref_img, tgt, np.zeros(3), qs.astype(np.float32).astype(np.float64), wh, wv, rh, rv)
        assert np.array_equal(pb.factors()[0], ri), (tgt.tolist(), qs.tolist(), pb.factors()[0], ri)

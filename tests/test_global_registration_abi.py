"""The boundary of the global registration without a device: the symbols exist and are bound with the header's
signatures, the ctypes structures have the header's sizes, sga_ransac_default gives the defaults; null arguments and every bad value are
refused before any handle is read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_crop_abi.py's
technique) — with *out NULL afterwards and nothing enqueued.  The host arithmetic of the RANSAC — the generator and the least-squares
solver — is reached through its debug entry points and held against tests/global_ref.py and numpy's SVD.  What needs live clouds is
tests/test_global_registration_gpu.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import global_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
INF, NAN = float("inf"), float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp, _pvp, _dp, _fp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.POINTER(C.c_float)
_pull = C.POINTER(C.c_ulonglong)


def message():
    return sga.load().sga_last_error().decode()


def launches():
    return api.cloud_fpfh_launches(), api.features_match_launches(), api.ransac_launches()


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    want = {
        "sga_features_create": (C.c_int, [_vp, _fp, C.c_size_t, C.c_int, _pvp]),
        "sga_features_size": (C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
        "sga_features_download": (C.c_int, [_vp, _vp, _fp]),
        "sga_features_destroy": (C.c_int, [_vp]),
        "sga_cloud_fpfh": (C.c_int, [_vp, _vp, _vp, C.c_int, _dp, _pvp]),  # ctx, cloud, kdtree, k, viewpoint, out
        "sga_features_match": (C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_size_t)]),
        "sga_ransac_default": (None, [C.POINTER(_lib.Ransac)]),
        "sga_ransac_correspondences": (C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(_lib.Ransac), _dp, C.POINTER(_lib.RansacResult)]),
        "sga_debug_cloud_fpfh_launches": (C.c_int, [_pull]),
        "sga_debug_features_match_launches": (C.c_int, [_pull]),
        "sga_debug_ransac_launches": (C.c_int, [_pull]),
        "sga_debug_ransac_draw": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
        "sga_debug_rigid_from_sums": (C.c_int, [C.c_uint64, _dp, _dp, _dp, _dp]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert bound.get(name) == sig, name
    for name in ("Features", "compute_fpfh", "match_features", "ransac_correspondences", "global_align", "cloud_fpfh_launches", "features_match_launches", "ransac_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.fpfh) and callable(sga.Features.from_array) and callable(sga.synthetic.bumpy_terrain)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_ransac \{(.*?)\} sga_ransac;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|uint64_t)\s+([a-z_, ]+);", m.group(1))
    assert [(t, n.strip()) for t, n in fields] == [("double", "max_distance"), ("uint64_t", "iterations"), ("uint64_t", "seed"), ("double", "edge_similarity"), ("double", "min_edge")]
    assert [n for n, _ in _lib.Ransac._fields_] == ["max_distance", "iterations", "seed", "edge_similarity", "min_edge"] and C.sizeof(_lib.Ransac) == 40
    m = re.search(r"typedef struct sga_ransac_result \{(.*?)\} sga_ransac_result;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|uint64_t)\s+([a-z_, ]+);", m.group(1))
    assert [(t, n.strip()) for t, n in fields] == [("uint64_t", "inliers"), ("double", "inlier_rmse"), ("uint64_t", "best_hypothesis"), ("uint64_t", "scored"), ("int", "refit"), ("int", "reserved")]
    assert [n for n, _ in _lib.RansacResult._fields_] == ["inliers", "inlier_rmse", "best_hypothesis", "scored", "refit", "reserved"] and C.sizeof(_lib.RansacResult) == 40
    assert "#define SGA_FPFH_DIM 33" in text and _lib.FPFH_DIM == 33
    assert "int sga_cloud_fpfh(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree" in text
    assert "int sga_features_match(sga_context* ctx, const sga_features* source, const sga_features* target, int mutual, int64_t* match" in text
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    for name in ("sga_debug_cloud_fpfh_launches", "sga_debug_features_match_launches", "sga_debug_ransac_launches"):
        assert "int %s(unsigned long long* launches);" % name in debug


def test_defaults():
    p = _lib.Ransac()
    sga.load().sga_ransac_default(C.byref(p))
    assert (p.max_distance, p.iterations, p.seed, p.edge_similarity, p.min_edge) == (1.0, 20000, 0, 0.9, 0.0)
    sga.load().sga_ransac_default(None)  # a NULL struct is left alone
    q = api._ransac_params(max_distance=0.75, seed=3)
    assert (q.max_distance, q.iterations, q.seed, q.edge_similarity, q.min_edge) == (0.75, 20000, 3, 0.9, 0.0)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def fpfh(ctx=STAND_IN, cloud=STAND_IN, k=20, viewpoint=None, with_out=True):
    out = C.c_void_p(0xDEAD)
    vp = None if viewpoint is None else (C.c_double * 3)(*viewpoint)
    rc = sga.load().sga_cloud_fpfh(C.c_void_p(ctx), C.c_void_p(cloud), None, k, vp, C.byref(out) if with_out else None)
    return rc, out.value


def test_fpfh_refusals_come_before_a_handle_is_read():
    before = launches()
    for kw in ({"ctx": 0}, {"cloud": 0}, {"with_out": False}):
        rc, out = fpfh(**kw)
        assert rc == INVALID and "null argument" in message(), kw
        if kw.get("with_out", True):
            assert out is None  # *out = NULL on every failure
    for k in (-1, 0, 1, 64, 1000):
        rc, out = fpfh(k=k)
        assert rc == INVALID and out is None and "k must be in [2,63]" in message(), k
    for vp in ((NAN, 0, 0), (0, INF, 0), (0, 0, -INF)):
        rc, out = fpfh(viewpoint=vp)
        assert rc == INVALID and out is None and "viewpoint" in message(), vp
    assert launches() == before


def test_features_refusals():
    lib = sga.load()
    before = launches()
    rows = (C.c_float * 4)()
    for ctx, data, n, dim, word in ((0, rows, 1, 4, "null argument"), (STAND_IN, None, 1, 4, "null argument"), (STAND_IN, rows, 1, 0, "dim must be in [1,128]"), (STAND_IN, rows, 1, 129, "dim must be in [1,128]"),
                                    (STAND_IN, rows, 1, -3, "dim must be in [1,128]"), (STAND_IN, rows, 1 << 31, 1, "too many rows")):
        out = C.c_void_p(0xDEAD)
        assert lib.sga_features_create(C.c_void_p(ctx), data, n, dim, C.byref(out)) == INVALID and out.value is None and word in message(), word
    assert lib.sga_features_create(C.c_void_p(STAND_IN), rows, 1, 4, None) == INVALID
    assert lib.sga_features_size(None, None, None) == INVALID and lib.sga_features_download(None, None, None) == INVALID
    assert lib.sga_features_destroy(None) == OK
    match = (C.c_int64 * 1)()
    for ctx, s, t, mutual, m, word in ((0, STAND_IN, STAND_IN, 1, match, "null argument"), (STAND_IN, 0, STAND_IN, 1, match, "null argument"), (STAND_IN, STAND_IN, 0, 1, match, "null argument"),
                                       (STAND_IN, STAND_IN, STAND_IN, 1, None, "null argument"), (STAND_IN, STAND_IN, STAND_IN, 2, match, "mutual 2"), (STAND_IN, STAND_IN, STAND_IN, -1, match, "mutual -1")):
        assert lib.sga_features_match(C.c_void_p(ctx), C.c_void_p(s), C.c_void_p(t), mutual, m, None, None) == INVALID and word in message(), word
    assert launches() == before


@pytest.mark.parametrize(
    "fields, word",
    [
        ({"max_distance": 0.0}, "max_distance"),
        ({"max_distance": -1.0}, "max_distance"),
        ({"max_distance": NAN}, "max_distance"),
        ({"max_distance": INF}, "max_distance"),
        ({"iterations": 0}, "iterations"),
        ({"iterations": 1 << 32}, "iterations"),
        ({"edge_similarity": -0.1}, "edge_similarity"),
        ({"edge_similarity": 1.5}, "edge_similarity"),
        ({"edge_similarity": NAN}, "edge_similarity"),
        ({"min_edge": -1.0}, "min_edge"),
        ({"min_edge": NAN}, "min_edge"),
        ({"min_edge": INF}, "min_edge"),
    ],
)
def test_bad_ransac_parameters_are_refused_before_a_handle_is_read(fields, word):
    before = launches()
    p = api._ransac_params(**fields)
    pairs = (C.c_int64 * 6)(0, 0, 1, 1, 2, 2)
    T, r = (C.c_double * 16)(), _lib.RansacResult()
    rc = sga.load().sga_ransac_correspondences(C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), pairs, 3, C.byref(p), T, C.byref(r))  # (the stand-ins would fault if read)
    assert rc == INVALID and word in message(), message()
    assert launches() == before


def test_ransac_null_arguments():
    lib = sga.load()
    p = api._ransac_params()
    pairs = (C.c_int64 * 6)()
    T, r = (C.c_double * 16)(), _lib.RansacResult()
    S = C.c_void_p(STAND_IN)
    assert lib.sga_ransac_correspondences(None, S, S, pairs, 3, C.byref(p), T, C.byref(r)) == INVALID and "null argument" in message()
    assert lib.sga_ransac_correspondences(S, None, S, pairs, 3, C.byref(p), T, C.byref(r)) == INVALID
    assert lib.sga_ransac_correspondences(S, S, None, pairs, 3, C.byref(p), T, C.byref(r)) == INVALID
    assert lib.sga_ransac_correspondences(S, S, S, None, 3, C.byref(p), T, C.byref(r)) == INVALID
    assert lib.sga_ransac_correspondences(S, S, S, pairs, 3, None, T, C.byref(r)) == INVALID
    assert lib.sga_ransac_correspondences(S, S, S, pairs, 3, C.byref(p), None, C.byref(r)) == INVALID
    assert lib.sga_ransac_correspondences(S, S, S, pairs, 3, C.byref(p), T, None) == INVALID
    assert lib.sga_ransac_correspondences(S, S, S, pairs, 1 << 31, C.byref(p), T, C.byref(r)) == INVALID and "too many pairs" in message()


# ---- the host arithmetic --------------------------------------------------------------------------------------------------------------------
def test_the_generator_is_the_restatements():
    lib = sga.load()
    rng = np.random.default_rng(11)
    out = (C.c_uint64 * 3)()
    Ms = np.concatenate([[3, 4, 5, (1 << 31) - 1], rng.integers(3, 1 << 31, 96)])
    count = 0
    for M in Ms:
        seeds = rng.integers(0, 1 << 63, 10, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 10, dtype=np.uint64)  # all 64 bits
        for seed in seeds:
            hs = np.concatenate([[0, (1 << 32) - 2], rng.integers(0, 1 << 32, 8)])
            want = ref.draws(int(seed), hs, int(M))
            for h, w in zip(hs, want):
                assert lib.sga_debug_ransac_draw(int(seed), int(h), int(M), out) == OK
                assert list(out) == w.tolist(), (seed, h, M)
                assert len(set(out)) == 3 and max(out) < M
                count += 1
    assert count == 10000
    assert lib.sga_debug_ransac_draw(0, 0, 2, out) == INVALID and lib.sga_debug_ransac_draw(0, 0, 1 << 31, out) == INVALID
    assert lib.sga_debug_ransac_draw(0, 0, 3, None) == INVALID


def rigid_from_sums(ps, pt):
    ps, pt = np.ascontiguousarray(ps, dtype=np.float64), np.ascontiguousarray(pt, dtype=np.float64)
    ss, st = np.ascontiguousarray(ps.sum(axis=0)), np.ascontiguousarray(pt.sum(axis=0))
    cross = np.ascontiguousarray(ps.T @ pt).reshape(9)
    T = np.full(16, -7.0)
    ok = sga.load().sga_debug_rigid_from_sums(len(ps), api._dp(ss), api._dp(st), api._dp(cross), api._dp(T))
    return ok, T.reshape(4, 4).T


def test_the_solver_against_numpy_svd():
    rng = np.random.default_rng(21)
    worst = [0.0, 0.0]
    for trial in range(200):
        n = int(rng.integers(3, 60))
        axis, angle = rng.normal(size=3), rng.uniform(-np.pi, np.pi)
        if trial % 10 == 0:
            angle = np.pi - 1e-9 * trial  # a half turn: the quaternion's w is ~0
        K = np.cross(np.eye(3), axis / np.linalg.norm(axis))
        R = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
        ps = rng.uniform(-20, 20, (n, 3))
        if trial % 7 == 0:
            ps[:, 2] = 0.25 * ps[:, 0] - 3.0  # coplanar points: rank 2, still one proper rotation
        pt = ps @ R.T + rng.uniform(-50, 50, 3) + rng.normal(0, 0.05, (n, 3))
        ok, T = rigid_from_sums(ps, pt)
        assert ok == 1
        dt, dr = ref.pose_error(T, ref.kabsch(ps, pt))
        worst = [max(worst[0], dt), max(worst[1], dr)]
        assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12 and np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12)
        assert T[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    print("greatest deviation from numpy's SVD solution: %.3e m, %.3e rad" % tuple(worst))
    assert worst[0] < 1e-9 and worst[1] < 1e-10  # plain sums of coordinates up to 70 m over 60 points: ~1e5 eps


def test_the_solver_keeps_out_of_rank_deficient_sums():
    line = np.outer(np.linspace(-3, 3, 9), [1.0, 2.0, -1.0]) + [5.0, 0.0, 1.0]
    ok, T = rigid_from_sums(line, line @ ref.kabsch(np.eye(3), np.eye(3)[[1, 2, 0]])[:3, :3].T)
    assert ok == 0 and (T == -7.0).all()  # collinear: rank 1, T untouched
    pts = np.random.default_rng(2).normal(size=(2, 3))
    assert rigid_from_sums(pts, pts)[0] == 0  # fewer than three pairs
    same = np.tile([[1.0, 2.0, 3.0]], (5, 1))
    assert rigid_from_sums(same, same)[0] == 0  # rank 0
    lib = sga.load()
    assert lib.sga_debug_rigid_from_sums(5, None, None, None, None) == 0

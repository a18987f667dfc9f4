"""The boundary of the plane segmentation without a device: the symbols exist and are bound with the header's
signatures, the ctypes structures have the header's fields and sizes (72 and 48 bytes), sga_plane_default gives the defaults; null
arguments and parameters outside their ranges are refused before any handle is read — the handles are stand-ins at an address nothing
is mapped at (tests/test_global_registration_abi.py's technique) — with the outputs untouched and nothing enqueued.  The host solver of
the refit (sga_debug_plane_from_sums) is held against numpy.linalg.eigh."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
INF, NAN = float("inf"), float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP, U32, I64 = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_int64)
VP, PVP, ULL = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong)
PPP, PPR = C.POINTER(_lib.PlaneParams), C.POINTER(_lib.PlaneResult)
SENTINEL = 0xDEAD


def message():
    return sga.load().sga_last_error().decode()


def params(**fields):
    p = _lib.PlaneParams()
    sga.load().sga_plane_default(C.byref(p))
    for name, value in fields.items():
        if name == "axis":
            p.axis[0], p.axis[1], p.axis[2] = value
        else:
            setattr(p, name, value)
    return p


def counters():
    return [sga.segment_plane_launches(), sga.segment_plane_waits()]


def segment(p, ctx=STAND_IN, cloud=STAND_IN, with_plane=True, with_result=True, with_kept=False, with_out=None):
    """-> (status, outputs untouched, out)"""
    with_out = (p is not None and p.keep != 0) if with_out is None else with_out
    plane = np.full(4, -7.0)
    scores = np.full(4, 7, np.uint32)
    kept = np.full(4, -7, np.int64)
    res = _lib.PlaneResult(SENTINEL, -7.0, SENTINEL, SENTINEL, SENTINEL, 7, 7)
    out = C.c_void_p(SENTINEL)
    rc = sga.load().sga_cloud_segment_plane(C.c_void_p(ctx), C.c_void_p(cloud), None if p is None else C.byref(p), plane.ctypes.data_as(DP) if with_plane else None, scores.ctypes.data_as(U32),
                                            kept.ctypes.data_as(I64) if with_kept else None, C.byref(out) if with_out else None, C.byref(res) if with_result else None)
    untouched = (plane == -7.0).all() and (scores == 7).all() and (kept == -7).all() and res.inliers == SENTINEL and res.scored == SENTINEL and res.refit == 7
    return rc, untouched, out.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    want = {
        "sga_plane_default": (None, [PPP]),
        "sga_cloud_segment_plane": (C.c_int, [VP, VP, PPP, DP, U32, I64, PVP, PPR]),
        "sga_debug_segment_plane_launches": (C.c_int, [ULL]),
        "sga_debug_segment_plane_waits": (C.c_int, [ULL]),
        "sga_debug_plane_from_sums": (C.c_int, [C.c_uint64, DP, DP, DP, DP, DP]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert bound.get(name) == sig, name
    for name in ("segment_plane", "segment_planes", "segment_plane_launches", "segment_plane_waits"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.segment_plane)
    from small_gicp_amd import odometry

    assert callable(odometry.run_synthetic_ground)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    ctype = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64, "uint64_t": C.c_uint64}

    def fields_of(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
        assert m is not None, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        out = []
        for t, names in re.findall(r"\b(uint64_t|int64_t|int|double)\s+([a-z_, \[\]0-9]+);", body):
            for n in names.split(","):
                n = n.strip()
                arr = re.match(r"(\w+)\[(\d+)\]", n)
                out.append((arr.group(1), ctype[t] * int(arr.group(2))) if arr else (n, ctype[t]))
        return out

    def same(a, b):
        return [(n, C.sizeof(t)) for n, t in a] == [(n, C.sizeof(t)) for n, t in b]

    assert same(fields_of("sga_plane_params"), _lib.PlaneParams._fields_)
    assert [n for n, _ in _lib.PlaneParams._fields_] == ["distance_threshold", "iterations", "seed", "axis", "max_angle", "min_inliers", "refit", "keep"]
    assert same(fields_of("sga_plane_result"), _lib.PlaneResult._fields_)
    assert [n for n, _ in _lib.PlaneResult._fields_] == ["inliers", "rmse", "hypothesis_inliers", "best_hypothesis", "scored", "refit", "reserved"]
    assert (C.sizeof(_lib.PlaneParams), C.sizeof(_lib.PlaneResult)) == (72, 48)
    assert "} sga_plane_params; /* 72 bytes */" in text and "} sga_plane_result; /* 48 bytes */" in text
    for decl in (
        "void sga_plane_default(sga_plane_params* p);",
        "int sga_cloud_segment_plane(sga_context* ctx, const sga_cloud* cloud, const sga_plane_params* params, double plane[4], uint32_t* scores",
    ):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    for name in ("sga_debug_segment_plane_launches(unsigned long long* launches)", "sga_debug_segment_plane_waits(unsigned long long* waits)",
                 "sga_debug_plane_from_sums(uint64_t k, const double sum_x[3], const double sum_xx6[6], double normal[3], double centroid_offset[3], double eigenvalues[3])"):
        assert "int %s;" % name in debug, name


def test_defaults():
    p = params()
    assert (p.distance_threshold, p.iterations, p.seed, list(p.axis), p.max_angle, p.min_inliers, p.refit, p.keep) == (0.1, 1000, 0, [0.0, 0.0, 0.0], 0.0, 3, 1, 0)
    sga.load().sga_plane_default(None)  # a NULL struct is left alone
    assert bytes(api._plane_params()) == bytes(p)
    q = api._plane_params(0.25, iterations=64, seed=2**64 - 1, axis=(0, 0, 1), max_angle=0.2, min_inliers=10, refit=False, keep="rest")
    assert (q.distance_threshold, q.iterations, q.seed, list(q.axis), q.max_angle, q.min_inliers, q.refit, q.keep) == (0.25, 64, 2**64 - 1, [0.0, 0.0, 1.0], 0.2, 10, 0, 2)
    assert api._plane_params(q) is q and api._plane_params(keep="plane").keep == 1
    with pytest.raises(ValueError):
        api._plane_params(0.5, keep="everything")


def test_null_arguments_are_refused():
    before = counters()
    p = params()
    for rc, untouched, out in (segment(p, ctx=0), segment(p, cloud=0), segment(None), segment(p, with_plane=False), segment(p, with_result=False)):
        assert rc == INVALID and "null argument" in message() and untouched and out == SENTINEL
    rc, untouched, out = segment(params(keep=1), ctx=0)
    assert rc == INVALID and untouched and out is None  # *out = NULL on every refusal
    assert sga.load().sga_debug_segment_plane_launches(None) == INVALID and sga.load().sga_debug_segment_plane_waits(None) == INVALID
    z3, z6 = np.zeros(3), np.zeros(6)
    assert sga.load().sga_debug_plane_from_sums(5, None, z6.ctypes.data_as(DP), z3.ctypes.data_as(DP), z3.ctypes.data_as(DP), z3.ctypes.data_as(DP)) == 0
    assert counters() == before


BAD_PARAMS = [
    ({"distance_threshold": 0.0}, "distance_threshold must be finite and > 0"),
    ({"distance_threshold": -0.1}, "distance_threshold must be finite and > 0"),
    ({"distance_threshold": INF}, "distance_threshold must be finite and > 0"),
    ({"distance_threshold": NAN}, "distance_threshold must be finite and > 0"),
    ({"iterations": 0}, "iterations must be in [1, 2^20]"),
    ({"iterations": 2**20 + 1}, "iterations must be in [1, 2^20]"),
    ({"iterations": 2**63}, "iterations must be in [1, 2^20]"),
    ({"axis": (0.0, NAN, 1.0), "max_angle": 0.1}, "axis has a non-finite entry"),
    ({"axis": (INF, 0.0, 0.0), "max_angle": 0.1}, "axis has a non-finite entry"),
    ({"axis": (0.0, 0.0, 1.0)}, "an axis needs a max_angle"),
    ({"axis": (0.0, 0.0, 1.0), "max_angle": 1.6}, "max_angle must be in [0, pi/2]"),
    ({"max_angle": -0.1}, "max_angle must be in [0, pi/2]"),
    ({"max_angle": NAN}, "max_angle must be in [0, pi/2]"),
    ({"min_inliers": 2}, "min_inliers 2 is below 3"),
    ({"min_inliers": 0}, "min_inliers 0 is below 3"),
    ({"refit": 2}, "refit 2 is not 0 or 1"),
    ({"refit": -1}, "refit -1 is not 0 or 1"),
    ({"keep": 3}, "keep 3 is not 0"),
    ({"keep": -1}, "keep -1 is not 0"),
]


@pytest.mark.parametrize("fields, word", BAD_PARAMS)
def test_bad_parameters_are_refused_before_a_handle_is_read(fields, word):
    before = counters()
    rc, untouched, out = segment(params(**fields), with_out=False)  # (the stand-in handles would fault if they were read)
    assert rc == INVALID and word in message() and untouched, message()
    assert counters() == before


def test_keep_must_agree_with_its_outputs():
    before = counters()
    for p, kw, word in (
        (params(keep=0), {"with_out": True}, "keep is 0 but an output cloud is asked for"),
        (params(keep=1), {"with_out": False}, "keep is 1 but there is no place for the output cloud"),
        (params(keep=2), {"with_out": False}, "keep is 2 but there is no place"),
        (params(keep=0), {"with_kept": True, "with_out": False}, "kept is given but keep is 0"),
    ):
        rc, untouched, out = segment(p, **kw)
        assert rc == INVALID and word in message() and untouched and out in (SENTINEL, None), (message(), out)
    assert counters() == before


@pytest.mark.parametrize("fields", [{"distance_threshold": 1e-300}, {"distance_threshold": 1e300}, {"iterations": 1}, {"iterations": 2**20}, {"axis": (0.0, 0.0, 1e-300), "max_angle": np.pi / 2},
                                    {"min_inliers": 2**63}, {"seed": 2**64 - 1}])
def test_parameters_at_their_limits_pass_the_check(fields):
    """no handle can be read here, so acceptance shows through the refusal that stands behind the check of these parameters"""
    rc, untouched, out = segment(params(refit=5, **fields))
    assert rc == INVALID and "refit 5 is not 0 or 1" in message() and untouched


# ---- the host solver of the refit ---------------------------------------------------------------------------------------------------------
def from_sums(x):
    """sga_debug_plane_from_sums over the differences x (k, 3): (status, normal, centroid offset, eigenvalues)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    sx = np.ascontiguousarray(x.sum(axis=0))
    xx = x.T @ x
    s6 = np.array([xx[0, 0], xx[0, 1], xx[0, 2], xx[1, 1], xx[1, 2], xx[2, 2]])
    normal, off, ev = np.full(3, -7.0), np.full(3, -7.0), np.full(3, -7.0)
    rc = sga.load().sga_debug_plane_from_sums(len(x), sx.ctypes.data_as(DP), s6.ctypes.data_as(DP), normal.ctypes.data_as(DP), off.ctypes.data_as(DP), ev.ctypes.data_as(DP))
    return rc, normal, off, ev


def test_the_solver_against_numpy_eigh():
    """200 random inlier sets: slabs of every thickness down to 1e-4 of their extent, in any attitude, 3 .. 2000 points, a quarter of them
    from a cloud 256 km out taken as differences from one of its fp32 records.  Bounds: the normal within 1e-10 rad and the centroid
    offset within 1e-9 m of numpy's — those test_the_solver_against_numpy_svd applies to the same Jacobi routine."""
    g = np.random.default_rng(27)
    worst_angle = worst_off = 0.0
    for case in range(200):
        k = int(g.integers(3, 2000)) if case % 4 else int(g.integers(3, 12))
        ext = 10.0 ** g.uniform(-1, 2)
        thick = ext * 10.0 ** g.uniform(-4, -0.5)
        local = np.column_stack([g.uniform(-ext, ext, k), g.uniform(-0.6 * ext, 0.6 * ext, k), thick * g.standard_normal(k)])
        Q, _ = np.linalg.qr(g.standard_normal((3, 3)))
        pts = local @ Q.T + g.uniform(-ext, ext, 3)
        if case % 4 == 3:  # far out: fp32 records about an origin 256 km away, as differences from the first record
            rec = (pts + np.array([256e3, -100e3, 50.0])).astype(np.float32).astype(np.float64)
            pts = rec - rec[0]
        y = pts - pts.mean(axis=0)
        w, V = np.linalg.eigh(y.T @ y)
        if not (w[1] - w[0] > 1e-6 * w[2]):
            continue  # (an ill-conditioned draw decides nothing about the solver)
        rc, normal, off, ev = from_sums(pts)
        assert rc == 1, case
        ref = V[:, 0] / np.linalg.norm(V[:, 0])
        angle = float(np.arctan2(np.linalg.norm(np.cross(normal, ref)), abs(float(normal @ ref))))
        doff = float(np.abs(off - pts.mean(axis=0)).max())
        worst_angle, worst_off = max(worst_angle, angle), max(worst_off, doff)
        assert abs(np.linalg.norm(normal) - 1.0) < 1e-14
        lead = normal[2] if normal[2] != 0.0 else (normal[1] if normal[1] != 0.0 else normal[0])
        assert lead > 0.0
        assert np.all(np.diff(ev) >= 0.0) and np.allclose(ev, w, rtol=1e-9, atol=1e-12 * w[2])
    print("plane_from_sums against eigh over 200 sets: worst angle %.3e rad, worst offset %.3e m" % (worst_angle, worst_off))
    assert worst_angle < 1e-10 and worst_off < 1e-9


def test_rank_deficient_sums_report_no_refit():
    t = np.linspace(-3.0, 5.0, 40)
    line = np.column_stack([t, 2.0 * t, -0.5 * t])
    rc, normal, off, ev = from_sums(line)
    assert rc == 0 and (normal == -7.0).all() and np.allclose(off, line.mean(axis=0))
    rc, normal, _, _ = from_sums(np.tile([[1.0, 2.0, 3.0]], (7, 1)))  # one point, seven times
    assert rc == 0 and (normal == -7.0).all()
    rc, normal, _, _ = from_sums(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))  # k < 3
    assert rc == 0 and (normal == -7.0).all()
    rc, _, _, _ = from_sums(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, NAN, 0.0]]))
    assert rc == 0
    z3, z6 = np.zeros(3), np.zeros(6)
    assert sga.load().sga_debug_plane_from_sums(0, z3.ctypes.data_as(DP), z6.ctypes.data_as(DP), z3.ctypes.data_as(DP), z3.ctypes.data_as(DP), z3.ctypes.data_as(DP)) == 0
    # and three points in general position do give their plane
    rc, normal, _, _ = from_sums(np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    assert rc == 1 and np.allclose(normal, [0.0, 0.0, 1.0], atol=1e-15)

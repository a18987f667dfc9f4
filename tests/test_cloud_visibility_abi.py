"""The boundary of sga_cloud_visibility without a device: the symbols exist and are bound with the header's
signatures, the ctypes structures have the header's sizes (72 and 40 bytes), sga_visibility_default gives the defaults; null arguments, a
bad image, field of view, range, margin, window, keep / out / kept combination and a non-finite pose are refused before any handle is
read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_overlap_abi.py's technique) — with *out NULL
afterwards and nothing enqueued.  What needs live handles is tests/test_cloud_visibility_gpu.py's."""
import ctypes as C
import math
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
I64, U8, DP = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_double)
FIELDS = ["width", "height", "fov_up", "fov_down", "min_range", "max_range", "margin", "margin_ratio", "window_h", "window_v", "keep", "reserved"]


def message():
    return sga.load().sga_last_error().decode()


def params(**fields):
    p = _lib.VisibilityParams()
    sga.load().sga_visibility_default(C.byref(p))
    for name, value in fields.items():
        setattr(p, name, value)
    return p


def launches():
    v = C.c_ulonglong()
    assert sga.load().sga_debug_cloud_visibility_launches(C.byref(v)) == OK
    return v.value


def call(p, ctx=STAND_IN, cloud=STAND_IN, scan=STAND_IN, T=None, with_out=None, with_kept=False):
    """with_out None: an output cloud is asked for exactly when keep says so"""
    if with_out is None:
        with_out = p is not None and p.keep != 0
    out = C.c_void_p(0xDEAD)
    kept = (C.c_int64 * 4)()
    t16 = None if T is None else np.ascontiguousarray(T, dtype=np.float64).ctypes.data_as(DP)
    rc = sga.load().sga_cloud_visibility(C.c_void_p(ctx), C.c_void_p(cloud), C.c_void_p(scan), t16, None if p is None else C.byref(p), None, None, None, C.cast(kept, I64) if with_kept else None, None,
                                         C.byref(out) if with_out else None)
    return rc, out.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_visibility_default", "sga_cloud_visibility", "sga_debug_cloud_visibility_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _pvp, _pp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_lib.VisibilityParams)
    assert bound["sga_visibility_default"] == (None, [_pp])
    # ctx, map, scan, T, params, state, clearance, range_image, kept, stats, out
    assert bound["sga_cloud_visibility"] == (C.c_int, [_vp, _vp, _vp, DP, _pp, U8, DP, DP, I64, C.POINTER(_lib.VisibilityStats), _pvp])
    assert bound["sga_debug_cloud_visibility_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("cloud_visibility", "cloud_visibility_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.visibility)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_visibility \{(.*?)\} sga_visibility;", text, re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [(t, n.strip()) for t, names in re.findall(r"\b(int|double|size_t)\s+([a-z_, ]+);", body) for n in names.split(",")]
    assert fields == [("int", "width"), ("int", "height"), ("double", "fov_up"), ("double", "fov_down"), ("double", "min_range"), ("double", "max_range"), ("double", "margin"), ("double", "margin_ratio"),
                      ("int", "window_h"), ("int", "window_v"), ("int", "keep"), ("int", "reserved")]
    ctype = {"int": C.c_int, "double": C.c_double}
    assert [(n, t) for n, t in _lib.VisibilityParams._fields_] == [(n, ctype[t]) for t, n in fields] and C.sizeof(_lib.VisibilityParams) == 72
    m = re.search(r"typedef struct sga_visibility_stats \{(.*?)\} sga_visibility_stats;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|size_t)\s+([a-z_, ]+);", m.group(1))
    assert [(t, n.strip()) for t, n in fields] == [("size_t", "points, unobserved, consistent, occluded, seen_through")]
    assert [(n, t) for n, t in _lib.VisibilityStats._fields_] == [(n, C.c_size_t) for n in ("points", "unobserved", "consistent", "occluded", "seen_through")] and C.sizeof(_lib.VisibilityStats) == 40
    assert "void sga_visibility_default(sga_visibility* p);" in text
    assert "int sga_cloud_visibility(sga_context* ctx, const sga_cloud* map, const sga_cloud* scan, const double T[16]" in text
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    assert "int sga_debug_cloud_visibility_launches(unsigned long long* launches);" in debug


def test_defaults():
    p = params()
    assert [n for n, _ in p._fields_] == FIELDS
    assert (p.width, p.height, p.min_range, p.max_range, p.margin, p.margin_ratio, p.window_h, p.window_v, p.keep, p.reserved) == (1024, 64, 0.5, 60.0, 0.2, 0.01, 1, 1, 0, 0)
    assert abs(p.fov_up - math.radians(3.0)) <= 1e-15 and abs(p.fov_down - math.radians(-25.0)) <= 1e-15
    sga.load().sga_visibility_default(None)  # a NULL struct is left alone
    q = api._visibility_params()
    assert bytes(q) == bytes(p)
    q = api._visibility_params("rest", width=128, height=16, fov_up=0.25, max_range=INF, window_h=2)
    assert (q.width, q.height, q.fov_up, q.fov_down, q.max_range, q.window_h, q.window_v, q.keep) == (128, 16, 0.25, p.fov_down, INF, 2, 1, 2)
    assert api._visibility_params("seen_through").keep == 1
    with pytest.raises(ValueError):
        api._visibility_params("both")
    with pytest.raises(TypeError):
        api._visibility_params(None, depth=3)


def test_null_arguments_are_refused():
    before = launches()
    for keep in (0, 1):
        p = params(keep=keep)
        for kw in ({"ctx": 0}, {"cloud": 0}, {"scan": 0}):
            rc, out = call(p, **kw)
            assert rc == INVALID and "null argument" in message(), kw
            if keep:
                assert out is None  # *out = NULL on every failure
    for with_out in (False, True):
        rc, out = call(None, with_out=with_out)
        assert rc == INVALID and "null argument" in message()
        assert out is None or not with_out
    assert launches() == before


IDENTITY = np.eye(4).reshape(16)
HALF_PI = math.pi / 2


def bad_pose(k, v):
    T = IDENTITY.copy()
    T[k] = v
    return T


@pytest.mark.parametrize(
    "fields, kw, word",
    [
        ({"width": 0}, {}, "image"),
        ({"height": 0}, {}, "image"),
        ({"width": -5, "keep": 1}, {}, "image"),
        ({"width": 4097, "height": 4096}, {}, "2^24"),
        ({"width": 1 << 20, "height": 1 << 20}, {}, "2^24"),  # (the product does not fit 32 bits)
        ({"fov_up": NAN}, {}, "fov_up"),
        ({"fov_down": -INF}, {}, "fov_up"),
        ({"fov_up": np.nextafter(HALF_PI, 2.0)}, {}, "fov_up"),
        ({"fov_down": -np.nextafter(HALF_PI, 2.0)}, {}, "fov_up"),
        ({"fov_up": 0.1, "fov_down": 0.1}, {}, "above fov_down"),
        ({"fov_up": -0.2, "fov_down": 0.1, "keep": 2}, {}, "above fov_down"),
        ({"min_range": -0.1}, {}, "min_range"),
        ({"min_range": NAN}, {}, "min_range"),
        ({"min_range": INF, "max_range": INF}, {}, "min_range"),
        ({"max_range": NAN}, {}, "max_range"),
        ({"min_range": 2.0, "max_range": 1.0}, {}, "max_range"),
        ({"margin": -1.0}, {}, "margin"),
        ({"margin": INF}, {}, "margin"),
        ({"margin_ratio": NAN}, {}, "margin"),
        ({"margin_ratio": -0.01, "keep": 1}, {}, "margin"),
        ({"window_h": -1}, {}, "window"),
        ({"window_h": 17}, {}, "window"),
        ({"window_v": -1}, {}, "window"),
        ({"window_v": 17}, {}, "window"),
        ({"keep": 3}, {"with_out": True}, "keep 3"),
        ({"keep": -1}, {"with_out": True}, "keep -1"),
        ({"keep": 3}, {"with_out": False}, "keep 3"),
        ({"keep": 0}, {"with_out": True}, "keep is 0 but an output cloud"),
        ({"keep": 1}, {"with_out": False}, "no place for the output cloud"),
        ({"keep": 2}, {"with_out": False}, "no place for the output cloud"),
        ({"keep": 0}, {"with_kept": True}, "kept is given but keep is 0"),
        ({}, {"T": bad_pose(0, NAN)}, "non-finite entry"),
        ({}, {"T": bad_pose(13, INF)}, "non-finite entry"),
        ({"keep": 1}, {"T": bad_pose(15, -INF)}, "non-finite entry"),
    ],
)
def test_bad_arguments_are_refused_before_a_handle_is_read(fields, kw, word):
    before = launches()
    rc, out = call(params(**fields), **kw)  # (the stand-in handles would fault if they were read)
    assert rc == INVALID, message()
    if kw.get("with_out", fields.get("keep", 0) != 0):
        assert out is None
    assert word in message(), message()
    assert launches() == before


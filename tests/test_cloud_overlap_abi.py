"""The boundary of sga_cloud_overlap without a device: the symbols exist and are bound with the header's
signatures, the ctypes structures have the header's sizes (16 and 40 bytes), sga_overlap_default gives the defaults; null arguments, a bad
keep / out / kept combination, a bad max_distance and a non-finite pose are refused before any handle is read — the handles are stand-ins
at an address nothing is mapped at (tests/test_cloud_outliers_abi.py's technique) — with *out NULL afterwards and nothing enqueued.  What
needs live handles is tests/test_cloud_overlap_gpu.py's."""
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
I64 = C.POINTER(C.c_int64)


def message():
    return sga.load().sga_last_error().decode()


def params(**fields):
    p = _lib.OverlapParams()
    sga.load().sga_overlap_default(C.byref(p))
    for name, value in fields.items():
        setattr(p, name, value)
    return p


def launches():
    v = C.c_ulonglong()
    assert sga.load().sga_debug_cloud_overlap_launches(C.byref(v)) == OK
    return v.value


def call(p, ctx=STAND_IN, cloud=STAND_IN, target=STAND_IN, T=None, with_out=None, with_kept=False):
    """with_out None: an output cloud is asked for exactly when keep says so"""
    if with_out is None:
        with_out = p is not None and p.keep != 0
    out = C.c_void_p(0xDEAD)
    kept = (C.c_int64 * 4)()
    t16 = None if T is None else np.ascontiguousarray(T, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))
    rc = sga.load().sga_cloud_overlap(C.c_void_p(ctx), C.c_void_p(cloud), C.c_void_p(target), t16, None if p is None else C.byref(p), None, None, C.cast(kept, I64) if with_kept else None, None,
                                      C.byref(out) if with_out else None)
    return rc, out.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_overlap_default", "sga_cloud_overlap", "sga_debug_cloud_overlap_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _pvp, _dp, _pp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_double), C.POINTER(_lib.OverlapParams)
    assert bound["sga_overlap_default"] == (None, [_pp])
    # ctx, cloud, target, T, params, dist, nearest, kept, stats, out
    assert bound["sga_cloud_overlap"] == (C.c_int, [_vp, _vp, _vp, _dp, _pp, _dp, I64, I64, C.POINTER(_lib.OverlapStats), _pvp])
    assert bound["sga_debug_cloud_overlap_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("cloud_overlap", "cloud_overlap_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.overlap)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_overlap \{(.*?)\} sga_overlap;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|size_t)\s+([a-z_, ]+);", m.group(1))
    assert [(t, n.strip()) for t, n in fields] == [("double", "max_distance"), ("int", "keep"), ("int", "reserved")]
    assert [n for n, _ in _lib.OverlapParams._fields_] == ["max_distance", "keep", "reserved"] and C.sizeof(_lib.OverlapParams) == 16
    m = re.search(r"typedef struct sga_overlap_stats \{(.*?)\} sga_overlap_stats;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|size_t)\s+([a-z_, ]+);", m.group(1))
    assert [(t, n.strip()) for t, n in fields] == [("size_t", "points, matched"), ("double", "fitness"), ("double", "rmse"), ("double", "mean_distance")]
    assert [n for n, _ in _lib.OverlapStats._fields_] == ["points", "matched", "fitness", "rmse", "mean_distance"] and C.sizeof(_lib.OverlapStats) == 40
    assert "void sga_overlap_default(sga_overlap* p);" in text
    assert "int sga_cloud_overlap(sga_context* ctx, const sga_cloud* cloud, const sga_index* target, const double T[16]" in text
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    assert "int sga_debug_cloud_overlap_launches(unsigned long long* launches);" in debug


def test_defaults():
    p = params()
    assert (p.max_distance, p.keep, p.reserved) == (1.0, 0, 0)
    sga.load().sga_overlap_default(None)  # a NULL struct is left alone
    q = api._overlap_params()
    assert (q.max_distance, q.keep) == (1.0, 0)
    q = api._overlap_params(0.25, "unmatched")
    assert (q.max_distance, q.keep) == (0.25, 2)
    assert api._overlap_params(0.5, "matched").keep == 1
    with pytest.raises(ValueError):
        api._overlap_params(1.0, "both")


def test_null_arguments_are_refused():
    before = launches()
    for keep in (0, 1):
        p = params(keep=keep)
        for kw in ({"ctx": 0}, {"cloud": 0}, {"target": 0}):
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


def bad_pose(k, v):
    T = IDENTITY.copy()
    T[k] = v
    return T


@pytest.mark.parametrize(
    "fields, kw, word",
    [
        ({"keep": 3}, {"with_out": True}, "keep 3"),
        ({"keep": -1}, {"with_out": True}, "keep -1"),
        ({"keep": 3}, {"with_out": False}, "keep 3"),
        ({"keep": 0}, {"with_out": True}, "keep is 0 but an output cloud"),
        ({"keep": 1}, {"with_out": False}, "no place for the output cloud"),
        ({"keep": 2}, {"with_out": False}, "no place for the output cloud"),
        ({"keep": 0}, {"with_kept": True}, "kept is given but keep is 0"),
        ({"max_distance": 0.0}, {}, "max_distance"),
        ({"max_distance": -1.0}, {}, "max_distance"),
        ({"max_distance": NAN}, {}, "max_distance"),
        ({"max_distance": -INF}, {}, "max_distance"),
        ({"max_distance": NAN, "keep": 2}, {}, "max_distance"),
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

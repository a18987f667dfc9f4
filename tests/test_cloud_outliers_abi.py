"""The boundary of sga_cloud_remove_outliers without a device: the symbols exist and are bound with the header's
signatures, the ctypes structures have the header's sizes, sga_outlier_filter_default gives the defaults; null arguments and every bad
field of a filter are refused before any handle is read — the handles are stand-ins at an address nothing is mapped at
(tests/test_cloud_crop_abi.py's technique) — with *out NULL afterwards and nothing enqueued.  What needs live clouds is
tests/test_cloud_outliers_gpu.py's."""
import ctypes as C
import os
import re

import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
INF, NAN = float("inf"), float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def message():
    return sga.load().sga_last_error().decode()


def default_filter(**fields):
    f = _lib.OutlierFilter()
    sga.load().sga_outlier_filter_default(C.byref(f))
    for name, value in fields.items():
        setattr(f, name, value)
    return f


def launches():
    v = C.c_ulonglong()
    assert sga.load().sga_debug_cloud_outliers_launches(C.byref(v)) == OK
    return v.value


def call(f, ctx=STAND_IN, cloud=STAND_IN, tree=None, with_out=True):
    out = C.c_void_p(0xDEAD)
    rc = sga.load().sga_cloud_remove_outliers(C.c_void_p(ctx), C.c_void_p(cloud), tree, None if f is None else C.byref(f), None, None, None, C.byref(out) if with_out else None)
    return rc, out.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_outlier_filter_default", "sga_cloud_remove_outliers", "sga_debug_cloud_outliers_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _pvp, _pf = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_lib.OutlierFilter)
    assert bound["sga_outlier_filter_default"] == (None, [_pf])
    # ctx, cloud, kdtree, filter, kept, stat, stats, out
    assert bound["sga_cloud_remove_outliers"] == (C.c_int, [_vp, _vp, _vp, _pf, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(_lib.OutlierStats), _pvp])
    assert bound["sga_debug_cloud_outliers_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("remove_outliers", "cloud_outliers_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.without_outliers)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_outlier_filter \{(.*?)\} sga_outlier_filter;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|size_t)\s+([a-z_, ]+);", m.group(1))
    assert [(t, n.strip()) for t, n in fields] == [("int", "mode"), ("int", "k"), ("double", "std_mul"), ("double", "radius")]
    assert [n for n, _ in _lib.OutlierFilter._fields_] == ["mode", "k", "std_mul", "radius"] and C.sizeof(_lib.OutlierFilter) == 24
    m = re.search(r"typedef struct sga_outlier_stats \{(.*?)\} sga_outlier_stats;", text, re.S)
    assert m is not None and "double mean, stddev, threshold;" in m.group(1) and "size_t kept;" in m.group(1)
    assert [n for n, _ in _lib.OutlierStats._fields_] == ["mean", "stddev", "threshold", "kept"] and C.sizeof(_lib.OutlierStats) == 32
    assert "int sga_cloud_remove_outliers(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree" in text
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    assert "int sga_debug_cloud_outliers_launches(unsigned long long* launches);" in debug


def test_defaults():
    f = default_filter()
    assert (f.mode, f.k, f.std_mul, f.radius) == (0, 10, 1.0, 0.0)
    sga.load().sga_outlier_filter_default(None)  # a NULL filter is left alone
    g = api._outlier_filter()
    assert (g.mode, g.k, g.std_mul) == (0, 10, 1.0)
    g = api._outlier_filter(5, radius=0.5)
    assert (g.mode, g.k, g.radius) == (1, 5, 0.5)


def test_null_arguments_are_refused():
    before = launches()
    f = default_filter()
    for kw in ({"ctx": 0}, {"cloud": 0}, {"with_out": False}):
        rc, out = call(f, **kw)
        assert rc == INVALID and "null argument" in message(), kw
        if kw.get("with_out", True):
            assert out is None  # *out = NULL on every failure
    rc, out = call(None)
    assert rc == INVALID and out is None and "null argument" in message()
    assert launches() == before


@pytest.mark.parametrize(
    "fields, word",
    [
        ({"mode": 2}, "mode 2"),
        ({"mode": -1}, "mode -1"),
        ({"k": 0}, "k must be in [1,63]"),
        ({"k": -3}, "k must be in [1,63]"),
        ({"k": 64}, "k must be in [1,63]"),
        ({"std_mul": -0.5}, "std_mul"),
        ({"std_mul": NAN}, "std_mul"),
        ({"std_mul": INF}, "std_mul"),
        ({"mode": 1, "radius": 0.0}, "radius"),
        ({"mode": 1, "radius": -1.0}, "radius"),
        ({"mode": 1, "radius": NAN}, "radius"),
        ({"mode": 1, "radius": INF}, "radius"),
        ({"mode": 1, "radius": 1.0, "k": 64}, "k must be in [1,63]"),
    ],
)
def test_a_bad_filter_is_refused_before_a_handle_is_read(fields, word):
    before = launches()
    rc, out = call(default_filter(**fields))  # (the stand-in handles would fault if they were read)
    assert rc == INVALID and out is None
    assert word in message(), message()
    assert launches() == before


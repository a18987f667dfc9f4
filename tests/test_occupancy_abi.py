"""The boundary of sga_occupancy_*  without a device: the symbols exist and are bound with the header's signatures,
the ctypes structures have the header's sizes (64, 48 and 40 bytes), sga_occupancy_params_default gives OctoMap's log-odds; null
arguments, bad grid parameters, ranges, modes, thresholds, masks, out / kept combinations and non-finite poses are refused before any
handle is read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_overlap_abi.py's technique) — with *out
NULL afterwards and nothing enqueued.  What needs live handles is tests/test_occupancy_gpu.py's."""
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
I64, U8, U32, DP, FP = C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_float)
SYMBOLS = ["sga_occupancy_params_default", "sga_occupancy_create", "sga_occupancy_destroy", "sga_occupancy_get", "sga_occupancy_clear", "sga_occupancy_integrate", "sga_occupancy_classify", "sga_occupancy_stats",
           "sga_occupancy_export", "sga_occupancy_download", "sga_debug_occupancy_launches", "sga_debug_occupancy_waits"]


def message():
    return sga.load().sga_last_error().decode()


def counters():
    a, b = C.c_ulonglong(), C.c_ulonglong()
    assert sga.load().sga_debug_occupancy_launches(C.byref(a)) == OK and sga.load().sga_debug_occupancy_waits(C.byref(b)) == OK
    return a.value, b.value


def params(**fields):
    p = _lib.OccupancyParams()
    sga.load().sga_occupancy_params_default(C.byref(p))
    p.leaf = 0.5
    for k in range(3):
        p.dims[k] = 8
    for name, value in fields.items():
        if name in ("origin", "dims"):
            for k in range(3):
                getattr(p, name)[k] = value[k]
        else:
            setattr(p, name, value)
    return p


def t16(T):
    return None if T is None else np.ascontiguousarray(T, dtype=np.float64).ctypes.data_as(DP)


IDENTITY = np.eye(4).reshape(16)


def bad_pose(k, v):
    T = IDENTITY.copy()
    T[k] = v
    return T


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _pvp, _pp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_lib.OccupancyParams)
    _pc = C.POINTER(_lib.OccupancyCounts)
    assert bound["sga_occupancy_params_default"] == (None, [_pp])
    assert bound["sga_occupancy_create"] == (C.c_int, [_vp, _pp, _pvp])
    assert bound["sga_occupancy_get"] == (C.c_int, [_vp, _pp, C.POINTER(C.c_uint64)])
    # ctx, grid, scan, T, min_range, max_range, mode, stats
    assert bound["sga_occupancy_integrate"] == (C.c_int, [_vp, _vp, _vp, DP, C.c_double, C.c_double, C.c_int, C.POINTER(_lib.OccupancyScanStats)])
    # ctx, grid, cloud, T, threshold, keep_mask, state, kept, counts, out
    assert bound["sga_occupancy_classify"] == (C.c_int, [_vp, _vp, _vp, DP, C.c_double, C.c_int, U8, I64, _pc, _pvp])
    assert bound["sga_occupancy_stats"] == (C.c_int, [_vp, _vp, C.c_double, _pc])
    # ctx, grid, threshold, which_mask, capacity, indices, log_odds, count, out
    assert bound["sga_occupancy_export"] == (C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_size_t, I64, FP, C.POINTER(C.c_size_t), _pvp])
    assert bound["sga_occupancy_download"] == (C.c_int, [_vp, _vp, U32, FP])
    for name in ("OccupancyGrid", "occupancy_launches", "occupancy_waits"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    for name in ("integrate", "classify", "stats", "occupied_cloud", "export", "download", "clear"):
        assert callable(getattr(sga.OccupancyGrid, name)), name


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_occupancy_params \{(.*?)\} sga_occupancy_params;", text, re.S)
    assert m is not None
    fields = [(t, n.strip()) for t, names in re.findall(r"\b(int|double|float)\s+([a-z_0-9\[\], ]+);", m.group(1)) for n in names.split(",")]
    assert fields == [("double", "origin[3]"), ("double", "leaf"), ("int", "dims[3]"), ("int", "reserved"), ("float", "l_hit"), ("float", "l_miss"), ("float", "l_min"), ("float", "l_max")]
    ctype = {"double": C.c_double, "int": C.c_int, "float": C.c_float}
    want = [(n[:-3], ctype[t] * 3) if n.endswith("[3]") else (n, ctype[t]) for t, n in fields]
    assert [(n, t) for n, t in _lib.OccupancyParams._fields_] == want and C.sizeof(_lib.OccupancyParams) == 64
    m = re.search(r"typedef struct sga_occupancy_scan_stats \{(.*?)\} sga_occupancy_scan_stats;", text, re.S)
    assert m is not None and [n.strip() for n in re.search(r"size_t ([a-z_, ]+);", m.group(1)).group(1).split(",")] == [n for n, _ in _lib.OccupancyScanStats._fields_]
    assert all(t is C.c_size_t for _, t in _lib.OccupancyScanStats._fields_) and C.sizeof(_lib.OccupancyScanStats) == 48
    m = re.search(r"typedef struct sga_occupancy_counts \{(.*?)\} sga_occupancy_counts;", text, re.S)
    assert m is not None and re.findall(r"\b(size_t|uint64_t)\s+([a-z_, ]+);", m.group(1)) == [("size_t", "total, unknown, free, occupied"), ("uint64_t", "epoch")]
    assert [(n, t) for n, t in _lib.OccupancyCounts._fields_] == [(n, C.c_size_t) for n in ("total", "unknown", "free", "occupied")] + [("epoch", C.c_uint64)] and C.sizeof(_lib.OccupancyCounts) == 40
    for name in SYMBOLS[:-2]:
        assert re.search(r"\b(int|void) %s\(" % name, text), name
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    assert "int sga_debug_occupancy_launches(unsigned long long* launches);" in debug and "int sga_debug_occupancy_waits(unsigned long long* waits);" in debug
    hpp = open(os.path.join(ROOT, "include", "small_gicp_amd.hpp")).read()
    assert "struct OccupancyParams" in hpp and "class OccupancyGrid" in hpp


def test_defaults():
    p = _lib.OccupancyParams()
    sga.load().sga_occupancy_params_default(C.byref(p))
    assert list(p.origin) == [0.0, 0.0, 0.0] and p.leaf == 0.0 and list(p.dims) == [0, 0, 0] and p.reserved == 0
    f32 = np.float32
    assert (f32(p.l_hit), f32(p.l_miss), f32(p.l_min), f32(p.l_max)) == (f32(0.85), f32(-0.4), f32(-2.0), f32(3.5))  # OctoMap's
    sga.load().sga_occupancy_params_default(None)  # a NULL struct is left alone
    assert api._state_mask(None, "keep") == 0 and api._state_mask("occupied", "keep") == 4 and api._state_mask(("unknown", "occupied"), "keep") == 5 and api._state_mask(3, "keep") == 3
    with pytest.raises(ValueError):
        api._state_mask("solid", "keep")


def create(p, ctx=STAND_IN, with_out=True):
    out = C.c_void_p(0xDEAD)
    rc = sga.load().sga_occupancy_create(C.c_void_p(ctx), None if p is None else C.byref(p), C.byref(out) if with_out else None)
    return rc, out.value


@pytest.mark.parametrize(
    "fields, word",
    [
        ({"origin": (NAN, 0.0, 0.0)}, "origin"),
        ({"origin": (0.0, 0.0, -INF)}, "origin"),
        ({"leaf": 0.0}, "leaf"),
        ({"leaf": -0.5}, "leaf"),
        ({"leaf": NAN}, "leaf"),
        ({"leaf": INF}, "leaf"),
        ({"dims": (0, 8, 8)}, "each must be >= 1"),
        ({"dims": (8, -1, 8)}, "each must be >= 1"),
        ({"dims": (513, 512, 512)}, "2^27"),
        ({"dims": (1 << 30, 1 << 30, 1 << 30)}, "2^27"),  # (the product does not fit 64 bits)
        ({"l_hit": NAN}, "finite"),
        ({"l_max": INF}, "finite"),
        ({"l_hit": 0.0}, "l_hit"),
        ({"l_hit": -0.85}, "l_hit"),
        ({"l_miss": 0.0}, "l_miss"),
        ({"l_miss": 0.4}, "l_miss"),
        ({"l_min": 3.5}, "l_min"),
        ({"l_min": 1.0, "l_max": -1.0}, "l_min"),
    ],
)
def test_create_refuses_bad_parameters_before_the_context_is_read(fields, word):
    before = counters()
    rc, out = create(params(**fields))  # (the stand-in context would fault if it were read)
    assert rc == INVALID and out is None, message()
    assert word in message(), message()
    assert counters() == before


def test_null_arguments_are_refused():
    lib = sga.load()
    before = counters()
    vp = C.c_void_p
    for kw in ({"ctx": 0}, {"p": None}, {"with_out": False}):
        rc, out = create(kw.get("p", params()), ctx=kw.get("ctx", STAND_IN), with_out=kw.get("with_out", True))
        assert rc == INVALID and "null argument" in message(), kw
        assert out is None or not kw.get("with_out", True)
    assert lib.sga_occupancy_get(None, C.byref(params()), None) == INVALID and "null argument" in message()
    assert lib.sga_occupancy_get(vp(STAND_IN), None, None) == INVALID and "null argument" in message()
    assert lib.sga_occupancy_clear(None, vp(STAND_IN)) == INVALID and lib.sga_occupancy_clear(vp(STAND_IN), None) == INVALID
    for ctx, grid, scan in ((0, STAND_IN, STAND_IN), (STAND_IN, 0, STAND_IN), (STAND_IN, STAND_IN, 0)):
        assert lib.sga_occupancy_integrate(vp(ctx), vp(grid), vp(scan), None, 0.5, 12.0, 0, None) == INVALID and "null argument" in message()
        out = vp(0xDEAD)
        assert lib.sga_occupancy_classify(vp(ctx), vp(grid), vp(scan), None, 0.0, 4, None, None, None, C.byref(out)) == INVALID and "null argument" in message()
        assert out.value is None  # *out = NULL on every failure
    counts, n = _lib.OccupancyCounts(), C.c_size_t()
    for ctx, grid in ((0, STAND_IN), (STAND_IN, 0)):
        assert lib.sga_occupancy_stats(vp(ctx), vp(grid), 0.0, C.byref(counts)) == INVALID and "null argument" in message()
        out = vp(0xDEAD)
        assert lib.sga_occupancy_export(vp(ctx), vp(grid), 0.0, 4, 0, None, None, C.byref(n), C.byref(out)) == INVALID and "null argument" in message()
        assert out.value is None
        stamp = (C.c_uint32 * 1)()
        assert lib.sga_occupancy_download(vp(ctx), vp(grid), stamp, None) == INVALID and "null argument" in message()
    assert lib.sga_occupancy_stats(vp(STAND_IN), vp(STAND_IN), 0.0, None) == INVALID and "null argument" in message()
    assert lib.sga_occupancy_export(vp(STAND_IN), vp(STAND_IN), 0.0, 4, 0, None, None, None, None) == INVALID and "null argument" in message()
    assert lib.sga_occupancy_download(vp(STAND_IN), vp(STAND_IN), None, None) == INVALID and "null argument" in message()
    assert lib.sga_occupancy_destroy(None) == OK  # as the other destroy calls: nothing to do
    assert counters() == before


@pytest.mark.parametrize(
    "kw, word",
    [
        ({"min_range": -0.1}, "min_range"),
        ({"min_range": NAN}, "min_range"),
        ({"min_range": INF, "max_range": INF}, "min_range"),
        ({"max_range": NAN}, "max_range"),
        ({"max_range": INF}, "max_range"),
        ({"min_range": 2.0, "max_range": 1.0}, "max_range"),
        ({"mode": 2}, "mode 2"),
        ({"mode": -1}, "mode -1"),
        ({"T": bad_pose(0, NAN)}, "non-finite entry"),
        ({"T": bad_pose(13, INF)}, "non-finite entry"),
        ({"T": bad_pose(15, -INF)}, "non-finite entry"),
    ],
)
def test_integrate_refuses_bad_arguments_before_a_handle_is_read(kw, word):
    before = counters()
    st = _lib.OccupancyScanStats()
    vp = C.c_void_p
    rc = sga.load().sga_occupancy_integrate(vp(STAND_IN), vp(STAND_IN), vp(STAND_IN), t16(kw.get("T")), kw.get("min_range", 0.5), kw.get("max_range", 12.0), kw.get("mode", 0), C.byref(st))
    assert rc == INVALID and word in message(), message()
    assert counters() == before


@pytest.mark.parametrize(
    "kw, word",
    [
        ({"threshold": NAN}, "threshold"),
        ({"keep_mask": 8, "with_out": True}, "keep_mask 8"),
        ({"keep_mask": -1, "with_out": True}, "keep_mask -1"),
        ({"keep_mask": 0, "with_out": True}, "keep_mask is 0 but an output cloud"),
        ({"keep_mask": 5, "with_out": False}, "no place for the output cloud"),
        ({"keep_mask": 0, "with_out": False, "with_kept": True}, "kept is given but keep_mask is 0"),
        ({"keep_mask": 4, "with_out": True, "T": bad_pose(5, NAN)}, "non-finite entry"),
        ({"keep_mask": 0, "with_out": False, "T": bad_pose(12, INF)}, "non-finite entry"),
    ],
)
def test_classify_refuses_bad_arguments_before_a_handle_is_read(kw, word):
    before = counters()
    out, kept, vp = C.c_void_p(0xDEAD), (C.c_int64 * 4)(), C.c_void_p
    rc = sga.load().sga_occupancy_classify(vp(STAND_IN), vp(STAND_IN), vp(STAND_IN), t16(kw.get("T")), kw.get("threshold", 0.0), kw.get("keep_mask", 0), None, C.cast(kept, I64) if kw.get("with_kept") else None, None,
                                           C.byref(out) if kw.get("with_out") else None)
    assert rc == INVALID and word in message(), message()
    if kw.get("with_out"):
        assert out.value is None
    assert counters() == before


def test_stats_and_export_refuse_bad_arguments_before_a_handle_is_read():
    before = counters()
    lib, vp = sga.load(), C.c_void_p
    counts, n = _lib.OccupancyCounts(), C.c_size_t()
    assert lib.sga_occupancy_stats(vp(STAND_IN), vp(STAND_IN), NAN, C.byref(counts)) == INVALID and "threshold" in message()
    for mask, word in ((0, "which_mask 0"), (8, "which_mask 8"), (-4, "which_mask -4")):
        out = vp(0xDEAD)
        assert lib.sga_occupancy_export(vp(STAND_IN), vp(STAND_IN), 0.0, mask, 0, None, None, C.byref(n), C.byref(out)) == INVALID and word in message(), message()
        assert out.value is None
    out = vp(0xDEAD)
    assert lib.sga_occupancy_export(vp(STAND_IN), vp(STAND_IN), NAN, 4, 0, None, None, C.byref(n), C.byref(out)) == INVALID and "threshold" in message() and out.value is None
    assert counters() == before

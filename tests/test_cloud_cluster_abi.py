"""The boundary of the fixed-radius calls without a device: the symbols exist and are bound with the header's
signatures, the ctypes structures have the header's fields and sizes (24, 32, 32 and 64 bytes), sga_cluster_params_default gives the
defaults; null arguments and parameters outside their ranges are refused before any handle is read — the handles are stand-ins at an
address nothing is mapped at (tests/test_places_abi.py's technique) — with the outputs untouched and nothing enqueued.  What needs live
handles (another device, non-finite records, a tree of another cloud) is tests/test_cloud_cluster_gpu.py's."""
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
DP, I32, I64 = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
VP, PVP, ULL = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong)
PCP, PCR, PROW, PRR = C.POINTER(_lib.ClusterParams), C.POINTER(_lib.ClusterResult), C.POINTER(_lib.ClusterRow), C.POINTER(_lib.RadiusResult)
SENTINEL = 0xDEAD


def message():
    return sga.load().sga_last_error().decode()


def params(**fields):
    p = _lib.ClusterParams()
    sga.load().sga_cluster_params_default(C.byref(p))
    for name, value in fields.items():
        setattr(p, name, value)
    return p


def counters():
    return [sga.cloud_cluster_launches(), sga.radius_search_launches(), sga.radius_waits()]


def cluster(p, ctx=STAND_IN, cloud=STAND_IN, rows=0, with_table=None, with_kept=False, with_out=None):
    """-> (status, labels untouched, result untouched, out untouched)"""
    with_table = rows > 0 if with_table is None else with_table
    with_out = (p is not None and p.keep != 0) if with_out is None else with_out
    labels = np.full(4, -7, np.int32)
    table = (_lib.ClusterRow * 4)()
    kept = np.full(4, -7, np.int64)
    res = _lib.ClusterResult(SENTINEL, SENTINEL, SENTINEL, SENTINEL)
    out = C.c_void_p(SENTINEL)
    rc = sga.load().sga_cloud_cluster(C.c_void_p(ctx), C.c_void_p(cloud), None, None if p is None else C.byref(p), labels.ctypes.data_as(I32), table if with_table else None, rows,
                                      kept.ctypes.data_as(I64) if with_kept else None, C.byref(res), C.byref(out) if with_out else None)
    untouched = (labels == -7).all() and (kept == -7).all() and res.clusters == SENTINEL and res.rows == SENTINEL
    return rc, untouched, out.value


def search(radius=0.5, ctx=STAND_IN, tree=STAND_IN, cloud=STAND_IN, with_counts=True, with_result=True, offsets=False, indices=False, sq=False):
    counts, offs, idx, d2 = np.full(4, -7, np.int64), np.full(5, -7, np.int64), np.full(4, -7, np.int64), np.full(4, -7.0)
    res = _lib.RadiusResult(SENTINEL, SENTINEL, 7, 7)
    rc = sga.load().sga_index_radius_search(C.c_void_p(ctx), C.c_void_p(tree), C.c_void_p(cloud), radius, 4, counts.ctypes.data_as(I64) if with_counts else None, offs.ctypes.data_as(I64) if offsets else None,
                                            idx.ctypes.data_as(I64) if indices else None, d2.ctypes.data_as(DP) if sq else None, C.byref(res) if with_result else None)
    untouched = (counts == -7).all() and (offs == -7).all() and (idx == -7).all() and (d2 == -7.0).all() and res.total == SENTINEL and res.overflow == 7
    return rc, untouched


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    want = {
        "sga_index_radius_search": (C.c_int, [VP, VP, VP, C.c_double, C.c_size_t, I64, I64, I64, DP, PRR]),
        "sga_cluster_params_default": (None, [PCP]),
        "sga_cloud_cluster": (C.c_int, [VP, VP, VP, PCP, I32, PROW, C.c_size_t, I64, PCR, PVP]),
        "sga_debug_radius_search_launches": (C.c_int, [ULL]),
        "sga_debug_cloud_cluster_launches": (C.c_int, [ULL]),
        "sga_debug_radius_waits": (C.c_int, [ULL]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert bound.get(name) == sig, name
    for name in ("cluster_cloud", "cloud_cluster_launches", "radius_search_launches", "radius_waits"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.clusters) and callable(sga.KdTree.radius_search)
    from small_gicp_amd import odometry

    assert callable(odometry.run_synthetic_movers)


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

    assert same(fields_of("sga_radius_result"), _lib.RadiusResult._fields_) and [n for n, _ in _lib.RadiusResult._fields_] == ["total", "written", "overflow", "reserved"]
    assert same(fields_of("sga_cluster_params"), _lib.ClusterParams._fields_) and [n for n, _ in _lib.ClusterParams._fields_] == ["radius", "min_points", "keep", "min_size", "max_size"]
    assert same(fields_of("sga_cluster_result"), _lib.ClusterResult._fields_) and [n for n, _ in _lib.ClusterResult._fields_] == ["clusters", "noise", "dropped", "rows"]
    assert same(fields_of("sga_cluster_row"), _lib.ClusterRow._fields_) and [n for n, _ in _lib.ClusterRow._fields_] == ["seed", "size", "lo", "hi"]
    assert (C.sizeof(_lib.RadiusResult), C.sizeof(_lib.ClusterParams), C.sizeof(_lib.ClusterResult), C.sizeof(_lib.ClusterRow)) == (24, 32, 32, 64)
    assert api.CLUSTER_ROW_DTYPE.itemsize == 64 and [api.CLUSTER_ROW_DTYPE.fields[n][1] for n in ("seed", "size", "lo", "hi")] == [0, 8, 16, 40]
    for decl in (
        "void sga_cluster_params_default(sga_cluster_params* p);",
        "int sga_cloud_cluster(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree",
        "int sga_index_radius_search(sga_context* ctx, const sga_index* kdtree, const sga_cloud* queries, double radius, size_t capacity, int64_t* counts",
    ):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    for name in ("sga_debug_radius_search_launches(unsigned long long* launches)", "sga_debug_cloud_cluster_launches(unsigned long long* launches)", "sga_debug_radius_waits(unsigned long long* waits)"):
        assert "int %s;" % name in debug, name


def test_defaults():
    p = params()
    assert (p.radius, p.min_points, p.keep, p.min_size, p.max_size) == (0.5, 1, 0, 1, 0)
    sga.load().sga_cluster_params_default(None)  # a NULL struct is left alone
    assert bytes(api._cluster_params()) == bytes(p)
    q = api._cluster_params(0.25, min_points=4, min_size=10, max_size=500, keep="rest")
    assert (q.radius, q.min_points, q.keep, q.min_size, q.max_size) == (0.25, 4, 2, 10, 500)
    assert api._cluster_params(q) is q
    with pytest.raises(ValueError):
        api._cluster_params(0.5, keep="everything")


def test_null_arguments_are_refused():
    before = counters()
    p = params()
    for rc, untouched, out in (cluster(p, ctx=0), cluster(p, cloud=0), cluster(None)):
        assert rc == INVALID and "null argument" in message() and untouched and out == SENTINEL
    for kw in ({"ctx": 0}, {"tree": 0}, {"cloud": 0}, {"with_counts": False}, {"with_result": False}):
        rc, untouched = search(**kw)
        assert rc == INVALID and "null argument" in message() and untouched, kw
    for kw in ({"offsets": True}, {"offsets": True, "indices": True}, {"offsets": True, "sq": True}):
        rc, untouched = search(**kw)
        assert rc == INVALID and "without room for indices and sq_dists" in message() and untouched, kw
    assert sga.load().sga_debug_cloud_cluster_launches(None) == INVALID and sga.load().sga_debug_radius_search_launches(None) == INVALID and sga.load().sga_debug_radius_waits(None) == INVALID
    assert counters() == before


BAD_PARAMS = [
    ({"radius": 0.0}, "radius must be finite and > 0"),
    ({"radius": -0.5}, "radius must be finite and > 0"),
    ({"radius": INF}, "radius must be finite and > 0"),
    ({"radius": NAN}, "radius must be finite and > 0"),
    ({"min_points": 0}, "min_points 0 is below 1"),
    ({"min_points": -3}, "min_points -3 is below 1"),
    ({"min_size": 0}, "min_size 0 is below 1"),
    ({"max_size": -1}, "max_size -1 is negative"),
    ({"min_size": 11, "max_size": 10}, "min_size 11 is above max_size 10"),
    ({"keep": 3}, "keep 3 is not 0"),
    ({"keep": -1}, "keep -1 is not 0"),
]


@pytest.mark.parametrize("fields, word", BAD_PARAMS)
def test_bad_parameters_are_refused_before_a_handle_is_read(fields, word):
    before = counters()
    rc, untouched, out = cluster(params(**fields), with_out=False)  # (the stand-in handles would fault if they were read)
    assert rc == INVALID and word in message() and untouched, message()
    assert counters() == before


@pytest.mark.parametrize("radius", [0.0, -1.0, INF, NAN])
def test_a_bad_radius_is_refused_by_the_search_before_a_handle_is_read(radius):
    before = counters()
    rc, untouched = search(radius=radius)
    assert rc == INVALID and "radius must be finite and > 0" in message() and untouched
    assert counters() == before


def test_keep_and_the_table_must_agree_with_their_outputs():
    before = counters()
    for p, kw, word in (
        (params(keep=0), {"with_out": True}, "keep is 0 but an output cloud is asked for"),
        (params(keep=1), {"with_out": False}, "keep is 1 but there is no place for the output cloud"),
        (params(keep=2), {"with_out": False}, "keep is 2 but there is no place"),
        (params(keep=0), {"with_kept": True, "with_out": False}, "kept is given but keep is 0"),
        (params(), {"rows": 4, "with_table": False}, "a table needs a capacity"),
        (params(), {"rows": 0, "with_table": True}, "a table needs a capacity"),
    ):
        rc, untouched, out = cluster(p, **kw)
        assert rc == INVALID and word in message() and untouched and out in (SENTINEL, None), (message(), out)
    assert counters() == before


@pytest.mark.parametrize("fields", [{"radius": 1e-300}, {"radius": 1e300}, {"min_points": 1}, {"min_points": 2**31 - 1}])
def test_parameters_at_their_limits_pass_the_check(fields):
    """no handle can be read here, so acceptance shows through the refusal that stands behind the check of these parameters"""
    rc, untouched, out = cluster(params(min_size=11, max_size=10, **fields))
    assert rc == INVALID and "min_size 11 is above max_size 10" in message() and untouched

"""The boundary of the place-recognition calls without a device: the symbols exist and are bound with the
header's signatures, the ctypes structures have the header's fields and sizes (24 and 24 bytes), sga_place_params_default gives the
defaults; null arguments, parameters outside their ranges, a non-finite center and a k outside [1, 32] are refused before any handle is
read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_overlap_abi.py's technique) — with the outputs
untouched and nothing enqueued.  What needs live handles (another device, a range beyond the size, a bad host image) is
tests/test_places_gpu.py's."""
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
DP, FP, I32, SZ = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_size_t)
VP, PVP = C.c_void_p, C.POINTER(C.c_void_p)
PP, PM = C.POINTER(_lib.PlaceParams), C.POINTER(_lib.PlaceMatch)
SENTINEL = 0xDEAD


def message():
    return sga.load().sga_last_error().decode()


def params(**fields):
    p = _lib.PlaceParams()
    sga.load().sga_place_params_default(C.byref(p))
    for name, value in fields.items():
        setattr(p, name, value)
    return p


def counters():
    out = []
    for name in ("sga_debug_places_add_launches", "sga_debug_places_query_launches", "sga_debug_places_waits"):
        v = C.c_ulonglong()
        assert getattr(sga.load(), name)(C.byref(v)) == OK
        out.append(v.value)
    return out


def center(c):
    return None if c is None else np.ascontiguousarray(c, dtype=np.float64).ctypes.data_as(DP)


IMAGE = np.zeros(4096, np.float32)


def create(p, ctx=STAND_IN, with_out=True):
    out = C.c_void_p(SENTINEL)
    rc = sga.load().sga_places_create(C.c_void_p(ctx), None if p is None else C.byref(p), C.byref(out) if with_out else None)
    return rc, out.value


def add(ctx=STAND_IN, db=STAND_IN, cloud=STAND_IN, c=None, with_index=True):
    index = C.c_size_t(SENTINEL)
    rc = sga.load().sga_places_add(C.c_void_p(ctx), C.c_void_p(db), C.c_void_p(cloud), center(c), C.byref(index) if with_index else None)
    return rc, index.value


def scan_context(p, ctx=STAND_IN, cloud=STAND_IN, c=None, with_image=True):
    image = np.full(8, -7.0, np.float32)
    rc = sga.load().sga_cloud_scan_context(C.c_void_p(ctx), C.c_void_p(cloud), None if p is None else C.byref(p), center(c), image.ctypes.data_as(FP) if with_image else None)
    return rc, image


def query(ctx=STAND_IN, db=STAND_IN, cloud=STAND_IN, c=None, k=1, with_out=True, with_found=True, by_image=False, image=IMAGE):
    out = (_lib.PlaceMatch * 32)()
    out[0].index = SENTINEL
    found = C.c_size_t(SENTINEL)
    tail = (0, 0, k, C.cast(out, PM) if with_out else None, C.byref(found) if with_found else None, None, None)
    if by_image:
        rc = sga.load().sga_places_query_descriptor(C.c_void_p(ctx), C.c_void_p(db), None if image is None else image.ctypes.data_as(FP), *tail)
    else:
        rc = sga.load().sga_places_query(C.c_void_p(ctx), C.c_void_p(db), C.c_void_p(cloud), center(c), *tail)
    return rc, out[0].index, found.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    want = {
        "sga_place_params_default": (None, [PP]),
        "sga_places_create": (C.c_int, [VP, PP, PVP]),
        "sga_places_destroy": (C.c_int, [VP]),
        "sga_places_size": (C.c_int, [VP, SZ]),
        "sga_places_params": (C.c_int, [VP, PP]),
        "sga_places_add": (C.c_int, [VP, VP, VP, DP, SZ]),
        "sga_places_add_descriptor": (C.c_int, [VP, VP, FP, SZ]),
        "sga_places_download": (C.c_int, [VP, VP, C.c_size_t, C.c_size_t, FP]),
        "sga_cloud_scan_context": (C.c_int, [VP, VP, PP, DP, FP]),
        "sga_places_query": (C.c_int, [VP, VP, VP, DP, C.c_size_t, C.c_size_t, C.c_int, PM, SZ, DP, I32]),
        "sga_places_query_descriptor": (C.c_int, [VP, VP, FP, C.c_size_t, C.c_size_t, C.c_int, PM, SZ, DP, I32]),
        "sga_debug_places_add_launches": (C.c_int, [C.POINTER(C.c_ulonglong)]),
        "sga_debug_places_query_launches": (C.c_int, [C.POINTER(C.c_ulonglong)]),
        "sga_debug_places_waits": (C.c_int, [C.POINTER(C.c_ulonglong)]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert bound.get(name) == sig, name
    for name in ("PlaceDatabase", "scan_context_distance", "places_add_launches", "places_query_launches", "places_waits"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.scan_context) and callable(sga.synthetic.scan_at)
    for member in ("add", "add_descriptor", "query", "descriptors", "__len__", "yaw_guess"):
        assert callable(getattr(sga.PlaceDatabase, member)), member


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    ctype = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32}

    def fields_of(name):
        m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S)
        assert m is not None, name
        body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
        return [(n.strip(), ctype[t]) for t, names in re.findall(r"\b(int64_t|int32_t|int|double)\s+([a-z_, ]+);", body) for n in names.split(",")]

    assert fields_of("sga_place_params") == [("rings", C.c_int), ("sectors", C.c_int), ("max_range", C.c_double), ("height", C.c_double)] == list(_lib.PlaceParams._fields_)
    assert fields_of("sga_place_match") == [("index", C.c_int64), ("shift", C.c_int32), ("reserved", C.c_int32), ("distance", C.c_double)] == list(_lib.PlaceMatch._fields_)
    assert C.sizeof(_lib.PlaceParams) == 24 and C.sizeof(_lib.PlaceMatch) == 24
    assert api.PLACE_MATCH_DTYPE.itemsize == 24 and [api.PLACE_MATCH_DTYPE.fields[n][1] for n in ("index", "shift", "reserved", "distance")] == [0, 8, 12, 16]
    for decl in (
        "void sga_place_params_default(sga_place_params* p);",
        "int sga_places_create(sga_context* ctx, const sga_place_params* params, sga_places** out);",
        "int sga_places_destroy(sga_places* db);",
        "int sga_places_size(const sga_places* db, size_t* n);",
        "int sga_places_params(const sga_places* db, sga_place_params* params);",
        "int sga_places_add(sga_context* ctx, sga_places* db, const sga_cloud* cloud, const double center[3]",
        "int sga_places_add_descriptor(sga_context* ctx, sga_places* db, const float* image",
        "int sga_places_download(sga_context* ctx, const sga_places* db, size_t first, size_t count, float* images",
        "int sga_cloud_scan_context(sga_context* ctx, const sga_cloud* cloud, const sga_place_params* params, const double center[3]",
        "int sga_places_query(sga_context* ctx, const sga_places* db, const sga_cloud* cloud, const double center[3]",
        "int sga_places_query_descriptor(sga_context* ctx, const sga_places* db, const float* image",
    ):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    for name in ("sga_debug_places_add_launches(unsigned long long* launches)", "sga_debug_places_query_launches(unsigned long long* launches)", "sga_debug_places_waits(unsigned long long* waits)"):
        assert "int %s;" % name in debug, name


def test_defaults():
    p = params()
    assert (p.rings, p.sectors, p.max_range, p.height) == (20, 60, 80.0, 2.0)
    sga.load().sga_place_params_default(None)  # a NULL struct is left alone
    assert bytes(api._place_params()) == bytes(p)
    q = api._place_params(rings=3, height=None, max_range=12.5)
    assert (q.rings, q.sectors, q.max_range, q.height) == (3, 60, 12.5, 2.0)


def test_null_arguments_are_refused():
    before = counters()
    p = params()
    for rc, out in (create(p, ctx=0), create(None)):
        assert rc == INVALID and "null argument" in message() and out == SENTINEL
    assert create(p, with_out=False)[0] == INVALID and "null argument" in message()
    for kw in ({"ctx": 0}, {"db": 0}, {"cloud": 0}, {"with_index": False}):
        rc, index = add(**kw)
        assert rc == INVALID and "null argument" in message() and index == SENTINEL, kw
    for kw in ({"ctx": 0}, {"cloud": 0}, {"with_image": False}):
        rc, image = scan_context(p, **kw)
        assert rc == INVALID and "null argument" in message() and (image == -7.0).all(), kw
    assert scan_context(None)[0] == INVALID and "null argument" in message()
    for kw in ({"ctx": 0}, {"db": 0}, {"cloud": 0}, {"with_out": False}, {"with_found": False}):
        rc, index, found = query(**kw)
        assert rc == INVALID and "null argument" in message() and index == SENTINEL and found == SENTINEL, kw
    for kw in ({"ctx": 0}, {"db": 0}, {"image": None}, {"with_out": False}, {"with_found": False}):
        rc, index, found = query(by_image=True, **kw)
        assert rc == INVALID and "null argument" in message() and index == SENTINEL and found == SENTINEL, kw
    lib = sga.load()
    n, i = C.c_size_t(SENTINEL), C.c_size_t(SENTINEL)
    assert lib.sga_places_size(None, C.byref(n)) == INVALID and lib.sga_places_size(C.c_void_p(STAND_IN), None) == INVALID and n.value == SENTINEL
    assert lib.sga_places_params(None, C.byref(p)) == INVALID and lib.sga_places_params(C.c_void_p(STAND_IN), None) == INVALID
    for ctx, db, image, index in ((0, STAND_IN, IMAGE, i), (STAND_IN, 0, IMAGE, i), (STAND_IN, STAND_IN, None, i), (STAND_IN, STAND_IN, IMAGE, None)):
        rc = lib.sga_places_add_descriptor(C.c_void_p(ctx), C.c_void_p(db), None if image is None else image.ctypes.data_as(FP), None if index is None else C.byref(index))
        assert rc == INVALID and "null argument" in message() and i.value == SENTINEL
    for ctx, db, images in ((0, STAND_IN, IMAGE), (STAND_IN, 0, IMAGE), (STAND_IN, STAND_IN, None)):
        rc = lib.sga_places_download(C.c_void_p(ctx), C.c_void_p(db), 0, 1, None if images is None else images.ctypes.data_as(FP))
        assert rc == INVALID and "null argument" in message()
    assert lib.sga_places_destroy(None) == OK  # as free(NULL)
    assert counters() == before


BAD_PARAMS = [
    ({"rings": 0}, "rings 0 outside [1, 64]"),
    ({"rings": -3}, "rings -3 outside"),
    ({"rings": 65, "sectors": 1}, "rings 65 outside"),
    ({"sectors": 0}, "sectors 0 outside [1, 256]"),
    ({"sectors": -1}, "sectors -1 outside"),
    ({"sectors": 257, "rings": 1}, "sectors 257 outside"),
    ({"rings": 17, "sectors": 241}, "more than 4096 cells"),
    ({"rings": 64, "sectors": 65}, "more than 4096 cells"),
    ({"max_range": 0.0}, "max_range"),
    ({"max_range": -80.0}, "max_range"),
    ({"max_range": INF}, "max_range"),
    ({"max_range": NAN}, "max_range"),
    ({"height": NAN}, "height"),
    ({"height": INF}, "height"),
    ({"height": -INF}, "height"),
]


@pytest.mark.parametrize("fields, word", BAD_PARAMS)
def test_bad_parameters_are_refused_before_a_handle_is_read(fields, word):
    before = counters()
    rc, out = create(params(**fields))  # (the stand-in handles would fault if they were read)
    assert rc == INVALID and word in message() and out == SENTINEL, message()
    rc, image = scan_context(params(**fields))
    assert rc == INVALID and word in message() and (image == -7.0).all(), message()
    assert counters() == before


@pytest.mark.parametrize("fields", [{"rings": 1, "sectors": 1}, {"rings": 64, "sectors": 64}, {"rings": 16, "sectors": 256}, {"max_range": 1e-300}, {"height": -1e300}])
def test_parameters_at_their_limits_pass_the_check(fields):
    """no handle can be read here, so acceptance shows through the refusal that stands behind the parameter check"""
    rc, image = scan_context(params(**fields), c=[0.0, NAN, 0.0])
    assert rc == INVALID and "center has a non-finite entry" in message() and (image == -7.0).all()


@pytest.mark.parametrize("c", [[NAN, 0.0, 0.0], [0.0, INF, 0.0], [0.0, 0.0, -INF]])
def test_a_non_finite_center_is_refused_before_a_handle_is_read(c):
    before = counters()
    rc, index = add(c=c)
    assert rc == INVALID and "center has a non-finite entry" in message() and index == SENTINEL
    rc, image = scan_context(params(), c=c)
    assert rc == INVALID and "center has a non-finite entry" in message() and (image == -7.0).all()
    rc, index, found = query(c=c)
    assert rc == INVALID and "center has a non-finite entry" in message() and index == SENTINEL and found == SENTINEL
    assert counters() == before


@pytest.mark.parametrize("k", [0, -1, 33, 1 << 20])
def test_k_outside_its_range_is_refused_before_a_handle_is_read(k):
    before = counters()
    for by_image in (False, True):
        rc, index, found = query(k=k, by_image=by_image)
        assert rc == INVALID and "k %d outside [1, 32]" % k in message() and index == SENTINEL and found == SENTINEL
    assert counters() == before


def test_python_layer_checks_shapes():
    assert np.allclose(sga.PlaceDatabase.yaw_guess(type("P", (), {"sectors": 60})(), 15), [[0, -1, 0, 0], [1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], atol=1e-15)
    d, s = sga.scan_context_distance(np.float32([[1, 0], [0, 1]]), np.float32([[0, 2], [2, 0]]))
    assert (d, s) == (0.0, 1)
    with pytest.raises(ValueError):
        sga.scan_context_distance(np.zeros((2, 3)), np.zeros((3, 2)))

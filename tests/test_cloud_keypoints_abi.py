"""The boundary of the ISS keypoints and of the descriptor gather without a device: the symbols exist and are
bound with the header's signatures, sga_iss_params has the header's fields, offsets and size (40 bytes), sga_iss_default gives the
defaults; null arguments and parameters outside their ranges are refused before any handle is read — the handles are stand-ins at an
address nothing is mapped at (tests/test_cloud_plane_abi.py's technique) — with the outputs cleared or untouched and nothing enqueued."""
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
DP, I64, SZ = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_size_t)
VP, PVP, ULL = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_ulonglong)
PIP = C.POINTER(_lib.IssParams)
SENTINEL = 0xDEAD


def message():
    return sga.load().sga_last_error().decode()


def params(**fields):
    p = _lib.IssParams()
    sga.load().sga_iss_default(C.byref(p))
    p.salient_radius, p.non_max_radius = 1.5, 0.75
    for name, value in fields.items():
        setattr(p, name, value)
    return p


def counters():
    return [sga.iss_launches(), sga.iss_waits()]


def keypoints(p, ctx=STAND_IN, cloud=STAND_IN, tree=None, with_count=True, with_out=None):
    """-> (status, saliency and kept untouched, count, out)"""
    with_out = (p is not None and p.keep != 0) if with_out is None else with_out
    sal, kept = np.full(4, -7.0), np.full(4, -7, np.int64)
    count = C.c_size_t(SENTINEL)
    out = C.c_void_p(SENTINEL)
    rc = sga.load().sga_cloud_iss_keypoints(C.c_void_p(ctx), C.c_void_p(cloud), None if tree is None else C.c_void_p(tree), None if p is None else C.byref(p), sal.ctypes.data_as(DP), kept.ctypes.data_as(I64),
                                            C.byref(count) if with_count else None, C.byref(out) if with_out else None)
    return rc, bool((sal == -7.0).all() and (kept == -7).all()), count.value, out.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    want = {
        "sga_iss_default": (None, [PIP]),
        "sga_cloud_iss_keypoints": (C.c_int, [VP, VP, VP, PIP, DP, I64, SZ, PVP]),
        "sga_features_select": (C.c_int, [VP, VP, I64, C.c_size_t, PVP]),
        "sga_debug_iss_launches": (C.c_int, [ULL]),
        "sga_debug_iss_waits": (C.c_int, [ULL]),
    }
    for name, sig in want.items():
        assert hasattr(lib, name), name
        assert bound.get(name) == sig, name
    for name in ("iss_keypoints", "iss_launches", "iss_waits"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.iss_keypoints) and callable(sga.Features.selected)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_iss_params \{(.*?)\} sga_iss_params;", text, re.S)
    assert m is not None
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    fields = [(name, ctype[t]) for t, name in re.findall(r"\b(double|int32_t)\s+(\w+);", body)]
    assert fields == _lib.IssParams._fields_
    assert [n for n, _ in fields] == ["salient_radius", "non_max_radius", "gamma_21", "gamma_32", "min_neighbors", "keep"]
    assert C.sizeof(_lib.IssParams) == 40 and "} sga_iss_params; /* 40 bytes */" in text
    assert [getattr(_lib.IssParams, n).offset for n, _ in fields] == [0, 8, 16, 24, 32, 36]
    for decl in (
        "void sga_iss_default(sga_iss_params* p);",
        "int sga_cloud_iss_keypoints(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree",
        "int sga_features_select(sga_context* ctx, const sga_features* features, const int64_t* indices, size_t m, sga_features** out);",
    ):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    for name in ("sga_debug_iss_launches(unsigned long long* launches)", "sga_debug_iss_waits(unsigned long long* waits)"):
        assert "int %s;" % name in debug, name
    hpp = open(os.path.join(ROOT, "include", "small_gicp_amd.hpp")).read()
    for word in ("struct IssParams : sga_iss_params", "struct Keypoints", "Keypoints iss_keypoints(", "selected(const std::vector<int64_t>& indices)"):
        assert word in hpp, word


def test_defaults():
    p = _lib.IssParams(7.0, 7.0, 7.0, 7.0, 7, 7)
    sga.load().sga_iss_default(C.byref(p))
    assert (p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32, p.min_neighbors, p.keep) == (0.0, 0.0, 0.975, 0.975, 5, 0)  # the radii have no default
    sga.load().sga_iss_default(None)  # a NULL struct is left alone
    q = api._iss_params(1.5, 0.75)
    assert (q.salient_radius, q.non_max_radius, q.gamma_21, q.gamma_32, q.min_neighbors, q.keep) == (1.5, 0.75, 0.975, 0.975, 5, 0)
    q = api._iss_params(2.0, 1.0, 0.9, 0.8, 7, True)
    assert (q.salient_radius, q.non_max_radius, q.gamma_21, q.gamma_32, q.min_neighbors, q.keep) == (2.0, 1.0, 0.9, 0.8, 7, 1)
    assert api._iss_params(q) is q


def test_null_arguments_are_refused():
    before = counters()
    p = params()
    for rc, untouched, count, out in (keypoints(p, ctx=0), keypoints(p, cloud=0), keypoints(None)):
        assert rc == INVALID and "null argument" in message() and untouched and count == 0 and out == SENTINEL  # *count = 0 on every refusal
    rc, untouched, count, out = keypoints(p, with_count=False)
    assert rc == INVALID and "null argument" in message() and untouched
    rc, untouched, count, out = keypoints(params(keep=1), ctx=0)
    assert rc == INVALID and untouched and count == 0 and out is None  # *out = NULL on every refusal
    assert sga.load().sga_debug_iss_launches(None) == INVALID and sga.load().sga_debug_iss_waits(None) == INVALID
    assert counters() == before


BAD_PARAMS = [
    ({"salient_radius": 0.0}, "salient_radius must be finite and > 0"),
    ({"salient_radius": -1.0}, "salient_radius must be finite and > 0"),
    ({"salient_radius": INF}, "salient_radius must be finite and > 0"),
    ({"salient_radius": NAN}, "salient_radius must be finite and > 0"),
    ({"non_max_radius": 0.0}, "non_max_radius must be finite and > 0"),
    ({"non_max_radius": -0.5}, "non_max_radius must be finite and > 0"),
    ({"non_max_radius": INF}, "non_max_radius must be finite and > 0"),
    ({"non_max_radius": NAN}, "non_max_radius must be finite and > 0"),
    ({"gamma_21": 0.0}, "gamma_21 must be in (0, 1]"),
    ({"gamma_21": 1.0000001}, "gamma_21 must be in (0, 1]"),
    ({"gamma_21": NAN}, "gamma_21 must be in (0, 1]"),
    ({"gamma_32": 0.0}, "gamma_32 must be in (0, 1]"),
    ({"gamma_32": -0.5}, "gamma_32 must be in (0, 1]"),
    ({"gamma_32": INF}, "gamma_32 must be in (0, 1]"),
    ({"min_neighbors": 0}, "min_neighbors 0 is below 1"),
    ({"min_neighbors": -3}, "min_neighbors -3 is below 1"),
    ({"keep": 2}, "keep 2 is not 0"),
    ({"keep": -1}, "keep -1 is not 0"),
]


@pytest.mark.parametrize("fields, word", BAD_PARAMS)
def test_bad_parameters_are_refused_before_a_handle_is_read(fields, word):
    before = counters()
    rc, untouched, count, out = keypoints(params(**fields), tree=STAND_IN, with_out=False)  # (the stand-in handles would fault if they were read)
    assert rc == INVALID and word in message() and untouched and count == 0, message()
    assert counters() == before


def test_keep_must_agree_with_out():
    before = counters()
    rc, untouched, count, out = keypoints(params(keep=0), with_out=True)
    assert rc == INVALID and "keep is 0 but an output cloud is asked for" in message() and untouched and out is None
    rc, untouched, count, out = keypoints(params(keep=1), with_out=False)
    assert rc == INVALID and "keep is 1 but there is no place for the output cloud" in message() and untouched
    assert counters() == before


@pytest.mark.parametrize("fields", [{"salient_radius": 1e-300}, {"non_max_radius": 1e300}, {"gamma_21": 1.0}, {"gamma_32": 1e-300}, {"min_neighbors": 1}, {"min_neighbors": 2**31 - 1}])
def test_parameters_at_their_limits_pass_the_check(fields):
    """no handle can be read here, so acceptance shows through the refusal that stands behind the check of these parameters"""
    rc, untouched, count, out = keypoints(params(keep=5, **fields), with_out=False)
    assert rc == INVALID and "keep 5 is not 0" in message() and untouched


def test_features_select_refusals():
    lib = sga.load()
    idx = np.zeros(2, np.int64)
    ip = idx.ctypes.data_as(I64)
    for ctx, feats, indices, m in ((0, STAND_IN, ip, 2), (STAND_IN, 0, ip, 2), (STAND_IN, STAND_IN, None, 2)):
        out = C.c_void_p(SENTINEL)
        assert lib.sga_features_select(C.c_void_p(ctx), C.c_void_p(feats), indices, m, C.byref(out)) == INVALID and "null argument" in message()
        assert out.value is None  # *out = NULL
    assert lib.sga_features_select(C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), ip, 2, None) == INVALID and "null argument" in message()
    out = C.c_void_p(SENTINEL)
    assert lib.sga_features_select(C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), ip, 2**31, C.byref(out)) == INVALID and "too many indices" in message() and out.value is None

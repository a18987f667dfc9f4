"""The boundary of the sweep registration calls without a device: the symbols exist and are bound with the
header's signatures, the ctypes structures have the header's sizes, sga_sweep_params_default gives the defaults; NULL arguments,
non-finite entries of T, the twist, ref_time or the prior, an information matrix that is not symmetric, robust kernels and restrict_dof
are refused before any handle is read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_overlap_abi.py's
technique) — with nothing enqueued.  What needs live handles is tests/test_sweep_gpu.py's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID, UNSUPPORTED = 0, 1, 4
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
INF, NAN = float("inf"), float("nan")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)


def message():
    return sga.load().sga_last_error().decode()


def launches():
    v = C.c_ulonglong()
    assert sga.load().sga_debug_sweep_launches(C.byref(v)) == OK
    return v.value


def dp(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(DP)


IDENTITY = np.eye(4).reshape(16)
TIMES = np.zeros(4, np.float32)


def linearize(ctx=STAND_IN, target=STAND_IN, source=STAND_IN, times=TIMES, fp="default", T=IDENTITY, twist=np.zeros(6), ref_time=1.0, outputs=(True, True, True, True)):
    if isinstance(fp, str):
        fp = sga.make_setting("GICP").factor
    H, b, e, n = np.zeros(144), np.zeros(12), C.c_double(), C.c_uint64()
    return sga.load().sga_sweep_linearize(C.c_void_p(ctx), C.c_void_p(target), C.c_void_p(source), None if times is None else times.ctypes.data_as(C.POINTER(C.c_float)), None if fp is None else C.byref(fp), dp(T), dp(twist),
                                          ref_time, dp(H) if outputs[0] else None, dp(b) if outputs[1] else None, C.byref(e) if outputs[2] else None, C.byref(n) if outputs[3] else None, None)


def error(ctx=STAND_IN, target=STAND_IN, source=STAND_IN, times=TIMES, fp="default", T=IDENTITY, twist=np.zeros(6), ref_time=1.0, with_e=True):
    if isinstance(fp, str):
        fp = sga.make_setting("GICP").factor
    e = C.c_double()
    return sga.load().sga_sweep_error(C.c_void_p(ctx), C.c_void_p(target), C.c_void_p(source), None if times is None else times.ctypes.data_as(C.POINTER(C.c_float)), None if fp is None else C.byref(fp), dp(T), dp(twist), ref_time,
                                      C.byref(e) if with_e else None)


def align(ctx=STAND_IN, target=STAND_IN, source=STAND_IN, times=TIMES, T=None, twist=None, setting="default", params="default", with_out=True):
    if isinstance(setting, str):
        setting = sga.make_setting("GICP")
    if isinstance(params, str):
        params = api._sweep_params()
    out = _lib.SweepResultC()
    return sga.load().sga_align_sweep(C.c_void_p(ctx), C.c_void_p(target), C.c_void_p(source), None if times is None else times.ctypes.data_as(C.POINTER(C.c_float)), dp(T), dp(twist), None if setting is None else C.byref(setting),
                                      None if params is None else C.byref(params), C.byref(out) if with_out else None)


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_sweep_params_default", "sga_sweep_linearize", "sga_sweep_error", "sga_align_sweep", "sga_debug_sweep_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    vp, fp, fpar = C.c_void_p, C.POINTER(C.c_float), C.POINTER(_lib.FactorParams)
    assert bound["sga_sweep_params_default"] == (None, [C.POINTER(_lib.SweepParams)])
    assert bound["sga_sweep_linearize"] == (C.c_int, [vp, vp, vp, fp, fpar, DP, DP, C.c_double, DP, DP, DP, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)])
    assert bound["sga_sweep_error"] == (C.c_int, [vp, vp, vp, fp, fpar, DP, DP, C.c_double, DP])
    assert bound["sga_align_sweep"] == (C.c_int, [vp, vp, vp, fp, DP, DP, C.POINTER(_lib.RegistrationSettingC), C.POINTER(_lib.SweepParams), C.POINTER(_lib.SweepResultC)])
    assert bound["sga_debug_sweep_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("align_sweep", "linearize_sweep", "sweep_error", "sweep_launches", "SweepResult"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"typedef struct sga_sweep_params \{(.*?)\} sga_sweep_params;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|uint64_t)\s+([A-Za-z_, ]+)(\[\d+\])?;", m.group(1))
    assert [(t, n.strip(), d) for t, n, d in fields] == [("double", "ref_time", ""), ("double", "twist_prior", "[6]"), ("double", "twist_information", "[36]")]
    assert [n for n, _ in _lib.SweepParams._fields_] == ["ref_time", "twist_prior", "twist_information"] and C.sizeof(_lib.SweepParams) == 8 * 43
    m = re.search(r"typedef struct sga_sweep_result \{(.*?)\} sga_sweep_result;", text, re.S)
    assert m is not None
    fields = re.findall(r"\b(int|double|uint64_t)\s+([A-Za-z_, ]+)(\[\d+\])?;", m.group(1))
    assert [(t, n.strip(), d) for t, n, d in fields] == [("double", "T_target_source", "[16]"), ("double", "twist", "[6]"), ("int", "converged", ""), ("uint64_t", "iterations, num_inliers", ""), ("double", "H", "[144]"),
                                                          ("double", "b", "[12]"), ("double", "error", "")]
    assert [n for n, _ in _lib.SweepResultC._fields_] == ["T_target_source", "twist", "converged", "iterations", "num_inliers", "H", "b", "error"]
    assert C.sizeof(_lib.SweepResultC) == 8 * (16 + 6 + 1 + 2 + 144 + 12 + 1)  # (converged: an int and its padding)
    for decl in ("void sga_sweep_params_default(sga_sweep_params* p);", "int sga_sweep_linearize(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* params",
                 "int sga_sweep_error(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times", "int sga_align_sweep(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times"):
        assert decl in text, decl
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    assert "int sga_debug_sweep_launches(unsigned long long* launches);" in debug


def test_defaults():
    p = _lib.SweepParams()
    p.ref_time, p.twist_prior[2], p.twist_information[7] = 5.0, 1.0, 2.0
    sga.load().sga_sweep_params_default(C.byref(p))
    assert p.ref_time == 1.0 and list(p.twist_prior) == [0.0] * 6 and list(p.twist_information) == [0.0] * 36
    sga.load().sga_sweep_params_default(None)  # a NULL struct is left alone
    q = api._sweep_params(0.5, np.arange(6), np.eye(6) * 3)
    assert q.ref_time == 0.5 and list(q.twist_prior) == [0, 1, 2, 3, 4, 5] and q.twist_information[7] == 3.0 and q.twist_information[1] == 0.0
    r = sga.SweepResult()
    assert r.H.shape == (12, 12) and r.b.shape == (12,) and r.twist.shape == (6,) and not r.converged


def test_null_arguments_are_refused():
    before = launches()
    for kw in ({"ctx": 0}, {"target": 0}, {"source": 0}, {"times": None}, {"fp": None}, {"T": None}, {"twist": None}, {"outputs": (False, True, True, True)}, {"outputs": (True, False, True, True)},
               {"outputs": (True, True, False, True)}, {"outputs": (True, True, True, False)}):
        assert linearize(**kw) == INVALID and "null argument" in message(), kw
    for kw in ({"ctx": 0}, {"target": 0}, {"source": 0}, {"times": None}, {"fp": None}, {"T": None}, {"twist": None}, {"with_e": False}):
        assert error(**kw) == INVALID and "null argument" in message(), kw
    for kw in ({"ctx": 0}, {"target": 0}, {"source": 0}, {"times": None}, {"setting": None}, {"params": None}, {"with_out": False}):
        assert align(**kw) == INVALID and "null argument" in message(), kw
    assert launches() == before


def bad(base, k, v):
    a = np.array(base, dtype=np.float64).copy()
    a[k] = v
    return a


def robust():
    return sga.make_setting("GICP", robust_kernel="HUBER")


STATE_CASES = [
    ({"T": bad(IDENTITY, 0, NAN)}, INVALID, "T has a non-finite entry"),
    ({"T": bad(IDENTITY, 13, INF)}, INVALID, "T has a non-finite entry"),
    ({"twist": bad(np.zeros(6), 2, NAN)}, INVALID, "twist has a non-finite entry"),
    ({"twist": bad(np.zeros(6), 5, -INF)}, INVALID, "twist has a non-finite entry"),
    ({"ref_time": NAN}, INVALID, "reference time is not finite"),
    ({"ref_time": INF}, INVALID, "reference time is not finite"),
]


@pytest.mark.parametrize("kw, status, word", STATE_CASES + [({"fp": "robust"}, UNSUPPORTED, "robust kernels")])
def test_linearize_and_error_refuse_before_a_handle_is_read(kw, status, word):
    kw = dict(kw)
    if kw.get("fp") == "robust":
        kw["fp"] = robust().factor
    before = launches()
    assert linearize(**kw) == status and word in message(), message()  # (the stand-in handles would fault if they were read)
    assert error(**kw) == status and word in message(), message()
    assert launches() == before


def prior(**fields):
    p = api._sweep_params()
    for name, (k, v) in fields.items():
        getattr(p, name)[k] = v
    return p


def asymmetric():
    p = api._sweep_params(twist_information=np.eye(6))
    p.twist_information[6 * 1 + 4] = 0.5  # (1, 4) without (4, 1)
    return p


def ref_time_param(v):
    p = api._sweep_params()
    p.ref_time = v
    return p


@pytest.mark.parametrize(
    "kw, status, word",
    [
        (lambda: {"T": bad(IDENTITY, 5, NAN)}, INVALID, "T has a non-finite entry"),
        (lambda: {"twist": bad(np.zeros(6), 0, INF)}, INVALID, "twist has a non-finite entry"),
        (lambda: {"params": ref_time_param(NAN)}, INVALID, "reference time is not finite"),
        (lambda: {"params": prior(twist_prior=(3, NAN))}, INVALID, "twist prior has a non-finite entry"),
        (lambda: {"params": prior(twist_information=(35, INF))}, INVALID, "twist information has a non-finite entry"),
        (lambda: {"params": asymmetric()}, INVALID, "not symmetric"),
        (lambda: {"setting": robust()}, UNSUPPORTED, "robust kernels"),
        (lambda: {"setting": sga.make_setting("GICP", restrict_dof_lambda=1.0, restrict_dof_mask=[1, 1, 0, 1, 1, 1])}, UNSUPPORTED, "restrict_dof"),
    ],
)
def test_align_refuses_before_a_handle_is_read(kw, status, word):
    before = launches()
    assert align(**kw()) == status and word in message(), message()
    assert launches() == before

"""The boundary of the batched problem creation (sga_problem_create_batch) without a device: the three symbols
exist and are bound, count == 0 is SGA_OK whatever else is passed, null arguments and NULL members are refused before any handle is
read — the handles handed in are stand-ins at an address nothing is mapped at, so reading one would end the process — and the Python
layer refuses members that are not indices / PointCloud objects.  (What the plan decides about live members needs their point counts and
kinds, which live in device-side objects: tests/test_batch_problem_gpu.py checks it case by case.)"""
import ctypes as C
import inspect

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
NAMES = ["sga_problem_create_batch", "sga_debug_problem_batch_plan", "sga_debug_problem_batch_launches"]
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def message():
    return sga.load().sga_last_error().decode()


def launches():
    v = C.c_ulonglong()
    assert sga.load().sga_debug_problem_batch_launches(C.byref(v)) == OK
    return v.value


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert [len(bound[name][1]) for name in NAMES] == [6, 4, 1]
    for name in ("create_problems", "problem_batch_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(api._problem_batch_plan)
    from small_gicp_amd import odometry

    for driver in (odometry.run_synthetic_batched, odometry.run_synthetic_model_batched):
        assert inspect.signature(driver).parameters["batched_problems"].default is False  # off until measured


def test_refusals_come_before_any_handle_is_read():
    lib = sga.load()
    ctx = C.c_void_p(STAND_IN)
    targets, sources = handles(STAND_IN, STAND_IN, STAND_IN), handles(STAND_IN, STAND_IN, STAND_IN)
    T = (C.c_double * 48)()
    before = launches()
    # count == 0: SGA_OK whatever else is passed, and nothing is touched
    out = handles(7, 7, 7)
    assert lib.sga_problem_create_batch(None, None, None, None, 0, None) == OK
    assert lib.sga_problem_create_batch(ctx, targets, sources, T, 0, out) == OK and list(out) == [7, 7, 7]
    # null arguments
    for args in ((None, targets, sources, T, 3, out), (ctx, None, sources, T, 3, out), (ctx, targets, None, T, 3, out), (ctx, targets, sources, T, 3, None)):
        assert lib.sga_problem_create_batch(*args) == INVALID and "null argument" in message()
    assert list(out) == [None, None, None]  # every refusal that was given `out` left it all NULL
    # a NULL member is named (the stand-ins before it are not read: the NULL check of all members comes first), targets before sources
    out = handles(7, 7, 7)
    assert lib.sga_problem_create_batch(ctx, handles(STAND_IN, None, STAND_IN), sources, None, 3, out) == INVALID and "targets[1] is NULL" in message() and "null argument" in message()
    assert list(out) == [None, None, None]
    out = handles(7, 7, 7)
    assert lib.sga_problem_create_batch(ctx, targets, handles(STAND_IN, STAND_IN, None), T, 3, out) == INVALID and "sources[2] is NULL" in message()
    assert list(out) == [None, None, None]
    assert lib.sga_problem_create_batch(ctx, handles(None, STAND_IN), handles(None, STAND_IN), T, 2, out) == INVALID and "targets[0] is NULL" in message()
    assert launches() == before  # a refusal enqueues nothing


def test_debug_entry_points_check_their_arguments():
    lib = sga.load()
    before = launches()
    plan = (C.c_int * 4)(*([7] * 4))
    assert lib.sga_debug_problem_batch_plan(None, None, 0, plan) == OK and list(plan) == [0] * 4  # an empty call: no chain
    assert lib.sga_debug_problem_batch_plan(None, handles(STAND_IN), 1, plan) == INVALID and "null argument" in message()
    assert lib.sga_debug_problem_batch_plan(handles(STAND_IN), None, 1, plan) == INVALID and "null argument" in message()
    assert lib.sga_debug_problem_batch_plan(handles(STAND_IN), handles(STAND_IN), 1, None) == INVALID
    plan = (C.c_int * 4)(*([7] * 4))
    assert lib.sga_debug_problem_batch_plan(handles(None), handles(STAND_IN), 1, plan) == INVALID and "targets[0] is NULL" in message() and list(plan) == [0] * 4
    assert lib.sga_debug_problem_batch_plan(handles(STAND_IN), handles(None), 1, plan) == INVALID and "sources[0] is NULL" in message()
    assert lib.sga_debug_problem_batch_launches(None) == INVALID
    assert isinstance(api.problem_batch_launches(), int) and launches() == before


def test_python_layer_refuses_what_is_not_an_index_or_a_point_cloud():
    pts = np.zeros((4, 3), np.float32)
    for bad_targets, bad_sources in (([pts], [pts]), ([None], [None]), (["map"], ["cloud"]), ([object()], [object()])):
        with pytest.raises(TypeError):
            sga.create_problems(bad_targets, bad_sources)
        with pytest.raises(TypeError):
            api._problem_batch_plan(bad_targets, bad_sources)
    with pytest.raises(ValueError):
        sga.create_problems([], [pts])

"""The boundary of the batched voxel-map insert (sga_voxelmap_insert_batch) without a device: the three symbols
exist and are bound, count == 0 is SGA_OK whatever else is passed, null arguments and NULL members are refused before any handle is
read — the handles handed in are stand-ins at an address nothing is mapped at, so reading one would end the process — and the Python
layer refuses members that are not maps / PointCloud objects.  (What the plan decides about live members needs their point counts, which
live in device-side objects: tests/test_batch_voxelmap_insert_gpu.py checks it case by case.)"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
NAMES = ["sga_voxelmap_insert_batch", "sga_debug_voxelmap_insert_batch_plan", "sga_debug_voxelmap_insert_batch_launches"]
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def message():
    return sga.load().sga_last_error().decode()


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert len(bound["sga_voxelmap_insert_batch"][1]) == 5 and len(bound["sga_debug_voxelmap_insert_batch_plan"][1]) == 4
    for name in ("insert_batch", "voxelmap_insert_batch_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(api._voxelmap_insert_batch_plan)
    from small_gicp_amd import odometry

    assert callable(odometry.run_synthetic_model_batched)


def test_refusals_come_before_any_handle_is_read():
    lib = sga.load()
    ctx = C.c_void_p(STAND_IN)
    maps, clouds = handles(STAND_IN, STAND_IN, STAND_IN), handles(STAND_IN, STAND_IN, STAND_IN)
    T = (C.c_double * 48)()
    # count == 0: SGA_OK whatever else is passed
    assert lib.sga_voxelmap_insert_batch(None, None, None, None, 0) == OK
    assert lib.sga_voxelmap_insert_batch(ctx, maps, clouds, T, 0) == OK
    # null arguments
    for args in ((None, maps, clouds), (ctx, None, clouds), (ctx, maps, None)):
        assert lib.sga_voxelmap_insert_batch(*args, T, 3) == INVALID and "null argument" in message()
    # a NULL member is named (it is the first: the stand-ins behind it are not reached), maps before clouds
    assert lib.sga_voxelmap_insert_batch(ctx, handles(None, STAND_IN, STAND_IN), clouds, None, 3) == INVALID and "maps[0] is NULL" in message() and "null argument" in message()
    assert lib.sga_voxelmap_insert_batch(ctx, handles(None, STAND_IN), handles(None, STAND_IN), T, 2) == INVALID and "maps[0] is NULL" in message()


def test_debug_entry_points_check_their_arguments():
    lib = sga.load()
    plan = (C.c_int * 6)(*([7] * 6))
    assert lib.sga_debug_voxelmap_insert_batch_plan(None, None, 0, plan) == OK and list(plan) == [0] * 6  # an empty call: no chain
    assert lib.sga_debug_voxelmap_insert_batch_plan(None, handles(STAND_IN), 1, plan) == INVALID and "null argument" in message()
    assert lib.sga_debug_voxelmap_insert_batch_plan(handles(STAND_IN), None, 1, plan) == INVALID and "null argument" in message()
    assert lib.sga_debug_voxelmap_insert_batch_plan(handles(STAND_IN), handles(STAND_IN), 1, None) == INVALID
    plan = (C.c_int * 6)(*([7] * 6))
    assert lib.sga_debug_voxelmap_insert_batch_plan(handles(None), handles(STAND_IN), 1, plan) == INVALID and "maps[0] is NULL" in message() and list(plan) == [0] * 6
    assert lib.sga_debug_voxelmap_insert_batch_launches(None) == INVALID
    before = api.voxelmap_insert_batch_launches()
    assert isinstance(before, int) and api.voxelmap_insert_batch_launches() == before  # a refusal enqueues nothing


def test_python_layer_refuses_what_is_not_a_map_or_a_point_cloud():
    pts = np.zeros((4, 3), np.float32)
    for bad_maps, bad_clouds in (([pts], [pts]), ([None], [None]), (["map"], ["cloud"]), ([object()], [object()])):
        with pytest.raises(TypeError):
            sga.insert_batch(bad_maps, bad_clouds)
        with pytest.raises(TypeError):
            api._voxelmap_insert_batch_plan(bad_maps, bad_clouds)
    with pytest.raises(ValueError):
        sga.insert_batch([], [pts])

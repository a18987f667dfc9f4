"""sga_voxelgrid_sampling_batch without a device: the symbols, the argument checks that come before any device work, and the Python
layer's own check of its members."""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

INVALID = 1  # SGA_ERR_INVALID
NAMES = ("sga_voxelgrid_sampling_batch", "sga_debug_voxelgrid_batch_plan", "sga_debug_voxelgrid_batch_launches")


def test_the_symbols_exist():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name) and name in bound, name
    for name in ("voxelgrid_sampling_batch", "preprocess_points_batch"):
        assert callable(getattr(sga, name)), name


def test_null_arguments_are_refused_before_any_device_work():
    """No argument is dereferenced before the null checks: the stand-ins for the context and the cloud are never read."""
    lib = sga.load()
    stand_in = C.create_string_buffer(64)
    ctx = C.cast(stand_in, C.c_void_p)
    clouds = (C.c_void_p * 2)(C.addressof(stand_in), None)
    out = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    call = lib.sga_voxelgrid_sampling_batch
    for args in ((None, clouds, 2, 0.25, out), (ctx, None, 2, 0.25, out), (ctx, clouds, 2, 0.25, None)):
        assert call(*args) == INVALID
        assert b"null argument" in lib.sga_last_error()
    assert call(None, clouds, 2, 0.25, out) == INVALID and not out[0] and not out[1]  # on a failure every out[k] is NULL
    out = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    assert call(ctx, (C.c_void_p * 2)(None, None), 2, 0.25, out) == INVALID and b"clouds[0] is NULL" in lib.sga_last_error() and not out[0] and not out[1]
    assert call(ctx, (C.c_void_p * 2)(None, None), 2, 0.0, out) == INVALID and b"leaf size must be positive" in lib.sga_last_error()
    assert call(None, None, 0, 0.25, None) == 0  # count == 0
    plan = (C.c_int * 6)()
    assert lib.sga_debug_voxelgrid_batch_plan(None, 2, 0.25, plan) == INVALID
    assert lib.sga_debug_voxelgrid_batch_plan(clouds, 2, 0.25, None) == INVALID
    assert lib.sga_debug_voxelgrid_batch_plan((C.c_void_p * 2)(None, None), 2, 0.25, plan) == INVALID
    assert lib.sga_debug_voxelgrid_batch_plan(None, 0, 0.25, plan) == 0 and list(plan) == [0] * 6
    assert lib.sga_debug_voxelgrid_batch_launches(None) == INVALID
    assert sga.voxelgrid_batch_launches() >= 0


def test_the_python_layer_takes_point_clouds_only():
    with pytest.raises(TypeError):
        sga.voxelgrid_sampling_batch([np.zeros((4, 3), np.float32)], 0.25)
    with pytest.raises(TypeError):
        sga.preprocess_points_batch([None], 0.25, 10)
    with pytest.raises(TypeError):
        api._voxelgrid_batch_plan([object()], 0.25)

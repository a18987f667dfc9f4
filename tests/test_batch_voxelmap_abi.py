"""The boundary of the batched Gaussian voxel-map build (sga_index_build_gaussian_voxelmap_batch) without a device:
the three symbols exist and are bound, every refusal comes before any device work — the handles handed in are stand-ins at an address
nothing is mapped at, so reading one would end the process —, every out[k] is NULL after a refusal, count == 0 is SGA_OK, and the Python
layer refuses members that are not PointCloud objects."""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
NAMES = ["sga_index_build_gaussian_voxelmap_batch", "sga_debug_voxelmap_batch_plan", "sga_debug_voxelmap_batch_launches"]
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def dirty(n):
    return (C.c_void_p * n)(*([0xDEAD0] * n))


def message():
    return sga.load().sga_last_error().decode()


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert len(bound["sga_index_build_gaussian_voxelmap_batch"][1]) == 5 and len(bound["sga_debug_voxelmap_batch_plan"][1]) == 4
    for name in ("build_gaussian_voxelmaps", "voxelmap_batch_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(api._voxelmap_batch_plan) and callable(sga.GaussianVoxelMap.from_cloud)


def test_refusals_come_before_any_device_work():
    lib = sga.load()
    ctx = C.c_void_p(STAND_IN)
    clouds = handles(STAND_IN, STAND_IN, STAND_IN)
    # count == 0: SGA_OK whatever else is passed, nothing touched
    out = dirty(3)
    assert lib.sga_index_build_gaussian_voxelmap_batch(None, None, 0, 1.0, None) == OK
    assert lib.sga_index_build_gaussian_voxelmap_batch(ctx, clouds, 0, -1.0, out) == OK and [out[k] for k in range(3)] == [0xDEAD0] * 3
    # null arguments
    for args in ((None, clouds, 3, 1.0), (ctx, None, 3, 1.0)):
        out = dirty(3)
        assert lib.sga_index_build_gaussian_voxelmap_batch(*args, out) == INVALID and "null argument" in message()
        assert [out[k] for k in range(3)] == [None] * 3
    assert lib.sga_index_build_gaussian_voxelmap_batch(ctx, clouds, 3, 1.0, None) == INVALID and "null argument" in message()
    # a leaf size that is not positive (NaN included): refused before a member is looked at
    for leaf in (0.0, -1.0, float("nan")):
        out = dirty(3)
        assert lib.sga_index_build_gaussian_voxelmap_batch(ctx, clouds, 3, leaf, out) == INVALID and "leaf size must be positive" in message()
        assert [out[k] for k in range(3)] == [None] * 3
    # a NULL member is named (it is the first: the stand-ins behind it are not reached)
    out = dirty(3)
    assert lib.sga_index_build_gaussian_voxelmap_batch(ctx, handles(None, STAND_IN, STAND_IN), 3, 1.0, out) == INVALID and "clouds[0] is NULL" in message()
    assert [out[k] for k in range(3)] == [None] * 3


def test_debug_entry_points_check_their_arguments():
    lib = sga.load()
    plan = (C.c_int * 6)(*([7] * 6))
    assert lib.sga_debug_voxelmap_batch_plan(None, 0, 1.0, plan) == OK and list(plan) == [0] * 6
    assert lib.sga_debug_voxelmap_batch_plan(None, 2, 1.0, plan) == INVALID and "null argument" in message()
    assert lib.sga_debug_voxelmap_batch_plan(handles(STAND_IN), 1, 1.0, None) == INVALID
    assert lib.sga_debug_voxelmap_batch_plan(handles(STAND_IN), 1, 0.0, plan) == INVALID and "leaf size must be positive" in message()
    assert lib.sga_debug_voxelmap_batch_plan(handles(None), 1, 1.0, plan) == INVALID and "clouds[0] is NULL" in message()
    assert lib.sga_debug_voxelmap_batch_launches(None) == INVALID
    before = api.voxelmap_batch_launches()
    assert isinstance(before, int) and api.voxelmap_batch_launches() == before  # a refusal enqueues nothing


def test_python_layer_refuses_what_is_not_a_point_cloud():
    pts = np.zeros((4, 3), np.float32)
    for bad in ([pts], [None], ["cloud"], [object()]):
        with pytest.raises(TypeError):
            sga.build_gaussian_voxelmaps(bad, 1.0)
        with pytest.raises(TypeError):
            api._voxelmap_batch_plan(bad, 1.0)
    with pytest.raises(TypeError):
        sga.GaussianVoxelMap.from_cloud(pts, 1.0)

"""The boundary of the device-resident entry points (csrc/cloud_io.hip, problem.hip, device_io.hip) without a device: the four symbols
exist and are bound, the Python names are callable, an empty call is SGA_OK whatever else is passed, null arguments and a bad dtype /
cols / stride are refused before any handle is read — the handles handed in are stand-ins at an address nothing is mapped at, so reading
one would end the process — and from_torch refuses what it cannot take with ValueError before the library (or a context) is needed.
(What happens to live pointers — host memory, a row count past the allocation — needs the runtime's view of them:
tests/test_device_io_gpu.py.)"""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
NAMES = ["sga_cloud_create_device", "sga_cloud_export_device", "sga_index_knn_device", "sga_problem_get_factors_device"]
STAND_IN = 0x1000  # never mapped: a handle (or data) at this address cannot be read


def arr(dtype=_lib.F32, cols=3, stride=3, data=STAND_IN):
    a = _lib.DeviceArray()
    a.data, a.dtype, a.cols, a.stride = data, dtype, cols, stride
    return a


def message():
    return sga.load().sga_last_error().decode()


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in bound, name
    assert [len(bound[name][1]) for name in NAMES] == [9, 7, 10, 6]
    assert (_lib.F32, _lib.F64, _lib.IO_NO_ORDER, _lib.IO_RELATIVE) == (0, 1, 1, 2)
    assert C.sizeof(_lib.DeviceArray) == 24  # pointer + three ints, padded
    for name in ("from_torch", "from_device_pointer", "to_torch"):
        assert callable(getattr(sga.PointCloud, name)), name
    for cls in (sga.KdTree, sga.GaussianVoxelMap, api._FlatVoxelMap, api.IncrementalVoxelMap, api.IncrementalVoxelMapCov):
        assert callable(cls.batch_knn_search_torch), cls
    assert callable(sga.Problem.factors_torch)


def test_an_empty_call_is_ok_whatever_else_is_passed():
    lib = sga.load()
    ctx, h = C.c_void_p(STAND_IN), C.c_void_p(STAND_IN)
    out = C.c_void_p(7)
    assert lib.sga_cloud_create_device(None, None, None, None, 0, None, None, 0, None) == OK
    bad = arr(dtype=9, cols=5, stride=1)
    assert lib.sga_cloud_create_device(ctx, C.byref(bad), C.byref(bad), C.byref(bad), 0, None, C.c_void_p(STAND_IN), 3, C.byref(out)) == OK
    assert out.value is None  # no cloud is made
    assert lib.sga_index_knn_device(None, None, None, 0, 0, -1.0, None, None, None, 0) == OK
    assert lib.sga_index_knn_device(ctx, h, C.byref(bad), 0, 500, -1.0, C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), 0) == OK


def test_null_arguments_are_refused_before_any_handle_is_read():
    lib = sga.load()
    ctx, h = C.c_void_p(STAND_IN), C.c_void_p(STAND_IN)
    a, out = arr(), C.c_void_p(7)
    for args in ((None, C.byref(a), None, None, 4, None, None, 0, C.byref(out)), (ctx, None, None, None, 4, None, None, 0, C.byref(out)), (ctx, C.byref(a), None, None, 4, None, None, 0, None)):
        assert lib.sga_cloud_create_device(*args) == INVALID and "null argument" in message()
    assert out.value is None
    assert lib.sga_cloud_create_device(ctx, C.byref(a), None, None, 1 << 31, None, None, 0, C.byref(out)) == INVALID and "too large" in message()
    assert lib.sga_cloud_create_device(ctx, C.byref(a), None, None, 4, None, None, _lib.IO_RELATIVE, C.byref(out)) == INVALID and "origin" in message()
    for args in ((None, h, C.byref(a), None, None, None, 0), (ctx, None, C.byref(a), None, None, None, 0)):
        assert lib.sga_cloud_export_device(*args) == INVALID and "null argument" in message()
    d = C.c_void_p(STAND_IN)
    for args in ((None, h, C.byref(a), 4, 1, -1.0, d, d, None, 0), (ctx, None, C.byref(a), 4, 1, -1.0, d, d, None, 0), (ctx, h, None, 4, 1, -1.0, d, d, None, 0), (ctx, h, C.byref(a), 4, 1, -1.0, None, d, None, 0),
                 (ctx, h, C.byref(a), 4, 1, -1.0, d, None, None, 0)):
        assert lib.sga_index_knn_device(*args) == INVALID and "null argument" in message()
    assert lib.sga_index_knn_device(ctx, h, C.byref(a), 1 << 31, 1, -1.0, d, d, None, 0) == INVALID and "too many queries" in message()
    for k in (0, 129):
        assert lib.sga_index_knn_device(ctx, h, C.byref(a), 4, k, -1.0, d, d, None, 0) == INVALID and "k must be in [1,128]" in message()
    for args in ((None, h, d, d, None, 0), (ctx, None, d, d, None, 0), (ctx, h, None, None, None, 0)):
        assert lib.sga_problem_get_factors_device(*args) == INVALID and "null argument" in message()


@pytest.mark.parametrize("bad, word", [(dict(dtype=2), "dtype"), (dict(dtype=-1), "dtype"), (dict(cols=4, stride=4), "cols"), (dict(cols=6, stride=6), "cols"), (dict(stride=2), "stride"), (dict(stride=0), "stride")])
def test_a_bad_layout_is_refused_before_any_handle_is_read(bad, word):
    lib = sga.load()
    ctx, h, d = C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), C.c_void_p(STAND_IN)
    good, a, out = arr(), arr(**bad), C.c_void_p(7)
    assert lib.sga_cloud_create_device(ctx, C.byref(a), None, None, 4, None, None, 0, C.byref(out)) == INVALID and "points" in message() and word in message()
    assert lib.sga_cloud_create_device(ctx, C.byref(good), C.byref(a), None, 4, None, None, 0, C.byref(out)) == INVALID and "normals" in message() and word in message()
    assert lib.sga_cloud_export_device(ctx, h, C.byref(a), None, None, None, 0) == INVALID and "points" in message() and word in message()
    assert lib.sga_index_knn_device(ctx, h, C.byref(a), 4, 1, -1.0, d, d, None, 0) == INVALID and "queries" in message() and word in message()
    assert out.value is None


@pytest.mark.parametrize("cols, stride", [(3, 3), (12, 12), (9, 8), (16, 15)])
def test_covariances_are_6_9_or_16_columns(cols, stride):
    lib = sga.load()
    ctx, out = C.c_void_p(STAND_IN), C.c_void_p(7)
    good, c = arr(), arr(cols=cols, stride=stride)
    assert lib.sga_cloud_create_device(ctx, C.byref(good), None, C.byref(c), 4, None, None, 0, C.byref(out)) == INVALID and "covs" in message()
    assert lib.sga_cloud_export_device(ctx, C.c_void_p(STAND_IN), None, None, C.byref(c), None, 0) == INVALID and "covs" in message()


def test_from_torch_refuses_what_it_cannot_take():
    import torch

    cases = {
        "a CPU tensor": torch.zeros(4, 3),
        "float16": torch.zeros(4, 3, dtype=torch.float16),
        "1-D": torch.zeros(12),
        "a transposed view": torch.zeros(3, 4).t(),
        "five columns": torch.zeros(4, 5),
    }
    for what, t in cases.items():
        with pytest.raises(ValueError):
            sga.PointCloud.from_torch(t)
        print("refused:", what)
    with pytest.raises(ValueError):
        sga.PointCloud.from_torch(np.zeros((4, 3), np.float32))  # not a tensor at all
    with pytest.raises(ValueError):
        sga.PointCloud.from_device_pointer(STAND_IN, 4, dtype=np.float16)

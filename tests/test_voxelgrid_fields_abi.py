"""The boundary of the voxel grid that carries per-point columns without a device: the symbols exist and are
bound with the header's signatures, the SGA_REDUCE_* values are the header's, and every refusal the header lists as "before any handle
is read" returns SGA_ERR_INVALID with its message, NULL out pointers and the launch counter unchanged — the handles are stand-ins at an
address nothing is mapped at (tests/test_sweep_abi.py's technique).  The host form learns its number of columns from the fields handle, so
its ops are checked once the handle is read (tests/test_voxelgrid_fields_gpu.py); the device form's struct tells it, so there an op outside
0..4 is refused, named by its column, ahead of every handle.  What needs live handles is tests/test_voxelgrid_fields_gpu.py's."""
import ctypes as C
import os
import re

import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x77


def message():
    return sga.load().sga_last_error().decode()


def launches():
    v = C.c_ulonglong()
    assert sga.load().sga_debug_voxelgrid_fields_launches(C.byref(v)) == OK
    return v.value


def ops_array(ops):
    return None if ops is None else (C.c_int * len(ops))(*ops)


def host(ctx=STAND_IN, cloud=STAND_IN, fields=STAND_IN, ops=None, leaf=0.5, with_out=True, with_out_fields=True):
    out, out_f = C.c_void_p(SENTINEL), C.c_void_p(SENTINEL)
    rc = sga.load().sga_voxelgrid_sampling_fields(C.c_void_p(ctx), C.c_void_p(cloud), C.c_void_p(fields), ops_array(ops), leaf, C.byref(out) if with_out else None, C.byref(out_f) if with_out_fields else None, None, None)
    return rc, (out.value if with_out else None), (out_f.value if with_out_fields else None)


def device(ctx=STAND_IN, cloud=STAND_IN, fields="default", ops=None, leaf=0.5, with_out=True, with_out_fields=True, dtype=_lib.F32, cols=3, stride=4):
    out, out_f = C.c_void_p(SENTINEL), C.c_void_p(SENTINEL)
    arr = api._device_array(STAND_IN, dtype, cols, stride) if fields == "default" else fields
    rc = sga.load().sga_voxelgrid_sampling_fields_device(C.c_void_p(ctx), C.c_void_p(cloud), None if arr is None else C.byref(arr), ops_array(ops), leaf, C.byref(out) if with_out else None,
                                                         C.byref(out_f) if with_out_fields else None, None, None, None, 0)
    return rc, (out.value if with_out else None), (out_f.value if with_out_fields else None)


def refused(result, word):
    rc, out, out_f = result
    assert rc == INVALID and word in message(), (rc, message())
    assert not out and not out_f, (out, out_f)  # every out pointer that was given is NULL (None: not given)


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    names = ("sga_voxelgrid_sampling_fields", "sga_voxelgrid_sampling_fields_device", "sga_features_create_device", "sga_features_export_device", "sga_debug_voxelgrid_fields_launches")
    for name in names:
        assert hasattr(lib, name), name
        assert name in bound, name
    vp, pvp, ip, da = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.POINTER(_lib.DeviceArray)
    assert bound["sga_voxelgrid_sampling_fields"] == (C.c_int, [vp, vp, vp, ip, C.c_double, pvp, pvp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)])
    assert bound["sga_voxelgrid_sampling_fields_device"] == (C.c_int, [vp, vp, da, ip, C.c_double, pvp, pvp, vp, vp, vp, C.c_int])
    assert bound["sga_features_create_device"] == (C.c_int, [vp, da, C.c_size_t, vp, C.c_int, pvp])
    assert bound["sga_features_export_device"] == (C.c_int, [vp, vp, da, vp, C.c_int])
    assert bound["sga_debug_voxelgrid_fields_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("voxelgrid_sampling_fields", "voxelgrid_fields_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.Features.from_torch) and callable(sga.Features.to_torch)


def test_the_header_declares_what_is_bound():
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    m = re.search(r"enum \{ SGA_REDUCE_MEAN = (\d), SGA_REDUCE_MIN = (\d), SGA_REDUCE_MAX = (\d), SGA_REDUCE_FIRST = (\d), SGA_REDUCE_NEAREST = (\d) \};", text)
    assert m is not None and [int(v) for v in m.groups()] == [0, 1, 2, 3, 4]
    assert (_lib.REDUCE_MEAN, _lib.REDUCE_MIN, _lib.REDUCE_MAX, _lib.REDUCE_FIRST, _lib.REDUCE_NEAREST) == (0, 1, 2, 3, 4)
    assert api.REDUCE == {"mean": 0, "min": 1, "max": 2, "first": 3, "nearest": 4}
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    for decl in ("int sga_voxelgrid_sampling_fields(sga_context* ctx, const sga_cloud* in, const sga_features* fields , const int* ops , double leaf_size, sga_cloud** out, sga_features** out_fields , int32_t* counts , int64_t* voxel_of );",
                 "int sga_voxelgrid_sampling_fields_device(sga_context* ctx, const sga_cloud* in, const sga_device_array* fields, const int* ops, double leaf_size, sga_cloud** out, sga_features** out_fields, int32_t* d_counts, int64_t* d_voxel_of, void* user_stream, int flags);",
                 "int sga_features_create_device(sga_context* ctx, const struct sga_device_array* rows, size_t n, void* user_stream, int flags, sga_features** out);",
                 "int sga_features_export_device(sga_context* ctx, const sga_features* features, const struct sga_device_array* rows, void* user_stream, int flags);"):
        assert decl in flat, decl
    debug = open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()
    assert "int sga_debug_voxelgrid_fields_launches(unsigned long long* launches);" in debug


def test_null_arguments_are_refused():
    before = launches()
    for call in (host, device):
        for kw in ({"ctx": 0}, {"cloud": 0}, {"with_out": False}):
            refused(call(**kw), "null argument")
    refused(host(with_out_fields=False), "fields are given but out_fields is NULL")
    refused(host(fields=0), "out_fields is given but fields is NULL")
    refused(device(with_out_fields=False), "fields are given but out_fields is NULL")
    refused(device(fields=None), "out_fields is given but fields is NULL")
    assert launches() == before


@pytest.mark.parametrize("leaf", [0.0, -1.0, float("nan")])
def test_the_leaf_refusals_of_the_plain_call(leaf):
    before = launches()
    refused(host(leaf=leaf), "leaf size must be positive")
    refused(device(leaf=leaf), "leaf size must be positive")
    refused(host(fields=0, with_out_fields=False, leaf=leaf), "leaf size must be positive")  # membership only
    out = C.c_void_p(SENTINEL)
    assert sga.load().sga_voxelgrid_sampling(C.c_void_p(STAND_IN), C.c_void_p(STAND_IN), leaf, C.byref(out)) == INVALID and "leaf size must be positive" in message()
    assert launches() == before


@pytest.mark.parametrize("ops, column", [([5, 0, 0], 0), ([0, -1, 0], 1), ([4, 3, 7], 2)])
def test_an_op_outside_0_4_is_named_by_its_column(ops, column):
    before = launches()
    refused(device(ops=ops), "reduction %d of column %d" % (ops[column], column))
    assert launches() == before


def test_the_struct_of_the_device_form():
    before = launches()
    refused(device(dtype=2), "dtype 2 is neither SGA_F32 nor SGA_F64")
    refused(device(cols=0), "dim must be in [1,32], got 0")
    refused(device(cols=33, stride=40), "dim must be in [1,32], got 33")
    refused(device(cols=3, stride=2), "stride 2 < cols 3")
    assert launches() == before
    arr = api._device_array(STAND_IN, 2, 1, 1)
    out = C.c_void_p(SENTINEL)
    assert sga.load().sga_features_create_device(C.c_void_p(STAND_IN), C.byref(arr), 10, None, 0, C.byref(out)) == INVALID and "dtype 2" in message() and not out.value
    assert sga.load().sga_features_create_device(C.c_void_p(STAND_IN), None, 10, None, 0, C.byref(out)) == INVALID and "null argument" in message()
    assert sga.load().sga_features_export_device(C.c_void_p(STAND_IN), None, C.byref(arr), None, 0) == INVALID and "null argument" in message()


def test_reduce_names():
    assert list(api._reduce_ops("nearest", 3)) == [4, 4, 4]
    assert list(api._reduce_ops(["mean", "MIN", "max", "first", "nearest"], 5)) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="column 1"):
        api._reduce_ops(["mean", "median"], 2)
    with pytest.raises(ValueError, match="2 columns"):
        api._reduce_ops(["mean", "min"], 3)

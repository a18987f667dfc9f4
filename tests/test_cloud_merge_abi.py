"""The boundary of sga_cloud_merge / sga_cloud_transform without a device: the symbols exist and are bound with
the header's signatures; null arguments, a NULL member (named by number) and a non-finite entry of a pose or of the origin are refused
before any member is read — the members handed in are stand-ins at an address nothing is mapped at, so reading one would end the
process — and *out is NULL after every refusal; count == 0 is SGA_OK and makes an empty cloud.  (An empty merge reads one thing of its
context, the device number its cloud belongs to: the context of that case is a zeroed block, device 0.)  What needs live clouds — another
device, the point limit, every result — is tests/test_cloud_merge_gpu.py's."""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api

OK, INVALID = 0, 1
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
IDENTITY = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def message():
    return sga.load().sga_last_error().decode()


def poses(count, bad=None):
    T = (C.c_double * (16 * count))(*(IDENTITY * count))
    if bad is not None:
        T[bad[0]] = bad[1]
    return T


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_cloud_merge", "sga_cloud_transform", "sga_debug_cloud_merge_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _dp, _pvp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_void_p)
    assert bound["sga_cloud_merge"] == (C.c_int, [_vp, _pvp, _dp, C.c_size_t, _dp, _pvp])  # ctx, clouds, T, count, origin, out
    assert bound["sga_cloud_transform"] == (C.c_int, [_vp, _vp, _dp, _dp, _pvp])  # ctx, cloud, T, origin, out
    assert bound["sga_debug_cloud_merge_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("merge_clouds", "cloud_merge_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.transformed)
    from small_gicp_amd import odometry

    assert callable(odometry.run_synthetic_submap) and callable(odometry.SubmapOdometry)


def test_refusals_come_before_any_member_is_read():
    lib = sga.load()
    ctx = C.c_void_p(STAND_IN)
    clouds = handles(STAND_IN, STAND_IN, STAND_IN)
    out = C.c_void_p(STAND_IN)

    def refused(rc, text):
        assert rc == INVALID and text in message(), (rc, message())
        assert out.value is None  # on any failure *out is NULL
        out.value = STAND_IN

    # null arguments
    refused(lib.sga_cloud_merge(None, clouds, None, 3, None, C.byref(out)), "null argument")
    refused(lib.sga_cloud_merge(ctx, None, None, 3, None, C.byref(out)), "null argument")
    assert lib.sga_cloud_merge(ctx, clouds, None, 3, None, None) == INVALID and "null argument" in message()
    refused(lib.sga_cloud_merge(None, None, None, 0, None, C.byref(out)), "null argument")
    # a NULL member is named (the stand-ins around it are not read)
    refused(lib.sga_cloud_merge(ctx, handles(STAND_IN, None, STAND_IN), None, 3, None, C.byref(out)), "clouds[1] is NULL")
    assert "null argument" in message()
    refused(lib.sga_cloud_merge(ctx, handles(None, STAND_IN), poses(2), 2, None, C.byref(out)), "clouds[0] is NULL")
    refused(lib.sga_cloud_transform(ctx, None, poses(1), None, C.byref(out)), "clouds[0] is NULL")
    # a non-finite entry of a pose is named by its member; of the origin
    for value in (float("nan"), float("inf"), -float("inf")):
        refused(lib.sga_cloud_merge(ctx, clouds, poses(3, (16 * 2 + 13, value)), 3, None, C.byref(out)), "pose 2 has a non-finite entry")
        refused(lib.sga_cloud_merge(ctx, clouds, poses(3, (5, value)), 3, None, C.byref(out)), "pose 0 has a non-finite entry")
        refused(lib.sga_cloud_transform(ctx, C.c_void_p(STAND_IN), poses(1, (0, value)), None, C.byref(out)), "pose 0 has a non-finite entry")
        refused(lib.sga_cloud_merge(ctx, clouds, poses(3), 3, (C.c_double * 3)(0.0, value, 0.0), C.byref(out)), "origin has a non-finite entry")
    # more than 2^15 members: refused by the count alone
    many = (C.c_void_p * ((1 << 15) + 1))()
    refused(lib.sga_cloud_merge(ctx, many, None, (1 << 15) + 1, None, C.byref(out)), "too many members")
    before = api.cloud_merge_launches()
    assert isinstance(before, int) and api.cloud_merge_launches() == before  # a refusal enqueues nothing
    assert lib.sga_debug_cloud_merge_launches(None) == INVALID


@pytest.mark.parametrize("origin", [None, (256.0, -128.0, 0.0)])
def test_count_zero_is_ok_and_makes_an_empty_cloud(origin):
    lib = sga.load()
    block = (C.c_char * 65536)()  # a zeroed stand-in for a context: an empty merge reads its device number and nothing else
    ctx = C.cast(block, C.c_void_p)
    out = C.c_void_p()
    before = api.cloud_merge_launches()
    o = None if origin is None else (C.c_double * 3)(*origin)
    assert lib.sga_cloud_merge(ctx, None, None, 0, o, C.byref(out)) == OK and out.value
    n, has_n, has_c, got = C.c_size_t(7), C.c_int(7), C.c_int(7), (C.c_double * 3)(7, 7, 7)
    assert lib.sga_cloud_size(out, C.byref(n)) == OK and n.value == 0
    assert lib.sga_cloud_has(out, C.byref(has_n), C.byref(has_c)) == OK and (has_n.value, has_c.value) == (0, 0)
    assert lib.sga_cloud_origin(out, got) == OK and tuple(got) == (origin or (0.0, 0.0, 0.0))
    assert api.cloud_merge_launches() == before  # no device work
    assert lib.sga_cloud_destroy(out) == OK


def test_python_layer_refuses_what_is_not_a_point_cloud():
    pts = np.zeros((4, 3), np.float32)
    for bad in ([pts], [None], ["cloud"], [object()]):
        with pytest.raises(TypeError):
            sga.merge_clouds(bad)

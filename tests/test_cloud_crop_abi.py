"""The boundary of sga_cloud_crop / _batch / _device and sga_cloud_select without a device: the symbols exist and
are bound with the header's signatures, sizeof(sga_crop) is the ctypes structure's, sga_crop_default gives the defaults; null arguments, a
NULL member (named by number), every bad field of a crop (named by member and field) and too many members are refused before any handle
is read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_deskew_abi.py's technique) — with every out[k]
NULL afterwards and nothing enqueued; count == 0 is SGA_OK; random_sampling's choice of indices is distinct, ascending and reproducible.
What needs live clouds is tests/test_cloud_crop_gpu.py's."""
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


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def message():
    return sga.load().sga_last_error().decode()


def crops(count, **fields):
    """`count` default crops; fields: name -> (member, value) or (member, axis, value)"""
    cs = (_lib.Crop * count)()
    for k in range(count):
        sga.load().sga_crop_default(C.byref(cs[k]))
    for name, spec in fields.items():
        if len(spec) == 2:
            setattr(cs[spec[0]], name, spec[1])
        else:
            getattr(cs[spec[0]], name)[spec[1]] = spec[2]
    return cs


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_crop_default", "sga_cloud_crop_batch", "sga_cloud_crop", "sga_cloud_crop_device", "sga_cloud_select", "sga_debug_cloud_crop_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _pvp, _pc, _pi = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(_lib.Crop), C.POINTER(C.c_int64)
    assert bound["sga_crop_default"] == (None, [_pc])
    assert bound["sga_cloud_crop_batch"] == (C.c_int, [_vp, _pvp, _pc, _pvp, C.c_size_t, _pvp])  # ctx, clouds, crops, kept, count, out
    assert bound["sga_cloud_crop"] == (C.c_int, [_vp, _vp, _pc, _pi, _pvp])  # ctx, cloud, crop, kept, out
    assert bound["sga_cloud_crop_device"] == (C.c_int, [_vp, _vp, _pc, _vp, _vp, C.c_int, _pvp])  # ctx, cloud, crop, d_kept, stream, flags, out
    assert bound["sga_cloud_select"] == (C.c_int, [_vp, _vp, _pi, C.c_size_t, _pvp])  # ctx, cloud, indices, m, out
    assert bound["sga_debug_cloud_crop_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("crop_clouds", "random_sampling", "random_sampling_indices", "cloud_crop_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.cropped) and callable(sga.PointCloud.selected)


def test_the_header_declares_what_is_bound():
    """the struct's fields in the header's order and types (3 + 2 + 3 + 3 doubles, two ints: 96 bytes, no padding), and each prototype"""
    text = open(os.path.join(ROOT, "include", "small_gicp_amd.h")).read()
    body = re.search(r"typedef struct sga_crop \{(.*?)\} sga_crop;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls == ["double center[3]", "double min_range, max_range", "double box_lo[3], box_hi[3]", "int box_mode", "int pad"]
    assert [f[0] for f in _lib.Crop._fields_] == ["center", "min_range", "max_range", "box_lo", "box_hi", "box_mode", "pad"]
    assert C.sizeof(_lib.Crop) == 11 * 8 + 2 * 4 == 96
    assert _lib.Crop.min_range.offset == 24 and _lib.Crop.box_lo.offset == 40 and _lib.Crop.box_mode.offset == 88
    flat = " ".join(text.split())
    for proto in (
        "void sga_crop_default(sga_crop* crop);",
        "int sga_cloud_crop_batch(sga_context* ctx, const sga_cloud* const* clouds, const sga_crop* crops /* count */, int64_t* const* kept /* count, or NULL; entries may be NULL */, size_t count, sga_cloud** out /* count */);",
        "int sga_cloud_crop(sga_context* ctx, const sga_cloud* cloud, const sga_crop* crop, int64_t* kept /* or NULL */, sga_cloud** out);",
        "int sga_cloud_crop_device(sga_context* ctx, const sga_cloud* cloud, const sga_crop* crop, int64_t* d_kept, void* user_stream, int flags, sga_cloud** out);",
        "int sga_cloud_select(sga_context* ctx, const sga_cloud* cloud, const int64_t* indices, size_t m, sga_cloud** out);",
    ):
        assert proto in flat, proto
    assert "int sga_debug_cloud_crop_launches(unsigned long long* launches);" in open(os.path.join(ROOT, "include", "small_gicp_amd_debug.h")).read()


def test_crop_default():
    cr = _lib.Crop()
    C.memset(C.byref(cr), 0xFF, C.sizeof(cr))
    sga.load().sga_crop_default(C.byref(cr))
    assert list(cr.center) == [0.0, 0.0, 0.0] and cr.min_range == 0.0 and cr.max_range == INF
    assert list(cr.box_lo) == [0.0, 0.0, 0.0] and list(cr.box_hi) == [0.0, 0.0, 0.0] and cr.box_mode == 0 and cr.pad == 0
    sga.load().sga_crop_default(None)  # (nothing to fill: no fault)
    # the Python layer builds the same struct from cropped()'s arguments
    py = api._crop(3.0, 80.0, center=(1, 2, 3), box=((-1, -2, -3), (4, 5, INF)), box_mode="outside")
    assert (py.min_range, py.max_range, list(py.center), list(py.box_lo), list(py.box_hi), py.box_mode) == (3.0, 80.0, [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0], [4.0, 5.0, INF], 2)
    assert api._crop().box_mode == 0 and api._crop(box=((0, 0, 0), (1, 1, 1))).box_mode == 1
    with pytest.raises(ValueError):
        api._crop(box=((0, 0, 0), (1, 1, 1)), box_mode="around")


def test_refusals_come_before_any_handle_is_read():
    lib = sga.load()
    ctx = C.c_void_p(STAND_IN)
    clouds = handles(STAND_IN, STAND_IN, STAND_IN)
    out = handles(STAND_IN, STAND_IN, STAND_IN)
    one = C.c_void_p(STAND_IN)
    cloud = C.c_void_p(STAND_IN)
    before = api.cloud_crop_launches()

    def refused(rc, text, lone=False):
        assert rc == INVALID and text in message(), (rc, message())
        if lone:
            assert one.value is None
            one.value = STAND_IN
        else:
            assert list(out) == [None, None, None]  # on any failure every out[k] is NULL
            for k in range(3):
                out[k] = STAND_IN

    # null arguments
    refused(lib.sga_cloud_crop_batch(None, clouds, crops(3), None, 3, out), "null argument")
    refused(lib.sga_cloud_crop_batch(ctx, None, crops(3), None, 3, out), "null argument")
    refused(lib.sga_cloud_crop_batch(ctx, clouds, None, None, 3, out), "null argument")
    assert lib.sga_cloud_crop_batch(ctx, clouds, crops(3), None, 3, None) == INVALID and "null argument" in message()
    assert lib.sga_cloud_crop(ctx, cloud, crops(1), None, None) == INVALID and "null argument" in message()
    assert lib.sga_cloud_crop_device(ctx, cloud, crops(1), None, None, 0, None) == INVALID and "null argument" in message()
    refused(lib.sga_cloud_crop(ctx, cloud, None, None, C.byref(one)), "null argument", lone=True)
    refused(lib.sga_cloud_crop_device(ctx, cloud, None, None, None, 0, C.byref(one)), "null argument", lone=True)
    # a NULL member is named (the stand-ins around it are not read)
    refused(lib.sga_cloud_crop_batch(ctx, handles(STAND_IN, None, STAND_IN), crops(3), None, 3, out), "clouds[1] is NULL")
    assert "null argument" in message()
    refused(lib.sga_cloud_crop(ctx, None, crops(1), None, C.byref(one)), "clouds[0] is NULL", lone=True)
    refused(lib.sga_cloud_crop_device(ctx, None, crops(1), None, None, 0, C.byref(one)), "clouds[0] is NULL", lone=True)
    # the fields of a crop: named by member and field
    bad = [
        (dict(min_range=(2, -1.0)), "crops[2]: min_range"),
        (dict(min_range=(0, NAN)), "crops[0]: min_range"),
        (dict(min_range=(1, -INF)), "crops[1]: min_range"),
        (dict(max_range=(1, NAN)), "crops[1]: max_range is NaN"),
        (dict(min_range=(1, 5.0), max_range=(1, 4.0)), "crops[1]: min_range > max_range"),
        (dict(min_range=(0, INF), max_range=(0, 1e300)), "crops[0]: min_range > max_range"),
        (dict(max_range=(2, -1.0)), "crops[2]: min_range > max_range"),
        (dict(center=(2, 1, NAN)), "crops[2]: center"),
        (dict(center=(0, 0, INF)), "crops[0]: center"),
        (dict(center=(1, 2, -INF)), "crops[1]: center"),
        (dict(box_mode=(1, 3)), "crops[1]: box_mode"),
        (dict(box_mode=(2, -1)), "crops[2]: box_mode"),
        (dict(box_mode=(0, 1), box_lo=(0, 1, NAN)), "crops[0]: box_lo / box_hi has a NaN"),
        (dict(box_mode=(2, 2), box_hi=(2, 0, NAN)), "crops[2]: box_lo / box_hi has a NaN"),
        (dict(box_mode=(1, 1), box_lo=(1, 2, 1.0), box_hi=(1, 2, 0.5)), "crops[1]: box_lo > box_hi on axis 2"),
        (dict(box_mode=(1, 2), box_lo=(1, 0, INF)), "crops[1]: box_lo > box_hi on axis 0"),
    ]
    for fields, text in bad:
        refused(lib.sga_cloud_crop_batch(ctx, clouds, crops(3, **fields), None, 3, out), text)
    for fields, text in bad:
        lone_fields = {name: (0,) + tuple(spec[1:]) for name, spec in fields.items()}
        want = "crops[0]" + text[text.index("]") + 1:]
        refused(lib.sga_cloud_crop(ctx, cloud, crops(1, **lone_fields), None, C.byref(one)), want, lone=True)
        refused(lib.sga_cloud_crop_device(ctx, cloud, crops(1, **lone_fields), None, None, 0, C.byref(one)), want, lone=True)
    # more than 2^15 members: refused by the count alone
    count = (1 << 15) + 1
    many, many_out = (C.c_void_p * count)(), (C.c_void_p * count)(*([STAND_IN] * count))
    assert lib.sga_cloud_crop_batch(ctx, many, crops(1), None, count, many_out) == INVALID and "too many members" in message()
    assert not any(many_out)
    # sga_cloud_select: null arguments
    idx = (C.c_int64 * 2)(0, 1)
    refused(lib.sga_cloud_select(None, cloud, idx, 2, C.byref(one)), "null argument", lone=True)
    refused(lib.sga_cloud_select(ctx, None, idx, 2, C.byref(one)), "null argument", lone=True)
    refused(lib.sga_cloud_select(ctx, cloud, None, 2, C.byref(one)), "null argument", lone=True)
    assert lib.sga_cloud_select(ctx, cloud, idx, 2, None) == INVALID and "null argument" in message()
    assert api.cloud_crop_launches() == before  # a refusal enqueues nothing
    assert lib.sga_debug_cloud_crop_launches(None) == INVALID


def test_a_box_that_is_not_tested_is_not_judged():
    """box_mode 0: the bounds are not looked at — a refusal further down the list shows that the crop itself passed"""
    lib = sga.load()
    one = C.c_void_p(STAND_IN)
    cs = crops(2, box_lo=(0, 0, NAN), box_hi=(0, 1, -INF), center=(1, 0, NAN))
    assert lib.sga_cloud_crop_batch(C.c_void_p(STAND_IN), handles(STAND_IN, STAND_IN), cs, None, 2, handles(STAND_IN, STAND_IN)) == INVALID
    assert "crops[1]: center" in message()
    # infinite bounds are fine
    cs = crops(2, box_mode=(0, 1), box_lo=(0, 0, -INF), box_hi=(0, 0, INF), max_range=(0, INF), center=(1, 0, NAN))
    assert lib.sga_cloud_crop_batch(C.c_void_p(STAND_IN), handles(STAND_IN, STAND_IN), cs, None, 2, handles(STAND_IN, STAND_IN)) == INVALID
    assert "crops[1]: center" in message()
    assert one.value == STAND_IN


def test_count_zero_is_ok():
    lib = sga.load()
    before = api.cloud_crop_launches()
    assert lib.sga_cloud_crop_batch(None, None, None, None, 0, None) == OK  # before anything is looked at
    out = handles(STAND_IN)
    assert lib.sga_cloud_crop_batch(C.c_void_p(STAND_IN), handles(STAND_IN), crops(1, min_range=(0, NAN)), None, 0, out) == OK and out[0] == STAND_IN  # nothing of the arrays is touched
    assert api.cloud_crop_launches() == before  # no device work
    assert sga.crop_clouds([], []) == [] and sga.crop_clouds([], [], return_kept=True) == ([], [])


def test_python_layer_refuses_what_does_not_fit():
    pts = np.zeros((4, 3), np.float32)
    for bad in ([pts], [None], ["cloud"]):
        with pytest.raises(TypeError):
            sga.crop_clouds(bad, [{}])
    with pytest.raises(ValueError):
        sga.crop_clouds([], [{}])


def test_random_sampling_indices():
    for n, m, seed in ((1000, 100, 1), (1000, 999, 2), (7, 3, 3), (100000, 5000, 4), (10, 0, 5)):
        idx = sga.random_sampling_indices(n, m, seed)
        assert idx.dtype == np.int64 and idx.shape == (m,)
        assert np.all(np.diff(idx) > 0)  # ascending and distinct
        assert m == 0 or (idx[0] >= 0 and idx[-1] < n)
        assert np.array_equal(idx, sga.random_sampling_indices(n, m, seed))  # the seed decides
    assert not np.array_equal(sga.random_sampling_indices(1000, 100, 1), sga.random_sampling_indices(1000, 100, 2))
    for n, m in ((10, 10), (10, 11), (0, 5)):
        assert np.array_equal(sga.random_sampling_indices(n, m, 0), np.arange(n))  # num_samples >= n: every point
    with pytest.raises(ValueError):
        sga.random_sampling_indices(10, -1)
    # every index is reachable (a choice that never reached the tail would still be ascending and distinct)
    seen = np.zeros(50, bool)
    for seed in range(200):
        seen[sga.random_sampling_indices(50, 5, seed)] = True
    assert seen.all()

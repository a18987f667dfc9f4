"""The boundary of sga_cloud_deskew / _batch / _device and of sga_se3_log without a device: the symbols exist and
are bound with the header's signatures; se3_log inverts se3_exp to a few eps64 at every angle from 0 to 3 rad; null arguments, a NULL
member or times array (named by number), a non-finite twist entry or reference time and too many members are refused before any handle
is read — the handles are stand-ins at an address nothing is mapped at (tests/test_cloud_merge_abi.py's technique) — with every out[k]
NULL afterwards and nothing enqueued; count == 0 is SGA_OK; and synthetic.kitti_like_sweep really is skewed and is straightened by the
twist it returns.  What needs live clouds is tests/test_cloud_deskew_gpu.py's."""
import ctypes as C

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import _lib, api, synthetic

OK, INVALID = 0, 1
STAND_IN = 0x1000  # never mapped: a handle at this address cannot be read
EPS64 = float(np.finfo(np.float64).eps)


def handles(*values):
    return (C.c_void_p * len(values))(*values)


def message():
    return sga.load().sga_last_error().decode()


def test_symbols_exist_and_are_bound():
    lib = C.CDLL(sga.LIB_PATH)
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("sga_cloud_deskew_batch", "sga_cloud_deskew", "sga_cloud_deskew_device", "sga_se3_log", "sga_debug_cloud_deskew_launches"):
        assert hasattr(lib, name), name
        assert name in bound, name
    _vp, _dp, _fp, _pvp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_void_p)
    assert bound["sga_cloud_deskew_batch"] == (C.c_int, [_vp, _pvp, _pvp, _dp, _dp, C.c_size_t, _pvp])  # ctx, clouds, times, twists, ref_times, count, out
    assert bound["sga_cloud_deskew"] == (C.c_int, [_vp, _vp, _fp, _dp, C.c_double, _pvp])  # ctx, cloud, times, twist, ref_time, out
    assert bound["sga_cloud_deskew_device"] == (C.c_int, [_vp, _vp, C.POINTER(_lib.DeviceArray), _dp, C.c_double, _vp, C.c_int, _pvp])  # ..., times, twist, ref_time, stream, flags, out
    assert bound["sga_se3_log"] == (None, [_dp, _dp])
    assert bound["sga_debug_cloud_deskew_launches"] == (C.c_int, [C.POINTER(C.c_ulonglong)])
    for name in ("se3_exp", "se3_log", "deskew_clouds", "cloud_deskew_launches"):
        assert callable(getattr(sga, name)) and callable(getattr(api, name)), name
    assert callable(sga.PointCloud.deskewed)
    assert callable(synthetic.kitti_like_sweep)


# ---- se3_log ------------------------------------------------------------------------------------------------------------------------------
ANGLES = (0.0, 1e-12, 1e-8, 1e-5, 1e-3, 0.1, 1.0, 3.0)


def test_se3_log_inverts_se3_exp_at_every_angle():
    """200 seeded twists: rotation angles from ANGLES about random axes, translations up to 10 m.  Entry-wise 256 eps64 (1 + |t|) for the
    poses and for the twists, the latter scaled by 1 / (pi - theta) at theta = 3.  The bound follows from a well-conditioned evaluation (no
    coefficient is a difference of nearly equal numbers; V is inverted at a condition number below pi / 2; towards pi the axis is read from
    R - R^T, whose entries shrink like pi - theta): the worst ratios printed are what is left of it."""
    rng = np.random.default_rng(2024)
    worst_T, worst_xi = 0.0, 0.0
    for j in range(200):
        theta = ANGLES[j % len(ANGLES)]
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        v = rng.uniform(-1.0, 1.0, 3)
        v *= rng.uniform(0.0, 10.0) / np.linalg.norm(v)
        xi = np.concatenate([theta * axis, v])
        T = sga.se3_exp(xi)
        assert T.shape == (4, 4) and np.array_equal(T[3], [0.0, 0.0, 0.0, 1.0])
        assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 16 * EPS64
        back = sga.se3_log(T)
        bound = 256 * EPS64 * (1.0 + np.linalg.norm(T[:3, 3]))
        bound_xi = bound / (np.pi - theta) if theta >= 3.0 else bound
        e_T, e_xi = np.abs(sga.se3_exp(back) - T).max(), np.abs(back - xi).max()
        worst_T, worst_xi = max(worst_T, e_T / bound), max(worst_xi, e_xi / bound_xi)
        assert e_T <= bound, (j, theta, e_T, bound)
        assert e_xi <= bound_xi, (j, theta, e_xi, bound_xi)
    print("se3_log round trips: worst error / bound %.4f (poses) %.4f (twists)" % (worst_T, worst_xi))
    zero = sga.se3_log(np.eye(4))
    assert zero.tobytes() == np.zeros(6).tobytes()  # exactly, and no -0
    assert np.array_equal(sga.se3_exp(np.zeros(6)), np.eye(4))


def test_se3_exp_keeps_its_digits_where_the_textbook_form_loses_them():
    """theta = 1e-5, |v| = 10: t = V v with V = I + B W + C W^2; against the series of B and C in float64 (exact to eps there) the
    translation holds 256 eps64 (1 + |t|) — (1 - cos theta) / theta^2 evaluated as written is off by 1e-6 of B, 5e-11 m here"""
    w = 1e-5 * np.array([0.6, 0.0, -0.8])
    v = np.array([6.0, -8.0, 0.0])
    th2 = float(w @ w)
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    V = np.eye(3) + (0.5 - th2 / 24.0) * W + (1.0 / 6.0 - th2 / 120.0) * (W @ W)
    T = sga.se3_exp(np.concatenate([w, v]))
    assert np.abs(T[:3, 3] - V @ v).max() <= 256 * EPS64 * 11.0


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def twists(count, bad=None):
    xi = (C.c_double * (6 * count))(*([0.0, 0.0, 0.01, 1.0, 0.0, 0.0] * count))
    if bad is not None:
        xi[bad[0]] = bad[1]
    return xi


def test_refusals_come_before_any_handle_is_read():
    lib = sga.load()
    ctx = C.c_void_p(STAND_IN)
    clouds, times = handles(STAND_IN, STAND_IN, STAND_IN), handles(STAND_IN, STAND_IN, STAND_IN)
    out = handles(STAND_IN, STAND_IN, STAND_IN)
    one = C.c_void_p(STAND_IN)
    before = api.cloud_deskew_launches()

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
    refused(lib.sga_cloud_deskew_batch(None, clouds, times, twists(3), None, 3, out), "null argument")
    refused(lib.sga_cloud_deskew_batch(ctx, None, times, twists(3), None, 3, out), "null argument")
    refused(lib.sga_cloud_deskew_batch(ctx, clouds, None, twists(3), None, 3, out), "null argument")
    refused(lib.sga_cloud_deskew_batch(ctx, clouds, times, None, None, 3, out), "null argument")
    assert lib.sga_cloud_deskew_batch(ctx, clouds, times, twists(3), None, 3, None) == INVALID and "null argument" in message()
    assert lib.sga_cloud_deskew(ctx, C.c_void_p(STAND_IN), C.cast(STAND_IN, C.POINTER(C.c_float)), twists(1), 1.0, None) == INVALID and "null argument" in message()
    refused(lib.sga_cloud_deskew(ctx, C.c_void_p(STAND_IN), C.cast(STAND_IN, C.POINTER(C.c_float)), None, 1.0, C.byref(one)), "null argument", lone=True)
    refused(lib.sga_cloud_deskew_device(ctx, C.c_void_p(STAND_IN), None, twists(1), 1.0, None, 0, C.byref(one)), "null argument", lone=True)
    # a NULL member and a NULL times array are named (the stand-ins around them are not read)
    refused(lib.sga_cloud_deskew_batch(ctx, handles(STAND_IN, None, STAND_IN), times, twists(3), None, 3, out), "clouds[1] is NULL")
    assert "null argument" in message()
    refused(lib.sga_cloud_deskew_batch(ctx, clouds, handles(STAND_IN, None, STAND_IN), twists(3), None, 3, out), "times[1] is NULL")
    assert "null argument" in message()
    refused(lib.sga_cloud_deskew(ctx, None, C.cast(STAND_IN, C.POINTER(C.c_float)), twists(1), 1.0, C.byref(one)), "clouds[0] is NULL", lone=True)
    refused(lib.sga_cloud_deskew(ctx, C.c_void_p(STAND_IN), None, twists(1), 1.0, C.byref(one)), "times[0] is NULL", lone=True)
    # a non-finite entry of a twist, a non-finite reference time: named by member
    da = _lib.DeviceArray()
    da.data, da.dtype, da.cols, da.stride = STAND_IN, _lib.F32, 1, 1
    for value in (float("nan"), float("inf"), -float("inf")):
        refused(lib.sga_cloud_deskew_batch(ctx, clouds, times, twists(3, (6 * 2 + 4, value)), None, 3, out), "twist 2 has a non-finite entry")
        refused(lib.sga_cloud_deskew_batch(ctx, clouds, times, twists(3, (1, value)), None, 3, out), "twist 0 has a non-finite entry")
        refused(lib.sga_cloud_deskew_batch(ctx, clouds, times, twists(3), (C.c_double * 3)(1.0, value, 0.0), 3, out), "reference time 1 is not finite")
        refused(lib.sga_cloud_deskew(ctx, C.c_void_p(STAND_IN), C.cast(STAND_IN, C.POINTER(C.c_float)), twists(1, (5, value)), 1.0, C.byref(one)), "twist 0 has a non-finite entry", lone=True)
        refused(lib.sga_cloud_deskew(ctx, C.c_void_p(STAND_IN), C.cast(STAND_IN, C.POINTER(C.c_float)), twists(1), value, C.byref(one)), "reference time 0 is not finite", lone=True)
        refused(lib.sga_cloud_deskew_device(ctx, C.c_void_p(STAND_IN), C.byref(da), twists(1), value, None, 0, C.byref(one)), "reference time 0 is not finite", lone=True)
    # the layout of device times: refused from the struct alone
    for dtype, cols, stride in ((7, 1, 1), (_lib.F32, 3, 3), (_lib.F64, 1, 0)):
        da.dtype, da.cols, da.stride = dtype, cols, stride
        refused(lib.sga_cloud_deskew_device(ctx, C.c_void_p(STAND_IN), C.byref(da), twists(1), 1.0, None, 0, C.byref(one)), "times:", lone=True)
    # more than 2^15 members: refused by the count alone
    count = (1 << 15) + 1
    many, many_out = (C.c_void_p * count)(), (C.c_void_p * count)(*([STAND_IN] * count))
    assert lib.sga_cloud_deskew_batch(ctx, many, many, twists(count), None, count, many_out) == INVALID and "too many members" in message()
    assert not any(many_out)
    assert api.cloud_deskew_launches() == before  # a refusal enqueues nothing
    assert lib.sga_debug_cloud_deskew_launches(None) == INVALID


def test_count_zero_is_ok():
    lib = sga.load()
    before = api.cloud_deskew_launches()
    assert lib.sga_cloud_deskew_batch(C.c_void_p(STAND_IN), None, None, None, None, 0, None) == OK
    out = handles(STAND_IN)
    assert lib.sga_cloud_deskew_batch(C.c_void_p(STAND_IN), handles(STAND_IN), handles(STAND_IN), twists(1), None, 0, out) == OK and out[0] == STAND_IN  # nothing of the arrays is touched
    assert api.cloud_deskew_launches() == before  # no device work
    assert sga.deskew_clouds([], [], np.zeros((0, 6))) == []


def test_python_layer_refuses_what_does_not_fit():
    pts = np.zeros((4, 3), np.float32)
    for bad in ([pts], [None], ["cloud"]):
        with pytest.raises(TypeError):
            sga.deskew_clouds(bad, [np.zeros(4)], np.zeros((1, 6)))


# ---- the synthetic sweep ------------------------------------------------------------------------------------------------------------------
def wall_residuals(points, T_world_sensor, surface):
    """|distance to its wall's plane| of every wall return, the points mapped to the world by the pose"""
    centers, _, _, along_x = synthetic._walls(12345)
    world = points @ T_world_sensor[:3, :3].T + T_world_sensor[:3, 3]
    on_wall = surface >= 0
    w = surface[on_wall]
    axis = np.where(along_x[w], 1, 0)  # a wall's plane is constant in this axis
    return np.abs(world[on_wall][np.arange(len(w)), axis] - centers[w, axis])


def test_kitti_like_sweep_is_skewed_and_its_twist_straightens_it():
    pts, times, T_end, xi, surface = synthetic.kitti_like_sweep(3, n_rings=16, n_az=256, noise=0)
    assert pts.dtype == np.float32 and times.dtype == np.float32 and pts.shape == (len(times), 3) and surface.shape == times.shape
    assert xi.shape == (6,) and (surface >= 0).sum() > 500 and (surface == -1).sum() > 500
    assert 0.0 < times.min() < 0.01 and 0.99 < times.max() < 1.0
    assert np.allclose(T_end, synthetic.kitti_like_scan(3, n_rings=16, n_az=256, noise=0)[1], atol=0) and np.linalg.norm(xi[3:]) == pytest.approx(1.0, abs=1e-3)
    P = pts.astype(np.float64)
    # the host deskew in float64: p' = exp((s - 1) xi) p
    poses = {float(s): sga.se3_exp((float(s) - 1.0) * xi) for s in np.unique(times)}
    D = np.stack([poses[float(s)][:3, :3] @ p + poses[float(s)][:3, 3] for p, s in zip(P, times)])
    raw, straight = wall_residuals(P, T_end, surface), wall_residuals(D, T_end, surface)
    print("wall returns %d: worst distance to the wall's plane raw %.3f m, deskewed %.2e m" % (len(raw), raw.max(), straight.max()))
    assert straight.max() <= 1e-4  # about five times the two fp32 roundings at 80 m
    assert raw.max() > 0.1  # the sweep really is skewed
    with pytest.raises(ValueError):
        synthetic.kitti_like_sweep(0)

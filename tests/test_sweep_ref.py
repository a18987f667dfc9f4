"""The numpy restatement of sweep registration (tests/sweep_ref.py) checked against itself, without a device: its
analytic Jacobian against central differences of its own residual, its left Jacobian against identities that need no logarithm, and its
LM loop on the reduced frame-3 pair that tests/test_sweep_gpu.py registers on the device.  Also here: kitti_like_sweep, now written over
sweep_between, returns the bytes it returned before, and slalom_pose follows the law its docstring states."""
import hashlib

import numpy as np
import pytest

import sweep_ref as R
from small_gicp_amd import synthetic as syn

# The reduction of frame 3 that both this file and the GPU test register: 32 rings x 250 columns = 8 000 rays, 7 437 returns against the
# 7 417 of the snapshot of frame 2.  The 2 000-ray reductions (16 x 125, 8 x 250) do not hold the bounds below in the restatement itself —
# the pose comes within 42 mm / 7.5 mrad and 143 mm / 8.7 mrad, the rotation worse than a tenth of the held-twist loop's 19 mrad — and
# neither do 16 x 250, 32 x 125 or 24 x 250: with fewer rings the walls constrain the rotation rate too weakly.
RINGS, COLUMNS, FRAME = 32, 250, 3


def frame3_pair():
    pts, times, T1, xi, _ = syn.kitti_like_sweep(FRAME, n_rings=RINGS, n_az=COLUMNS)
    tgt, T0 = syn.kitti_like_scan(FRAME - 1, n_rings=RINGS, n_az=COLUMNS)
    return tgt, pts, times, np.linalg.inv(T0) @ T1, xi


CASES = [  # (a, xi): a xi of 0, 1e-9, 0.05 rad with 1 m, and 1 rad with 3 m
    (0.0, [0.3, -0.2, 0.1, 1.0, 2.0, -0.5]),
    (-1e-9, [0.6, 0.5, -0.62, 0.3, -0.4, 0.2]),
    (-0.5, [0.06, -0.04, 0.0693, 1.2, -1.2, 1.058]),
    (-1.0, [0.6, -0.64, 0.48, 2.0, -1.0, 2.0]),
]


@pytest.mark.parametrize("a, xi", CASES)
def test_analytic_jacobian_matches_central_differences(a, xi):
    xi = np.array(xi)
    rng = np.random.default_rng(11)
    T = R.se3_exp(np.array([0.2, -0.1, 0.4, 1.0, -2.0, 0.5]))
    points = rng.uniform(-10, 10, size=(5, 3))
    target = rng.uniform(-10, 10, size=(5, 3))
    ref_time = 0.0  # (so that float32 keeps a = -1e-9)
    times = np.full(5, np.float32(a))
    a_used = float(times[0]) - ref_time
    angle = {0.0: 0.0, 1e-9: 1e-9, 0.5: 0.05, 1.0: 1.0}[abs(a)]
    assert abs(np.linalg.norm(a_used * xi[:3]) - angle) <= 0.01 * angle and (a_used != 0.0) == (a != 0.0)
    j = np.arange(5)
    r0, J, _ = R.residual_and_jacobian(target, points, times, T, xi, ref_time, j)
    h = 1e-6
    num = np.zeros_like(J)
    for c in range(12):
        d = np.zeros(12)
        d[c] = h
        rp = R.residual_and_jacobian(target, points, times, T @ R.se3_exp(d[:6]), xi + d[6:], ref_time, j)[0]
        rm = R.residual_and_jacobian(target, points, times, T @ R.se3_exp(-d[:6]), xi - d[6:], ref_time, j)[0]
        num[:, :, c] = (rp - rm) / (2 * h)
    # J is dr / d(delta) for T <- T exp(delta[0:6]), xi <- xi + delta[6:12]
    for i in range(5):
        scale = np.abs(J[i]).max()
        assert np.abs(num[i] - J[i]).max() <= 1e-7 * scale, (i, np.abs(num[i] - J[i]).max() / scale)
    if a_used == 0.0:
        assert (J[:, :, 6:] == 0.0).all()


def test_left_jacobian_identities():
    assert np.array_equal(R.left_jacobian(np.zeros(6)), np.eye(6))
    rng = np.random.default_rng(5)
    for x in ([0.6, -0.64, 0.48, 2.0, -1.0, 2.0], [1e-9, 0, 0, 0, 1e-9, 0], [0.03, 0.02, -0.03, 0.5, 0.5, 0.7]):
        x = np.array(x)
        Jl = R.left_jacobian(x)
        errs = []
        for step in (1e-3, 5e-4):
            d = step * rng.normal(size=6) / np.sqrt(6)
            errs.append(np.abs(R.se3_exp(x + d) - R.se3_exp(Jl @ d) @ R.se3_exp(x)).max())
            assert errs[-1] <= 20 * step * step, (x, step, errs)  # second order in d


def test_lm_recovers_pose_and_twist_from_nothing():
    tgt, pts, times, T_true, xi_true = frame3_pair()
    t, p = tgt.astype(np.float64), pts.astype(np.float64)
    kw = dict(target_covs=R.estimate_covariances(t, 10), source_covs=R.estimate_covariances(p, 10), max_dist_sq=1.0)
    free = R.lm(R.GICP, t, p, times, **kw)
    held = R.lm(R.GICP, t, p, times, hold_twist=True, **kw)  # the twist held at zero: the raw sweep registered as if it were rigid
    ft, fr = R.pose_error(free.T_target_source, T_true)
    ht, hr = R.pose_error(held.T_target_source, T_true)
    print("free twist: %.4f m %.5f rad; twist held at zero: %.4f m %.5f rad" % (ft, fr, ht, hr))
    assert free.converged
    assert ft < 0.1 * ht and fr < 0.1 * hr, (ft, fr, ht, hr)
    dv, dw = np.linalg.norm(free.twist[3:] - xi_true[3:]), np.linalg.norm(free.twist[:3] - xi_true[:3])
    print("twist error: %.4f m %.5f rad" % (dv, dw))
    assert dv < 0.05 and dw < 5e-3, (dv, dw)


def digest(out):
    h = hashlib.sha256()
    for a in out:
        a = np.ascontiguousarray(a)
        h.update(str(a.dtype).encode() + str(a.shape).encode() + a.tobytes())
    return h.hexdigest()


@pytest.mark.parametrize(
    "args, sha",
    [  # the digests of the function as it was before sweep_between existed
        (dict(frame=3, n_rings=8, n_az=250), "c5d9c0386374824a159e08248ee8629b7200a6dbe9d63658759ecb17436cd991"),
        (dict(frame=1, n_rings=4, n_az=64, noise=0.05, seed=5), "993107c4af31b33fe2a37c98ed1c63031da5408718af76eb773cc4e65cbc0d1f"),
        (dict(frame=6, n_rings=16, n_az=500, layout_seed=99), "7cc79c54156d107e5f7a59f1671b22ec4b4f3acf683499bf5d255f3ec2bc958a"),
    ],
)
def test_kitti_like_sweep_is_unchanged_byte_for_byte(args, sha):
    assert digest(syn.kitti_like_sweep(**args)) == sha


def test_sweep_between_is_the_casting_of_kitti_like_sweep():
    a = syn.kitti_like_sweep(4, n_rings=4, n_az=100)
    b = syn.sweep_between(syn._sensor_pose(3), syn._sensor_pose(4), n_rings=4, n_az=100, seed=777 + 4)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    with pytest.raises(ValueError):
        syn.kitti_like_sweep(0)


def test_slalom_pose_follows_its_law():
    assert np.allclose(syn.slalom_pose(0), [[1, 0, 0, -30], [0, 1, 0, -20], [0, 0, 1, 1.8], [0, 0, 0, 1]])
    steps, turns = [], []
    for f in range(8):
        A, B = syn.slalom_pose(f), syn.slalom_pose(f + 1)
        rel = np.linalg.inv(A) @ B
        steps.append(rel[0, 3])
        turns.append(np.arctan2(rel[1, 0], rel[0, 0]))
        assert abs(rel[1, 3]) < 1e-12 and abs(rel[2, 3]) < 1e-12  # it advances along its heading
    assert np.allclose(steps, [1.0 + 0.5 * np.sin(0.9 * f) for f in range(8)])
    assert np.allclose(turns, [np.deg2rad(3.0 * np.sin(1.3 * f)) for f in range(8)])
    assert max(np.abs(np.diff(steps))) > 0.3 and max(np.abs(np.diff(turns))) > np.deg2rad(2.0)  # the motion changes from frame to frame

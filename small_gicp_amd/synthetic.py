"""Frozen synthetic workloads for the BASELINE.json configs.  The reference ships no data at these
sizes, so these generators ARE the definition of C2-C5; they are deterministic in (n, seed).

scene(n, seed): LiDAR-like mixture of planar patches in a 100 m x 100 m x 15 m volume —
  40 % ground plane z = 0 over [-50,50]^2, 50 % on 30 axis-aligned vertical walls of random extent 2-20 m and height
  2-10 m, 10 % uniform clutter in [-50,50]^2 x [0,5]; Gaussian noise sigma = 0.01 m; float32.
The wall layout depends only on `layout_seed`, so two calls with different `seed` resample the SAME surfaces.
"""
import numpy as np


def _rot(axis, angle):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def gt_transform():
    """T_target_source of C2/C3/C4: 2 deg about (0.2, 0.3, 0.93) and t = (0.30, -0.20, 0.05)."""
    T = np.eye(4)
    T[:3, :3] = _rot([0.2, 0.3, 0.93], np.deg2rad(2.0))
    T[:3, 3] = [0.30, -0.20, 0.05]
    return T


def scene(n, seed, layout_seed=12345, noise=0.01):
    lay = np.random.default_rng(layout_seed)
    nwalls = 30
    centers = lay.uniform(-45, 45, size=(nwalls, 2))
    lengths = lay.uniform(2, 20, size=nwalls)
    heights = lay.uniform(2, 10, size=nwalls)
    along_x = lay.integers(0, 2, size=nwalls).astype(bool)
    rng = np.random.default_rng(seed)
    n_ground = int(0.4 * n)
    n_clutter = int(0.1 * n)
    n_wall = n - n_ground - n_clutter
    ground = np.stack([rng.uniform(-50, 50, n_ground), rng.uniform(-50, 50, n_ground), np.zeros(n_ground)], axis=1)
    area = lengths * heights
    which = rng.choice(nwalls, size=n_wall, p=area / area.sum())
    u = rng.uniform(-0.5, 0.5, n_wall) * lengths[which]
    v = rng.uniform(0, 1, n_wall) * heights[which]
    wx = np.where(along_x[which], centers[which, 0] + u, centers[which, 0])
    wy = np.where(along_x[which], centers[which, 1], centers[which, 1] + u)
    walls = np.stack([wx, wy, v], axis=1)
    clutter = np.stack([rng.uniform(-50, 50, n_clutter), rng.uniform(-50, 50, n_clutter), rng.uniform(0, 5, n_clutter)], axis=1)
    pts = np.concatenate([ground, walls, clutter], axis=0)
    pts += rng.normal(0, noise, size=pts.shape)
    pts = pts[rng.permutation(len(pts))]
    return np.ascontiguousarray(pts, dtype=np.float32)


def bumpy_terrain(n, seed, layout_seed=2024, noise=0.01):
    """A terrain with shape of its own — what descriptors need, and what the plane and the axis-aligned walls of scene() lack: 40
    Gaussian bumps (centres uniform in +-20 m, heights uniform in [0.5, 3] m, widths uniform in [1, 4] m, all from
    default_rng(layout_seed)); x and y uniform in +-20 m from default_rng(seed), z the sum of the bumps, N(0, noise) on all three axes;
    float32.  Two calls with different `seed` resample the SAME surface."""
    lay = np.random.default_rng(layout_seed)
    centres = lay.uniform(-20, 20, size=(40, 2))
    heights = lay.uniform(0.5, 3.0, size=40)
    widths = lay.uniform(1.0, 4.0, size=40)
    rng = np.random.default_rng(seed)
    x = rng.uniform(-20, 20, n)
    y = rng.uniform(-20, 20, n)
    z = np.zeros(n)
    for c, h, w in zip(centres, heights, widths):
        z += h * np.exp(-((x - c[0]) ** 2 + (y - c[1]) ** 2) / (2.0 * w * w))
    pts = np.stack([x, y, z], axis=1)
    pts += rng.normal(0, noise, size=pts.shape)
    return np.ascontiguousarray(pts, dtype=np.float32)


def registration_pair(n, target_seed=1, source_seed=2):
    """(target, source, T_gt): independent resamples of one scene; the source is expressed in a frame displaced by T_gt^-1."""
    T = gt_transform()
    target = scene(n, target_seed)
    src_world = scene(n, source_seed).astype(np.float64)
    Ti = np.linalg.inv(T)
    source = (src_world @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return target, source, T


def _walls(layout_seed):
    lay = np.random.default_rng(layout_seed)
    nwalls = 30
    centers = lay.uniform(-45, 45, size=(nwalls, 2))
    lengths = lay.uniform(2, 20, size=nwalls)
    heights = lay.uniform(2, 10, size=nwalls)
    along_x = lay.integers(0, 2, size=nwalls).astype(bool)
    return centers, lengths, heights, along_x


def _sensor_pose(frame):
    """T_world_sensor of a frame: 1.8 m above ground, 1 m/frame on a gentle arc starting near the scene centre, 1 deg/frame yaw"""
    yaw = np.deg2rad(1.0 * frame)
    pos = np.array([-30.0, -20.0, 1.8])
    for f in range(frame):
        a = np.deg2rad(1.0 * f)
        pos = pos + np.array([np.cos(a), np.sin(a), 0.0])
    Tws = np.eye(4)
    Tws[:3, :3] = _rot([0, 0, 1], yaw)
    Tws[:3, 3] = pos
    return Tws


def _ring_directions(n_rings, n_az):
    """unit rays of the sensor frame, ring-major: ray ring * n_az + column"""
    el = np.deg2rad(np.linspace(-24.8, 2.0, n_rings))
    az = np.linspace(-np.pi, np.pi, n_az, endpoint=False)
    EL, AZ = np.meshgrid(el, az, indexing="ij")
    return np.stack([np.cos(EL) * np.cos(AZ), np.cos(EL) * np.sin(AZ), np.sin(EL)], axis=-1).reshape(-1, 3)


def _cast(o, d, layout):
    """Rays o + t d (o: one origin (3,) or one per ray (N,3); d (N,3), world frame) against the ground plane and the walls, analytically:
    (range of the nearest hit or inf, the surface it belongs to: -1 ground, else the wall number)"""
    centers, lengths, heights, along_x = layout
    t_best = np.full(len(d), np.inf)
    surface = np.full(len(d), -1)
    # ground z = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        tg = -o[..., 2] / d[:, 2]
        hit = o + tg[:, None] * d
    ok = (tg > 0) & np.isfinite(tg)
    ok &= (np.abs(hit[:, 0]) <= 50) & (np.abs(hit[:, 1]) <= 50)
    t_best = np.where(ok, tg, t_best)
    for w in range(len(lengths)):
        ax = 1 if along_x[w] else 0  # wall plane is constant in this axis
        other = 1 - ax
        with np.errstate(divide="ignore", invalid="ignore"):
            tw = (centers[w, ax] - o[..., ax]) / d[:, ax]
            hitw = o + tw[:, None] * d
        okw = (tw > 0) & np.isfinite(tw) & (np.abs(hitw[:, other] - centers[w, other]) <= 0.5 * lengths[w]) & (hitw[:, 2] >= 0) & (hitw[:, 2] <= heights[w])
        nearer = okw & (tw < t_best)
        t_best = np.where(nearer, tw, t_best)
        surface = np.where(nearer, w, surface)
    return t_best, surface


def kitti_like_scan(frame, n_rings=64, n_az=2030, layout_seed=12345, noise=0.02, seed=777):
    """C5: one ~130k-return scan of the scene from a sensor 1.8 m above ground moving 1 m/frame with 1 deg/frame yaw.
    Rays are cast against the ground plane and the 30 walls analytically; returns beyond 80 m or closer than 3 m are dropped.
    Returns (points in the sensor frame float32 (N,3), T_world_sensor)."""
    Tws = _sensor_pose(frame)
    d_s = _ring_directions(n_rings, n_az)
    d = d_s @ Tws[:3, :3].T
    t_best, _ = _cast(Tws[:3, 3], d, _walls(layout_seed))
    keep = np.isfinite(t_best) & (t_best >= 3.0) & (t_best <= 80.0)
    rng = np.random.default_rng(seed + frame)
    r = t_best[keep] + rng.normal(0, noise, keep.sum())
    pts = d_s[keep] * r[:, None]
    return np.ascontiguousarray(pts, dtype=np.float32), Tws


def scan_at(T_world_sensor, n_rings=64, n_az=2030, layout_seed=12345, noise=0.02, seed=777):
    """The scan of the scene of kitti_like_scan from ANY sensor pose (a revisit from another heading, a keyframe off the arc): the same
    rays, the same casting, the same range gate (3 m .. 80 m); range noise N(0, noise) from default_rng(seed).
    Returns the points in the sensor frame, float32 (N,3)."""
    Tws = np.asarray(T_world_sensor, dtype=np.float64)
    d_s = _ring_directions(n_rings, n_az)
    d = d_s @ Tws[:3, :3].T
    t_best, _ = _cast(Tws[:3, 3], d, _walls(layout_seed))
    keep = np.isfinite(t_best) & (t_best >= 3.0) & (t_best <= 80.0)
    rng = np.random.default_rng(seed)
    r = t_best[keep] + rng.normal(0, noise, keep.sum())
    pts = d_s[keep] * r[:, None]
    return np.ascontiguousarray(pts, dtype=np.float32)


def kitti_like_sweep(frame, n_rings=64, n_az=2030, layout_seed=12345, noise=0.02, seed=777):
    """The scan of kitti_like_scan(frame) as a spinning sensor delivers it: RAW, every azimuth column cast from the pose the sensor has at
    its own firing time.  The sweep starts at the pose of frame - 1 and ends at the pose of `frame` (frame >= 1); with
    xi = se3_log(T(frame - 1)^-1 T(frame)), column c fires at s = float32((c + 0.5) / n_az) from T(frame - 1) exp(s xi).
    Returns (points in the sensor frame AT FIRING TIME float32 (N,3), times float32 (N,), T_world_sensor at the sweep's end, xi (6,),
    surface (N,): the surface each return hit, -1 = ground, else the wall number).  Deskewed with xi to ref_time = 1 — p' =
    exp((s - 1) xi) p — the points are what a rigid snapshot at T_world_sensor would have measured."""
    if int(frame) < 1:
        raise ValueError("kitti_like_sweep: a sweep ends at its frame and starts at the one before, so frame >= 1")
    return sweep_between(_sensor_pose(frame - 1), _sensor_pose(frame), n_rings, n_az, layout_seed, noise, seed + frame)


def sweep_between(T0, T1, n_rings=64, n_az=2030, layout_seed=12345, noise=0.02, seed=777):
    """kitti_like_sweep's casting between ANY two sensor poses: the sweep starts at T0 (T_world_sensor) and ends at T1, the sensor moving
    with the constant twist xi = se3_log(T0^-1 T1); column c fires at s = float32((c + 0.5) / n_az) from T0 exp(s xi).  Range noise
    N(0, noise) from default_rng(seed).  Returns what kitti_like_sweep returns: (points float32 (N,3), times float32 (N,), T1, xi (6,),
    surface (N,))."""
    from .api import se3_exp, se3_log

    T0, T1 = np.asarray(T0, dtype=np.float64), np.asarray(T1, dtype=np.float64)
    xi = se3_log(np.linalg.inv(T0) @ T1)
    s_col = ((np.arange(n_az) + 0.5) / n_az).astype(np.float32)
    T_col = np.stack([T0 @ se3_exp(float(s) * xi) for s in s_col])  # (n_az, 4, 4)
    d_s = _ring_directions(n_rings, n_az)
    col = np.tile(np.arange(n_az), n_rings)
    d = np.einsum("nij,nj->ni", T_col[col, :3, :3], d_s)
    t_best, surface = _cast(T_col[col, :3, 3], d, _walls(layout_seed))
    keep = np.isfinite(t_best) & (t_best >= 3.0) & (t_best <= 80.0)
    rng = np.random.default_rng(seed)
    r = t_best[keep] + rng.normal(0, noise, keep.sum())
    pts = d_s[keep] * r[:, None]
    return np.ascontiguousarray(pts, dtype=np.float32), np.ascontiguousarray(s_col[col][keep]), T1, xi, surface[keep]


def slalom_pose(frame):
    """T_world_sensor of a frame of the slalom: 1.8 m above ground from (-30, -20), the speed and the yaw rate changing from frame to
    frame.  Step f (from frame f to f + 1) advances by v_f = 1.0 + 0.5 sin(0.9 f) metres along the heading psi_f and then turns by
    w_f = 3 sin(1.3 f) degrees:  pos_{f+1} = pos_f + v_f (cos psi_f, sin psi_f, 0),  psi_{f+1} = psi_f + w_f,  psi_0 = 0.  The relative
    motion of consecutive sweeps differs by up to 0.5 m and 3.8 degrees, so the previous motion is a poor twist for the next sweep."""
    pos = np.array([-30.0, -20.0, 1.8])
    psi = 0.0
    for f in range(int(frame)):
        pos = pos + (1.0 + 0.5 * np.sin(0.9 * f)) * np.array([np.cos(psi), np.sin(psi), 0.0])
        psi = psi + np.deg2rad(3.0 * np.sin(1.3 * f))
    Tws = np.eye(4)
    Tws[:3, :3] = _rot([0, 0, 1], psi)
    Tws[:3, 3] = pos
    return Tws


def with_isolated_returns(points, share=0.01, seed=4242, min_range=5.0, max_range=60.0):
    """The scan with isolated returns scattered into it — rain, dust, multipath: round(share * N) of its points (chosen from `seed`) are
    replaced by returns along their own rays at a range uniform in [min_range, max_range] m, i.e. somewhere in the free space in front
    of (or behind) the surface the ray hit.  The number and the order of the points are kept, so times and rings still line up.
    Returns (points float32 (N,3), indices of the replaced points, ascending)."""
    pts = np.array(points, dtype=np.float32)[:, :3].copy()
    n = len(pts)
    m = int(round(share * n))
    rng = np.random.default_rng(seed)
    idx = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    d = pts[idx].astype(np.float64)
    d /= np.maximum(np.linalg.norm(d, axis=1), 1e-9)[:, None]
    pts[idx] = (d * rng.uniform(min_range, max_range, m)[:, None]).astype(np.float32)
    return np.ascontiguousarray(pts), idx


def mover_centre(frame):
    """The world position of the moving sphere of run_synthetic_submap(mover=True) at a frame: it crosses the road 12 m ahead of the first
    sensor pose, 1 m above ground, at 1.5 m/frame."""
    return _sensor_pose(0)[:3, 3] + np.array([12.0, -6.0 + 1.5 * frame, -0.8])


def with_moving_sphere(points, T_world_sensor, centre_world, radius=1.0):
    """The scan with a sphere standing in the scene — a moving object caught at one instant: every ray of the scan (sensor frame, from the
    sensor's origin) that meets the sphere of `radius` around centre_world nearer than its own return is shortened to the sphere.  The
    number and the order of the points are kept.  Returns (points float32 (N,3), mask (N,) bool of the changed returns)."""
    pts = np.array(points, dtype=np.float32)[:, :3].copy()
    T = np.asarray(T_world_sensor, dtype=np.float64)
    c = T[:3, :3].T @ (np.asarray(centre_world, dtype=np.float64) - T[:3, 3])  # the centre in the sensor frame
    p = pts.astype(np.float64)
    r = np.linalg.norm(p, axis=1)
    d = p / np.maximum(r, 1e-9)[:, None]
    b = d @ c
    disc = b * b - (c @ c - float(radius) ** 2)
    with np.errstate(invalid="ignore"):
        t = b - np.sqrt(disc)
    hit = (disc >= 0) & (t > 0) & (t < r)
    pts[hit] = (d[hit] * t[hit, None]).astype(np.float32)
    return np.ascontiguousarray(pts), hit

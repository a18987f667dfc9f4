"""Scan-to-scan GICP odometry (config C5), the protocol of the reference's benchmark
(src/benchmark/odometry_benchmark_small_gicp_omp.cpp:16-49 + include/small_gicp/benchmark/benchmark_odom.hpp:49-82):

  per frame:  voxelgrid_sampling(0.25 m)                      -> "total" time only (benchmark_odom.hpp:60-66)
              index build + estimate_covariances(k = 20)       -> registration time
              Registration<GICPFactor>::align(prev, cur, prev_tree, Identity); T_world = T_world * T     -> registration time
              the current scan (with its index and covariances) becomes the next target: each scan is preprocessed once.

Everything runs on the GPU through the C-ABI; only the raw scan crosses PCIe.
"""
import os
import time

import numpy as np

from . import api


class OnlineOdometry:
    """shard = (rank, world): multi-GPU form (BASELINE config C5).  Every rank preprocesses the whole scan (voxel grid, index,
    covariances: replicated), registers only its contiguous shard of the source against the replicated target
    and the context's RCCL communicator (Context.comm_init) sums the shards' systems once per linearization / error pass, so every rank
    computes the same pose."""

    def __init__(self, downsampling_resolution=0.25, num_neighbors=20, max_correspondence_distance=1.0, ctx=None, shard=None, min_range=None, max_range=None, outlier_k=None, outlier_std_mul=1.0,
                 estimate_twist=False, twist_prior_information=None, sweep_points=12000, sweep_source="sample"):
        self.shard = shard
        # estimate_twist (False: off, the default — a sweep is deskewed with the previous motion): a RAW sweep is registered against the
        # previous deskewed scan by api.align_sweep, which estimates its pose and its twist together — from the
        # previous motion as the initial twist AND the initial pose, or from zero and the identity when there is none — and the sweep is then
        # deskewed with the ESTIMATED twist, downsampled, and registered rigidly once more from the sweep's pose (the sample's pose refined).
        # What is registered is, with sweep_source="sample" (the default), an even sample of at most sweep_points of the (cropped) raw
        # points, taken with PointCloud.selected so that the times follow; with sweep_source="voxelgrid", the voxel grid of the raw sweep
        # at downsampling_resolution — the cloud every other registration here uses — whose times api.voxelgrid_sampling_fields carries
        # along, reduced by "nearest": the time of the return nearest the centroid, one real return's, which stays meaningful across the
        # sweep's seam where a mean of 0.02 and 0.98 would not.  twist_prior_information (None: no prior; a
        # number w: w I; or (6,6)): the information of a Gaussian prior on the twist centred on the previous motion, once there is one.
        if sweep_source not in ("sample", "voxelgrid"):
            raise ValueError("sweep_source must be 'sample' or 'voxelgrid'")
        self.sweep_source = sweep_source
        self.estimate_twist = bool(estimate_twist)
        self.sweep_points = int(sweep_points)
        if twist_prior_information is None:
            self.twist_information = None
        else:
            w = np.asarray(twist_prior_information, dtype=np.float64)
            self.twist_information = w * np.eye(6) if w.ndim == 0 else w.reshape(6, 6)
        self.twists = []  # estimate_twist: the twist of every registered sweep
        # outlier_k (None: off, the default): every downsampled scan loses its isolated returns on the device (PointCloud.without_outliers:
        # the mean distance to outlier_k neighbours above mean + outlier_std_mul * stddev) after the voxel grid and before the kd-tree and
        # the covariances.  None: no such call is made.
        self.outlier = None if outlier_k is None else (int(outlier_k), float(outlier_std_mul))
        # min_range / max_range (metres from the sensor; None: no bound): when either is given, every scan is cropped on the device ahead of
        # the deskew (PointCloud.cropped), non-finite returns included, and a sweep's times follow the points kept.  Both None: no crop call.
        self.crop = None if min_range is None and max_range is None else (0.0 if min_range is None else float(min_range), np.inf if max_range is None else float(max_range))
        self.res = downsampling_resolution
        self.k = num_neighbors
        self.setting = api.make_setting("GICP", max_correspondence_distance=max_correspondence_distance)
        self.max_dist = max_correspondence_distance
        # every step of a scan runs on ONE context in stream-ordered mode: no host wait between the index build, the covariances and the
        # registration.  The mode changes what "returned" means for every user of that context, so the estimator takes a context of its own
        # unless it is handed one (the sharded bench leg: the context that carries the communicator), whose mode it restores in close().
        self._own_ctx = ctx is None
        self.ctx = ctx or api.Context(0)
        self._prev_mode = self.ctx.set_stream_ordered(True)
        self.target = None  # (cloud, tree)
        self.T_world = np.eye(4)
        self.motion = None  # the last registration's relative pose: the constant-velocity guess a raw sweep is deskewed with
        self.reg_ms = []
        self.total_ms = []
        self.iterations = []

    def close(self):
        """Give a borrowed context its previous mode back (synchronises it)."""
        if self.ctx is not None and not self._own_ctx:
            self.ctx.set_stream_ordered(self._prev_mode)
        self.target = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def estimate(self, points, times=None):
        """points: (N,3|4) float32 in the sensor frame. Returns T_world_sensor of this scan.
        times: None — the scan is a rigid snapshot — or the time of every point within its sweep, 0 = start .. 1 = end (numpy (N,), or a
        torch tensor on the context's device): the points are a RAW sweep, each in the sensor frame of its own instant, and are deskewed on
        the device ahead of the voxel grid (PointCloud.deskewed) to the sweep's end under constant velocity — the twist is se3_log of the
        previous frame's relative motion.  The first frame, which has no motion before it, is taken as it is; so is the second when it is
        registered (two sweeps skewed alike still give their relative motion), but it becomes the third frame's target deskewed by the
        motion it has just yielded: a deskewed scan is never registered against a skewed one."""
        t0 = time.perf_counter()
        raw = api.PointCloud(points, ctx=self.ctx)
        if self.crop is not None:
            raw, times = self._cropped(raw, times)
        if self.estimate_twist and times is not None and self.target is not None:
            return self._estimate_sweep(raw, times, t0)
        bootstrap =times is not None and self.motion is None and self.target is not None  # the first registration of a sequence of sweeps
        if times is not None and self.motion is not None:
            raw = raw.deskewed(times, api.se3_log(self.motion), 1.0)
        cloud = self._downsampled(raw)
        self.ctx.synchronize()
        t1 = time.perf_counter()
        tree = api.KdTree(cloud)
        api.estimate_covariances(cloud, tree, self.k)
        if self.target is not None:
            tgt_cloud, tgt_tree = self.target
            src = tree  # the scan by its own index: its kd order is spatially coherent, the problem takes it as it is (no sort)
            if self.shard is not None:
                rank, world = self.shard
                n = cloud.size()
                lo, hi = rank * n // world, (rank + 1) * n // world
                src = cloud.slice(lo, hi - lo)
            res = api.Problem(tgt_tree, src, np.eye(4)).align(self.setting, np.eye(4))
            self.T_world = self.T_world @ res.T_target_source
            self.motion = res.T_target_source
            self.iterations.append(res.iterations + 1)
            if bootstrap:  # once per sequence: this scan again, deskewed, as the next frame's target
                cloud = self._downsampled(raw.deskewed(times, api.se3_log(self.motion), 1.0))
                tree = api.KdTree(cloud)
                api.estimate_covariances(cloud, tree, self.k)
        self.ctx.synchronize()
        t2 = time.perf_counter()
        self.target = (cloud, tree)
        self.reg_ms.append(1e3 * (t2 - t1))
        self.total_ms.append(1e3 * (t2 - t0))
        return self.T_world.copy()

    def _estimate_sweep(self, raw, times, t0):
        """estimate_twist: the raw sweep's pose and twist from api.align_sweep over an even sample of it (sweep_source="sample") or over its
        voxel grid with the times carried along ("voxelgrid"), then the sweep deskewed with that twist as the next target.  (The times
        are a host array here: a sample's times are gathered on the host, the grid's M reduced times come to the host once, for
        align_sweep's host `times`.)"""
        if self.shard is not None:
            raise ValueError("estimate_twist is not available on a sharded estimator")
        times = np.ascontiguousarray(np.asarray(times, dtype=np.float32).reshape(-1))
        n = raw.size()
        if self.sweep_source == "voxelgrid":
            sample, reduced = api.voxelgrid_sampling_fields(raw, times, self.res, reduce="nearest")
            sample_times = np.ascontiguousarray(reduced.numpy().reshape(-1))
        else:
            idx = np.arange(0, n, max(1, -(-n // max(1, self.sweep_points))), dtype=np.int64)
            sample = raw if len(idx) == n else raw.selected(idx)
            sample_times = times[idx]
        self.ctx.synchronize()
        t1 = time.perf_counter()
        api.estimate_covariances(sample, None, self.k)
        tgt_cloud, tgt_tree = self.target
        centre = None if self.motion is None else api.se3_log(self.motion)
        prior = self.twist_information if centre is not None else None
        # under a constant twist the pose at the sweep's end, seen from its start, is exp(twist): the previous motion is the guess for both
        # (from the identity a step of more than the correspondence distance is outside the loop's reach: 1.4 m errors on the slalom)
        init_T = self.motion if self.motion is not None else np.eye(4)
        res = api.align_sweep(tgt_cloud, sample, sample_times, tgt_tree, init_T=init_T, init_twist=centre, ref_time=1.0, twist_prior=centre if prior is not None else None, twist_information=prior, setting=self.setting)
        pose = res.T_target_source
        self.twists.append(res.twist)
        self.iterations.append(res.iterations + 1)
        cloud = self._downsampled(raw.deskewed(times, res.twist, 1.0))
        tree = api.KdTree(cloud)
        api.estimate_covariances(cloud, tree, self.k)
        # the deskewed scan, at the voxel grid's full density, registered rigidly from the sweep's pose: the sample's pose refined
        pose = api.Problem(tgt_tree, tree, pose).align(self.setting, pose).T_target_source
        self.T_world = self.T_world @ pose
        self.motion = pose
        self.ctx.synchronize()
        t2 = time.perf_counter()
        self.target = (cloud, tree)
        self.reg_ms.append(1e3 * (t2 - t1))
        self.total_ms.append(1e3 * (t2 - t0))
        return self.T_world.copy()

    def _downsampled(self, raw):
        """The voxel grid of the raw cloud and, when outlier_k is given, that cloud without its isolated returns (a temporary tree: the
        scan's own tree is built over what is left)."""
        cloud = api.voxelgrid_sampling(raw, self.res)
        if self.outlier is not None:
            cloud = cloud.without_outliers(self.outlier[0], self.outlier[1])
        return cloud

    def _cropped(self, raw, times):
        """The raw cloud within the estimator's ranges, and the times of the points kept (numpy times: numpy indices; a torch tensor on
        the device: the indices stay there)."""
        lo, hi = self.crop
        if times is None:
            return raw.cropped(lo, hi), None
        if isinstance(times, np.ndarray) or not type(times).__module__.startswith("torch"):
            raw, kept = raw.cropped(lo, hi, return_kept=True)
            return raw, np.asarray(times).reshape(-1)[kept]
        import torch

        raw, kept = raw.cropped(lo, hi, return_kept=True, stream=torch.cuda.current_stream(int(self.ctx.device)))
        return raw, times.reshape(-1)[kept]


class ModelOdometry:
    """Scan-to-MODEL VGICP odometry (src/benchmark/odometry_benchmark_small_vgicp_model_omp.cpp:12-57): the target is one
    GaussianVoxelMap accumulating every registered scan (incremental insert with the estimated pose + LRU removal of voxels the
    sensor has left behind); each new scan is registered against it starting from the previous pose, then inserted."""

    def __init__(self, downsampling_resolution=0.25, num_neighbors=20, voxel_resolution=1.0, max_correspondence_distance=1.0, ctx=None, model="gaussian", factor="GICP"):
        """model = "gaussian": GaussianVoxelMap / VGICP (odometry_benchmark_small_vgicp_model_omp.cpp); "flat": IncrementalVoxelMap<
        FlatContainerCov> / GICP against the stored points (odometry_benchmark_small_gicp_model_omp.cpp).  factor = "PLANE_ICP" (flat
        model only): IncrementalVoxelMap<FlatContainerNormal> / point-to-plane ICP against the stored points and their normals (the
        linear iVox of Faster-LIO, flat_container.hpp:15-17); the scans get normals instead of covariances."""
        if factor not in ("GICP", "PLANE_ICP"):
            raise ValueError("factor must be 'GICP' or 'PLANE_ICP'")
        if factor == "PLANE_ICP" and model != "flat":
            raise ValueError("PLANE_ICP needs the flat model: a GaussianVoxelMap keeps no normals")
        self.model = model
        self.factor = factor
        self.res = downsampling_resolution
        self.k = num_neighbors
        self.voxel_resolution = voxel_resolution
        self.setting = api.make_setting(factor, max_correspondence_distance=max_correspondence_distance)
        self.ctx = ctx or api.default_context()
        self.voxelmap = None
        self.T_world = np.eye(4)
        self.reg_ms, self.total_ms, self.iterations = [], [], []

    def estimate(self, points):
        t0 = time.perf_counter()
        raw = api.PointCloud(points, ctx=self.ctx)
        cloud = api.voxelgrid_sampling(raw, self.res)
        self.ctx.synchronize()
        t1 = time.perf_counter()
        if self.factor == "PLANE_ICP":
            api.estimate_normals(cloud, None, self.k)
        else:
            api.estimate_covariances(cloud, None, self.k)
        if self.voxelmap is None:  # the very first frame
            if self.factor == "PLANE_ICP":
                kind = api.IncrementalVoxelMapNormal
            else:
                kind = api.IncrementalVoxelMapCov if self.model == "flat" else api.GaussianVoxelMap
            self.voxelmap = kind(self.voxel_resolution, ctx=self.ctx)
            self.voxelmap.insert(cloud)
        else:
            res = api.Problem(self.voxelmap, cloud, self.T_world).align(self.setting, self.T_world)
            self.T_world = res.T_target_source
            self.iterations.append(res.iterations + 1)
            self.voxelmap.insert(cloud, self.T_world)
            self.ctx.synchronize()
            self.reg_ms.append(1e3 * (time.perf_counter() - t1))
        self.ctx.synchronize()
        self.total_ms.append(1e3 * (time.perf_counter() - t0))
        return self.T_world.copy()


def run_synthetic_model(num_frames=20, **kw):
    """ModelOdometry over the frozen synthetic sequence (keyword arguments, model= and factor= among them, go to ModelOdometry);
    absolute trajectory error against the generator's ground truth."""
    from . import synthetic

    odom = ModelOdometry(**kw)
    est, gt = [], []
    T0 = None
    for f in range(num_frames):
        pts, Tws = synthetic.kitti_like_scan(f)
        if T0 is None:
            T0 = Tws
        est.append(odom.estimate(pts))
        gt.append(np.linalg.inv(T0) @ Tws)
    ate = [float(np.linalg.norm(e[:3, 3] - g[:3, 3])) for e, g in zip(est, gt)]
    skip = 2 if num_frames > 4 else 0
    return {
        "frames": num_frames,
        "registration_ms_per_scan": float(np.mean(odom.reg_ms[skip:])) if len(odom.reg_ms) > skip else float("nan"),
        "total_ms_per_scan": float(np.mean(odom.total_ms[skip + 1 :])) if len(odom.total_ms) > skip + 1 else float("nan"),
        "total_ms_per_scan_median": float(np.median(odom.total_ms[skip + 1 :])) if len(odom.total_ms) > skip + 1 else float("nan"),
        "mean_iterations": float(np.mean(odom.iterations)) if odom.iterations else 0.0,
        "ate_trans_m_max": max(ate),
        "num_voxels": odom.voxelmap.size(),
        "estimated": est,
        "ground_truth": gt,
    }


class SubmapOdometry:
    """Scan-to-SUBMAP GICP odometry against an exact kd-tree: the target of a scan is ONE cloud made of the last `window` preprocessed
    scans at their estimated world poses (api.merge_clouds: one launch, the covariances ride along rotated, nothing is estimated twice)
    and the KdTree over it; the scan is registered from the previous pose, as ModelOdometry does.  Per scan the preprocessing is
    OnlineOdometry's.  The driver names the submap's device-frame origin itself — the library's rule applied to the previous position —
    so the stream-ordered context never waits for a bounding box.
    keyframe_overlap (None: off, the default — every scan joins the window): a registered scan joins the window only when the share of
    its points that the submap already explains (PointCloud.overlap against the submap's tree at the new pose: the fitness within
    overlap_distance, default the downsampling resolution) is BELOW keyframe_overlap; the first scan always joins.  fitness: the figure
    of every registered scan; keyframes_added: the scans that joined.
    remove_seen_through (False: off, the default): once a scan is registered, every keyframe (cloud_k, T_k) of the window is replaced by
    the points the RAW scan does not see through (PointCloud.visibility with keep="rest" and T = T_k^-1 T_world: the free-space check
    that takes the trails of moving objects out of the submap); visibility: a dict of that call's keyword arguments (None: the
    library's defaults).  removed_points: the points taken out, per registered scan."""

    def __init__(self, window=5, downsampling_resolution=0.25, num_neighbors=20, max_correspondence_distance=1.0, ctx=None, record=False, keyframe_overlap=None, overlap_distance=None,
                 remove_seen_through=False, visibility=None):
        if window < 1:
            raise ValueError("window must be at least 1")
        self.remove_seen_through = bool(remove_seen_through)
        self.visibility = dict(visibility or {})
        self.removed_points = []
        self.keyframe_overlap = None if keyframe_overlap is None else float(keyframe_overlap)
        self.overlap_distance = float(downsampling_resolution if overlap_distance is None else overlap_distance)
        self.fitness, self.keyframes_added = [], 0
        self.window = window
        self.res = downsampling_resolution
        self.k = num_neighbors
        self.setting = api.make_setting("GICP", max_correspondence_distance=max_correspondence_distance)
        self._own_ctx = ctx is None
        self.ctx = ctx or api.Context(0)
        self._prev_mode = self.ctx.set_stream_ordered(True)
        self.keyframes = []  # (cloud, T_world) of the last `window` scans
        self.T_world = np.eye(4)
        self.reg_ms, self.total_ms, self.iterations = [], [], []
        self.record = record
        self.records = []  # record=True: (submap cloud, scan cloud, initial pose, result pose, iterations) per registered scan

    def close(self):
        """Give a borrowed context its previous mode back (synchronises it)."""
        if self.ctx is not None and not self._own_ctx:
            self.ctx.set_stream_ordered(self._prev_mode)
        self.keyframes = []

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _submap_origin(self):
        p = np.ascontiguousarray(self.T_world[:3, 3], dtype=np.float64)
        o = np.zeros(3)
        api.load().sga_choose_origin(api._dp(p), api._dp(p), api._dp(o))
        return o

    def _remove_seen_through(self, raw):
        """every keyframe of the window without the points that the raw scan, at the pose just found, sees through -> the points removed"""
        removed = 0
        for k, (cloud_k, T_k) in enumerate(self.keyframes):
            _, rest = cloud_k.visibility(raw, np.linalg.inv(T_k) @ self.T_world, keep="rest", params=self.visibility, ctx=self.ctx)
            if 0 < rest.size() < cloud_k.size():  # (a keyframe the scan would see through entirely is left alone: the pose is in doubt, not the map)
                removed += cloud_k.size() - rest.size()
                self.keyframes[k] = (rest, T_k)
        return removed

    def estimate(self, points):
        """points: (N,3|4) float32 in the sensor frame. Returns T_world_sensor of this scan."""
        t0 = time.perf_counter()
        raw = api.PointCloud(points, ctx=self.ctx)
        cloud = api.voxelgrid_sampling(raw, self.res)
        self.ctx.synchronize()
        t1 = time.perf_counter()
        tree = api.KdTree(cloud)
        api.estimate_covariances(cloud, tree, self.k)
        joins = True
        if self.keyframes:
            submap = api.merge_clouds([c for c, _ in self.keyframes], [T for _, T in self.keyframes], origin=self._submap_origin(), ctx=self.ctx)
            target = api.KdTree(submap)
            init = self.T_world.copy()
            res = api.Problem(target, tree, init).align(self.setting, init)
            self.T_world = res.T_target_source
            self.iterations.append(res.iterations + 1)
            if self.record:
                self.records.append((submap, cloud, init, self.T_world.copy(), res.iterations + 1))
            if self.keyframe_overlap is not None:
                self.fitness.append(cloud.overlap(target, self.T_world, self.overlap_distance, ctx=self.ctx)["fitness"])
                joins = self.fitness[-1] < self.keyframe_overlap
            if self.remove_seen_through:
                self.removed_points.append(self._remove_seen_through(raw))
        self.ctx.synchronize()
        t2 = time.perf_counter()
        if joins:
            self.keyframes = (self.keyframes + [(cloud, self.T_world.copy())])[-self.window :]
            self.keyframes_added += 1
        self.reg_ms.append(1e3 * (t2 - t1))
        self.total_ms.append(1e3 * (t2 - t0))
        return self.T_world.copy()


def run_synthetic_submap(num_frames=20, window=5, mover=False, **kw):
    """SubmapOdometry over the frozen synthetic sequence (keyword arguments go to SubmapOdometry); absolute trajectory error against the
    generator's ground truth.  The return value has run_synthetic_model's shape (num_points: the last submap's size, in place of num_voxels),
    with keyframes_added (the scans that joined the window) and fitness (the overlap figure of every registered scan; empty unless
    keyframe_overlap is given).  mover: every scan goes through synthetic.with_moving_sphere at synthetic.mover_centre(frame).
    ghost_points (0 without a mover): the points of the final window, at their estimated poses, within 1.1 radii of the mover's centre at
    an EARLIER frame and farther than that from its centre at the last one — the trail it left in the submap.  removed_points: what
    remove_seen_through took out, per registered scan (empty when it is off); entered_points: the points that joined the window."""
    from . import synthetic

    odom = SubmapOdometry(window=window, **kw)
    est, gt = [], []
    T0 = None
    entered, added = 0, 0
    for f in range(num_frames):
        pts, Tws = synthetic.kitti_like_scan(f)
        if mover:
            pts, _ = synthetic.with_moving_sphere(pts, Tws, synthetic.mover_centre(f))
        if T0 is None:
            T0 = Tws
        est.append(odom.estimate(pts))
        gt.append(np.linalg.inv(T0) @ Tws)
        if odom.keyframes_added > added:  # the scan joined the window (it is checked against later scans only)
            added = odom.keyframes_added
            entered += odom.keyframes[-1][0].size()
    ate = [float(np.linalg.norm(e[:3, 3] - g[:3, 3])) for e, g in zip(est, gt)]
    ghosts = 0
    if mover:
        radius, Ti = 1.1 * 1.0, np.linalg.inv(T0)
        centres = [Ti[:3, :3] @ synthetic.mover_centre(f) + Ti[:3, 3] for f in range(num_frames)]  # in the frame of the first scan, as the estimates are
        for c, T in odom.keyframes:
            p = c.xyz().astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            trail = np.zeros(len(p), bool)
            for centre in centres[:-1]:
                trail |= np.linalg.norm(p - centre, axis=1) <= radius
            ghosts += int((trail & (np.linalg.norm(p - centres[-1], axis=1) > radius)).sum())
    skip = 2 if num_frames > 4 else 1  # (as run_synthetic: the first frames carry first-touch allocations)
    out = {
        "frames": num_frames,
        "window": window,
        "registration_ms_per_scan": float(np.mean(odom.reg_ms[skip:])) if len(odom.reg_ms) > skip else float("nan"),
        "total_ms_per_scan": float(np.mean(odom.total_ms[skip:])) if len(odom.total_ms) > skip else float("nan"),
        "total_ms_per_scan_median": float(np.median(odom.total_ms[skip:])) if len(odom.total_ms) > skip else float("nan"),
        "mean_iterations": float(np.mean(odom.iterations)) if odom.iterations else 0.0,
        "ate_trans_m_max": max(ate),
        "num_points": sum(c.size() for c, _ in odom.keyframes),
        "keyframes_added": odom.keyframes_added,
        "fitness": list(odom.fitness),
        "ghost_points": ghosts,
        "removed_points": list(odom.removed_points),
        "entered_points": entered,
        "estimated": est,
        "ground_truth": gt,
    }
    if odom.record:
        out["records"] = odom.records
    odom.close()
    return out


class PipelinedOdometry:
    """The same scan-to-scan odometry as a flow of stages over HIP streams (one context each) — the HIP-stream analogue of the reference's
    TBB flow graph (src/benchmark/odometry_benchmark_small_gicp_tbb_flow.cpp:55-141):

      preprocess_node   (`workers` threads, frames i, i + workers, ...: upload, voxel grid, index build, covariances; :61-67)
      pairing_node      (frame i-1 is the target of frame i; :73-78)
      registration_node (`reg_workers` threads: pair i is registered from the identity whatever pair i-1 gave, so the pairs are independent
                         and the reference runs this node with unlimited concurrency too; :81-97)
      output_node       (the relative poses multiplied up in frame order; :103-110)

    A frame is a chain of ~30 dependent launches that leaves the GPU mostly idle, so several chains interleave almost for free.  Poses
    are identical to OnlineOdometry's (same kernels, same order of operations per frame and per pair; the products in frame order)."""

    def __init__(self, downsampling_resolution=0.25, num_neighbors=20, max_correspondence_distance=1.0, device=0, workers=2, depth=None, reg_workers=2):
        # defaults: 2 x 2 workers — the measured optimum on one MI355X (profiles/r06_flow_cpp_grid.txt); more streams make every kernel slower
        self.res = downsampling_resolution
        self.k = num_neighbors
        self.setting = api.make_setting("GICP", max_correspondence_distance=max_correspondence_distance)
        self.ctx_pre = [api.Context(device) for _ in range(max(1, workers))]
        for c in self.ctx_pre:  # a frame's chain is enqueued without host waits; whoever consumes its cloud / index waits for their events (common.hpp: Ready)
            c.set_stream_ordered(True)
        self.ctx_reg = [api.Context(device) for _ in range(max(1, reg_workers))]
        self.depth = max(depth or 6, len(self.ctx_pre) + len(self.ctx_reg) + 1)

    def _preprocess(self, points, ctx):
        raw = api.PointCloud(points, ctx=ctx)
        cloud = api.voxelgrid_sampling(raw, self.res)
        tree = api.KdTree(cloud)
        api.estimate_covariances(cloud, tree, self.k)
        return cloud, tree

    def run(self, scans):
        """scans: sequence of (N,3|4) float32 arrays.  Returns (poses T_world_sensor, wall seconds, iterations per registration)."""
        import threading

        scans = list(scans)
        n = len(scans)
        P, R = len(self.ctx_pre), len(self.ctx_reg)
        ready = {}  # frame -> (cloud, tree), until both of its pairs are registered
        rel = {}    # frame -> (T_(frame-1) frame, iterations)
        cv = threading.Condition()
        state = {"next_pair": 1, "error": None}  # every pair below next_pair is registered (the producers run at most `depth` frames ahead of it)

        def fail(ex):
            with cv:
                if state["error"] is None:
                    state["error"] = ex
                cv.notify_all()

        def producer(w):
            try:
                for i in range(w, n, P):
                    with cv:
                        cv.wait_for(lambda: i < state["next_pair"] + self.depth or state["error"] is not None)
                        if state["error"] is not None:
                            return
                    item = self._preprocess(scans[i], self.ctx_pre[w])
                    with cv:
                        ready[i] = item
                        cv.notify_all()
            except BaseException as ex:  # noqa: BLE001
                fail(ex)

        def registrar(r):
            try:
                ctx = self.ctx_reg[r]
                for i in range(1 + r, n, R):
                    with cv:
                        cv.wait_for(lambda: (i in ready and i - 1 in ready) or state["error"] is not None)
                        if state["error"] is not None:
                            return
                        tgt, src = ready[i - 1], ready[i]
                    # the registration runs on its own context / stream, which waits for the events behind the producers' work
                    res = api.Problem(tgt[1], src[1], np.eye(4), ctx=ctx).align(self.setting, np.eye(4))
                    del tgt, src
                    with cv:
                        rel[i] = (res.T_target_source, res.iterations + 1)
                        while state["next_pair"] in rel:  # pairs up to here are done: their frames below the last one have served as source and target
                            ready.pop(state["next_pair"] - 1, None)
                            state["next_pair"] += 1
                        if state["next_pair"] == n:
                            ready.pop(n - 1, None)
                        cv.notify_all()
            except BaseException as ex:  # noqa: BLE001
                fail(ex)

        # The threads spend their time inside ctypes calls (GIL released) and need the GIL for microseconds in between; with CPython's default
        # switch interval (5 ms) a thread coming back from a call can wait that long for one that is running bytecode.  SGA_PIPE_SWITCH_S
        # (default 2e-5 s) for the duration of the run.
        import os
        import sys

        old_switch = sys.getswitchinterval()
        sys.setswitchinterval(float(os.environ.get("SGA_PIPE_SWITCH_S", "2e-5")))
        t0 = time.perf_counter()
        threads = [threading.Thread(target=producer, args=(w,), daemon=True) for w in range(P)]
        threads += [threading.Thread(target=registrar, args=(r,), daemon=True) for r in range(R)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        sys.setswitchinterval(old_switch)
        if state["error"] is not None:
            raise state["error"]
        for c in self.ctx_reg:
            c.synchronize()
        # output node: the relative poses multiplied up in frame order (the same products as OnlineOdometry's)
        poses, iters = [], []
        T_world = np.eye(4)
        for i in range(n):
            if i > 0:
                T_world = T_world @ rel[i][0]
                iters.append(rel[i][1])
            poses.append(T_world.copy())
        wall = time.perf_counter() - t0
        return poses, wall, iters


def run_synthetic(num_frames=20, pinned=False, sweeps=False, times=True, min_range=None, max_range=None, outliers=False, outlier_share=0.01, trajectory="arc", n_rings=64, n_az=2030, **kw):
    """Drive OnlineOdometry over the frozen KITTI-shaped synthetic sequence (small_gicp_amd.synthetic.kitti_like_scan).
    pinned: the scans are held in pinned host memory (api.pinned_copy) before the timed loop, like a driver that reads its scans into
    memory from sga_host_alloc — the reference's benchmark holds them in host memory too (benchmark/benchmark_odom.hpp:36-47); the upload
    then has no CPU pass.
    sweeps: the scans are RAW sweeps of a spinning sensor (synthetic.kitti_like_sweep of frames 1 .. num_frames: every column measured
    from the pose of its own instant) and are handed to the estimator with their times, which deskews them on the device; times=False
    withholds the times, so the skewed sweeps are registered as if they were snapshots (what the deskew is compared against).
    min_range / max_range: the estimator crops every scan to these ranges on the device first (OnlineOdometry); both None: no crop.
    outliers: outlier_share of every scan's returns (1 % by default) are replaced by isolated returns along their own rays
    (synthetic.with_isolated_returns, seeded by the frame); outlier_k= / outlier_std_mul= (OnlineOdometry) remove them on the device.
    trajectory: "arc" (the default: synthetic._sensor_pose, constant speed and yaw rate) or "slalom" (synthetic.slalom_pose: both change
    from frame to frame; sweep f is synthetic.sweep_between(slalom_pose(f), slalom_pose(f + 1)), a snapshot synthetic.scan_at(slalom_pose(f))).
    n_rings / n_az: the sensor's rays.  estimate_twist= / twist_prior_information= (OnlineOdometry): sweeps are registered with their
    twist free (api.align_sweep) instead of being deskewed with the previous motion; "twists" then holds the estimates.  sweep_source=
    (OnlineOdometry: "sample", the default, or "voxelgrid") chooses what of the raw sweep is registered."""
    from . import synthetic

    if trajectory not in ("arc", "slalom"):
        raise ValueError("trajectory must be 'arc' or 'slalom'")
    odom = OnlineOdometry(min_range=min_range, max_range=max_range, **kw)
    est, gt, sizes = [], [], []
    # every scan is in host memory before the loop starts, as in the reference's driver (benchmark/benchmark_odom.hpp:36-47; the generator
    # is ~50 ms of host work per scan: run between the frames it would leave the GPU idle and clocked down)
    scans, stamps, T0 = [], [], None
    for f in range(num_frames):
        if sweeps:
            if trajectory == "slalom":
                pts, ts, Tws = synthetic.sweep_between(synthetic.slalom_pose(f), synthetic.slalom_pose(f + 1), n_rings=n_rings, n_az=n_az, seed=777 + f + 1)[:3]
            else:
                pts, ts, Tws = synthetic.kitti_like_sweep(f + 1, n_rings=n_rings, n_az=n_az)[:3]
            stamps.append(ts if times else None)
        elif trajectory == "slalom":
            Tws = synthetic.slalom_pose(f)
            pts = synthetic.scan_at(Tws, n_rings=n_rings, n_az=n_az, seed=777 + f)
        else:
            pts, Tws = synthetic.kitti_like_scan(f, n_rings=n_rings, n_az=n_az)
        if outliers:
            pts = synthetic.with_isolated_returns(pts, outlier_share, seed=4242 + f)[0]
        scans.append(api.pinned_copy(pts[:, :3], np.float32) if pinned else np.ascontiguousarray(pts[:, :3], dtype=np.float32))
        if T0 is None:
            T0 = Tws
        sizes.append(len(pts))
        gt.append(np.linalg.inv(T0) @ Tws)
    for f, pts in enumerate(scans):
        est.append(odom.estimate(pts, stamps[f]) if sweeps else odom.estimate(pts))
    # relative pose error per frame pair (what scan-to-scan registration controls)
    rpe_t, rpe_r = [], []
    for i in range(1, num_frames):
        de = np.linalg.inv(est[i - 1]) @ est[i]
        dg = np.linalg.inv(gt[i - 1]) @ gt[i]
        E = np.linalg.inv(dg) @ de
        rpe_t.append(float(np.linalg.norm(E[:3, 3])))
        rpe_r.append(float(np.arccos(min(1.0, max(-1.0, (np.trace(E[:3, :3]) - 1) / 2)))))
    skip = 2 if num_frames > 4 else 1  # first frames carry first-touch allocations
    return {
        "frames": num_frames,
        "scans_in_pinned_host_memory": bool(pinned),
        "points_per_scan": float(np.mean(sizes)),
        "registration_ms_per_scan": float(np.mean(odom.reg_ms[skip:])) if len(odom.reg_ms) > skip else float("nan"),
        "total_ms_per_scan": float(np.mean(odom.total_ms[skip:])) if len(odom.total_ms) > skip else float("nan"),
        "mean_iterations": float(np.mean(odom.iterations)) if odom.iterations else 0.0,
        "rpe_trans_m_mean": float(np.mean(rpe_t)) if rpe_t else 0.0,
        "rpe_rot_rad_mean": float(np.mean(rpe_r)) if rpe_r else 0.0,
        "rpe_trans_m": rpe_t,
        "ate_trans_m_max": max(float(np.linalg.norm(e[:3, 3] - g[:3, 3])) for e, g in zip(est, gt)),
        "sweeps": bool(sweeps),
        "twists": list(odom.twists),
        "estimated": est,
        "ground_truth": gt,
    }


def run_synthetic_batched(num_frames=20, batch=8, downsampling_resolution=0.25, num_neighbors=20, max_correspondence_distance=1.0, ctx=None, batched_preprocessing=False, batched_downsampling=False,
                          registration_type="GICP", voxel_resolution=1.0, batched_voxelmaps=False, batched_problems=False):
    """The flow protocol (every pair (i - 1, i) registered from the identity, the relative poses multiplied up in frame order:
    odometry_benchmark_small_gicp_tbb_flow.cpp:73-110) with the registrations BATCHED: the scans are preprocessed as OnlineOdometry does,
    then groups of `batch` consecutive pairs are registered by one BatchProblem.align each — one search + factor launch, one row
    reduction and one hand-off per LM round for the whole group.  The last group may be smaller; batch = 1 works.  Returns the poses,
    the relative poses and iteration counts per pair, and the wall time of the registration stage per scan.
    batched_preprocessing: the kd-trees and covariances of every `batch` scans are made by one api.preprocess_batch (the same trees and
    covariances, bit for bit: the results do not change).
    batched_downsampling: the raw scans of every `batch` frames are uploaded and downsampled by one api.voxelgrid_sampling_batch (the
    same clouds, bit for bit); without it the scans are downsampled one by one.
    registration_type: "GICP" (every pair against the kd-tree of scan i - 1) or "VGICP" (against the Gaussian voxel map of scan i - 1 at
    voxel_resolution).  batched_voxelmaps: the maps of every `batch` scans are made by one api.build_gaussian_voxelmaps (the same maps,
    bit for bit: the results do not change); without it by GaussianVoxelMap.from_cloud one by one.
    batched_problems: the problems of a group of VGICP pairs are made by one api.create_problems (the same source orders, bit for bit: the
    results do not change); without it, and for GICP pairs (the scan by its own index: no sort to batch), by Problem one by one."""
    from . import synthetic

    if batch < 1:
        raise ValueError("batch must be at least 1")
    if registration_type not in ("GICP", "VGICP"):
        raise ValueError("registration_type must be GICP or VGICP")
    ctx = ctx or api.Context(0)
    prev_mode = ctx.set_stream_ordered(True)
    try:
        setting = api.make_setting(registration_type, max_correspondence_distance=max_correspondence_distance)
        frames = []  # (cloud, tree) per scan
        pending = []  # downsampled scans waiting for their batched trees and covariances
        raw = []  # uploaded scans waiting for their batched voxel grid
        for f in range(num_frames):
            pts, _ = synthetic.kitti_like_scan(f)
            scan = api.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32), ctx=ctx)
            if batched_downsampling:
                raw.append(scan)
                if len(raw) < batch and f < num_frames - 1:
                    continue
                clouds = api.voxelgrid_sampling_batch(raw, downsampling_resolution)
                raw = []
            else:
                clouds = [api.voxelgrid_sampling(scan, downsampling_resolution)]
            for cloud in clouds:
                if batched_preprocessing:
                    pending.append(cloud)
                    continue
                tree = api.KdTree(cloud)
                api.estimate_covariances(cloud, tree, num_neighbors)
                frames.append((cloud, tree))
            if pending and (len(pending) >= batch or f == num_frames - 1):
                frames.extend(api.preprocess_batch(pending, num_neighbors))
                pending = []
        targets = [tree for _, tree in frames]
        if registration_type == "VGICP":  # the target of pair (i - 1, i): the map of scan i - 1 (the last scan is nobody's target)
            targets = []
            for first in range(0, num_frames - 1, batch):
                clouds = [frames[i][0] for i in range(first, min(first + batch, num_frames - 1))]
                targets.extend(api.build_gaussian_voxelmaps(clouds, voxel_resolution) if batched_voxelmaps else [api.GaussianVoxelMap.from_cloud(c, voxel_resolution) for c in clouds])
        ctx.synchronize()
        rel, iters = [], []
        t0 = time.perf_counter()
        for first in range(1, num_frames, batch):
            group = range(first, min(first + batch, num_frames))
            src = 0 if registration_type == "VGICP" else 1  # kd-tree targets: the scan by its own index, as OnlineOdometry; map targets: the scan's cloud
            if batched_problems and src == 0:
                problems = api.create_problems([targets[i - 1] for i in group], [frames[i][0] for i in group], [np.eye(4)] * len(group), ctx=ctx)
            else:
                problems = [api.Problem(targets[i - 1], frames[i][src], np.eye(4), ctx=ctx) for i in group]
            bp = api.BatchProblem(problems)
            for r in bp.align(setting):
                rel.append(r.T_target_source)
                iters.append(r.iterations + 1)
            del bp  # before its problems
        ctx.synchronize()
        wall = time.perf_counter() - t0
    finally:
        ctx.set_stream_ordered(prev_mode)
    est = [np.eye(4)]
    for T in rel:
        est.append(est[-1] @ T)
    return {"frames": num_frames, "batch": batch, "registration_ms_per_scan": 1e3 * wall / max(1, num_frames - 1), "mean_iterations": float(np.mean(iters)) if iters else 0.0,
            "relative_poses": rel, "iterations": iters, "estimated": est}


def run_synthetic_model_batched(num_frames=20, streams=4, batched_insert=False, downsampling_resolution=0.25, num_neighbors=20, voxel_resolution=1.0, max_correspondence_distance=1.0, ctx=None,
                                batched_problems=False):
    """`streams` independent scan-to-model VGICP streams (ModelOdometry's protocol: register against the stream's own GaussianVoxelMap from
    the previous pose, then insert the scan at the estimated pose) over the frozen synthetic sequence in lock-step on one context: stream
    s starts at frame s, so round r gives stream s the frame s + r, while every stream has one (num_frames - streams + 1 rounds).  A round
    preprocesses each stream's scan, registers all streams by ONE BatchProblem.align against their maps, then updates the maps — by one
    api.insert_batch when batched_insert is set (the same maps, bit for bit: the results do not change), by one insert per stream
    otherwise; batched_problems: the round's problems are made by one api.create_problems (the same source orders, bit for bit), by one
    Problem per stream otherwise.  Returns per stream the poses (the first is the identity) and the iteration counts, the final map sizes, and the wall
    time of the map updates per round."""
    from . import synthetic

    if streams < 1 or num_frames < streams:
        raise ValueError("streams must be in [1, num_frames]")
    ctx = ctx or api.Context(0)
    setting = api.make_setting("VGICP", max_correspondence_distance=max_correspondence_distance)
    maps = [api.GaussianVoxelMap(voxel_resolution, ctx=ctx) for _ in range(streams)]
    poses = [[] for _ in range(streams)]
    iterations = [[] for _ in range(streams)]
    insert_s = 0.0
    for r in range(num_frames - streams + 1):
        clouds = []
        for s in range(streams):
            pts, _ = synthetic.kitti_like_scan(s + r)
            cloud = api.voxelgrid_sampling(api.PointCloud(np.ascontiguousarray(pts[:, :3], dtype=np.float32), ctx=ctx), downsampling_resolution)
            api.estimate_covariances(cloud, None, num_neighbors)
            clouds.append(cloud)
        if r == 0:
            Ts = [np.eye(4) for _ in range(streams)]
        else:
            prev = [poses[s][-1] for s in range(streams)]
            problems = api.create_problems(maps, clouds, prev, ctx=ctx) if batched_problems else [api.Problem(maps[s], clouds[s], prev[s], ctx=ctx) for s in range(streams)]
            bp = api.BatchProblem(problems)
            results = bp.align(setting, prev)
            del bp  # before its problems
            Ts = [res.T_target_source for res in results]
            for s, res in enumerate(results):
                iterations[s].append(res.iterations + 1)
        ctx.synchronize()
        t0 = time.perf_counter()
        if batched_insert:
            api.insert_batch(maps, clouds, Ts)
        else:
            for s in range(streams):
                maps[s].insert(clouds[s], Ts[s])
        ctx.synchronize()
        insert_s += time.perf_counter() - t0
        for s in range(streams):
            poses[s].append(np.array(Ts[s], dtype=np.float64))
    return {"frames": num_frames, "streams": streams, "poses": poses, "iterations": iterations, "num_voxels": [m.size() for m in maps],
            "insert_ms_per_round": 1e3 * insert_s / max(1, num_frames - streams + 1)}


def run_synthetic_pairs(num_frames, rank, world, device=0, **kw):
    """Frame-pair parallelism over ranks (the other way to spread C5 over GPUs): under the reference's protocol every pair (scan f-1, scan f)
    is registered from the identity (odometry_benchmark_small_gicp_omp.cpp:16-49), so the pairs are independent — rank r takes the
    contiguous block of frames [r F / W, (r + 1) F / W), preprocesses those scans plus the one before the block, and registers its pairs
    on a context of its own with no collective at all.  Returns this rank's wall time, its relative poses {f: T_(f-1) f} and frame count;
    the job's ms/scan is max over ranks of the wall time / F.  flow=(P, R): the rank runs its block as a flow of stages (PipelinedOdometry: P
    preprocessing and R registration workers with a stream each) instead of frame by frame."""
    import time as _time

    from . import synthetic

    lo, hi = rank * num_frames // world, (rank + 1) * num_frames // world
    flow = kw.pop("flow", None)
    # generate the scans first: the generator is host work that a real stream would not pay
    scans = {f: synthetic.kitti_like_scan(f)[0] for f in range(max(lo - 1, 0), hi)}
    if flow:  # (preprocessing workers, registration workers): the rank's block through the flow form (PipelinedOdometry) on its device
        frames = sorted(scans)
        pipe = PipelinedOdometry(device=device, workers=flow[0], reg_workers=flow[1], **kw)
        pipe.run([scans[f] for f in frames[: min(4, len(frames))]])  # first-touch allocations, code objects
        poses, el, _ = pipe.run([scans[f] for f in frames])
        rel = {f: np.linalg.inv(poses[k - 1]) @ poses[k] for k, f in enumerate(frames) if k > 0 and f >= max(lo, 1)}
        return {"seconds": el, "frames": hi - lo, "relative_poses": rel}
    odom = OnlineOdometry(ctx=api.Context(device), **kw)
    rel = {}
    odom.ctx.synchronize()
    t0 = _time.perf_counter()
    prev_T = None
    for f in sorted(scans):
        T = odom.estimate(scans[f])
        if prev_T is not None and f >= max(lo, 1):
            rel[f] = np.linalg.inv(prev_T) @ T
        prev_T = T
    odom.ctx.synchronize()
    el = _time.perf_counter() - t0
    odom.close()
    return {"seconds": el, "frames": hi - lo, "relative_poses": rel}


def run_synthetic_pipelined(num_frames=20, pinned=False, **kw):
    """Throughput of the two-stream pipeline on the synthetic sequence: wall time / frame with all frames in flight."""
    from . import synthetic

    scans = [synthetic.kitti_like_scan(f)[0] for f in range(num_frames)]
    if pinned:
        scans = [api.pinned_copy(s[:, :3], np.float32) for s in scans]
    odom = PipelinedOdometry(**kw)
    odom.run(scans[: min(3, num_frames)])  # first-touch allocations, code objects
    poses, wall, iters = odom.run(scans)
    return {"frames": num_frames, "ms_per_scan": 1e3 * wall / num_frames, "estimated": poses, "mean_iterations": float(np.mean(iters)) if iters else 0.0}


REVISITS = ((10, 150.0, (0.2, -0.15)), (30, -75.0, (-0.1, 0.25)), (50, 33.0, (0.3, 0.0)), (70, 180.0, (-0.15, -0.2)))


def _pose_error(T, T_ref):
    E = np.linalg.inv(T) @ T_ref
    R = E[:3, :3]
    s = 0.5 * float(np.linalg.norm([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]))
    return float(np.linalg.norm(E[:3, 3])), float(np.arctan2(s, (np.trace(R) - 1.0) / 2.0))


def run_synthetic_revisit(keyframes=tuple(range(0, 80, 2)), revisits=REVISITS, n_az=2030, downsampling_resolution=0.25, num_neighbors=10, rings=20, sectors=60, max_range=80.0, height=2.0, seed=1000,
                          from_identity=False, ctx=None):
    """Loop closure on the synthetic scene: a first pass stores the Scan Context descriptor of the scan at every
    keyframe pose of the arc (synthetic._sensor_pose(f), f in keyframes) in a PlaceDatabase; each revisit (frame, yaw in degrees, (dx, dy))
    then returns to a stored pose moved by (dx, dy) metres in the world frame and turned by yaw about z, looks its scan up, and
    registers it against the retrieved keyframe by GICP from yaw_guess(shift).  Per revisit: "retrieved" (the keyframe's frame),
    "rank" (where the revisited keyframe stands in the ranking, 0 = first), "shift", "distance", "place_error_m" (between the retrieved
    keyframe and the revisit), "yaw_error_rad" (the shift's yaw against the true one), "T" (GICP's T_keyframe_revisit), "converged",
    "pose_error" ((m, rad) against the generator's relative pose) and — from_identity — "identity_error", what GICP reaches without
    the guess."""
    from . import synthetic

    keyframes = tuple(keyframes)
    ctx = ctx or api.default_context()
    db = api.PlaceDatabase(ctx, rings, sectors, max_range, height)
    poses, clouds = [], []
    for f in keyframes:
        poses.append(synthetic._sensor_pose(f))
        clouds.append(api.PointCloud(synthetic.scan_at(poses[-1], n_az=n_az), ctx=ctx))
        db.add(clouds[-1])
    setting = api.make_setting("GICP")
    prepared = {}
    out = []
    for frame, yaw_deg, (dx, dy) in revisits:
        yaw = np.deg2rad(yaw_deg)
        Tq = synthetic._sensor_pose(frame).copy()
        Tq[:3, 3] += [dx, dy, 0.0]
        Tq[:3, :3] = Tq[:3, :3] @ synthetic._rot([0, 0, 1], yaw)
        scan = api.PointCloud(synthetic.scan_at(Tq, n_az=n_az, seed=seed + frame), ctx=ctx)
        res = db.query(scan, k=1, return_all=True)
        i, shift = int(res["index"][0]), int(res["shift"][0])
        order = np.lexsort((np.arange(len(db)), res["all_distance"]))
        true = np.linalg.inv(poses[i]) @ Tq
        true_yaw = np.arctan2(true[1, 0], true[0, 0])
        if i not in prepared:
            prepared[i] = api.preprocess_points(clouds[i], downsampling_resolution, num_neighbors)
        _, tree = prepared[i]
        src, _ = api.preprocess_points(scan, downsampling_resolution, num_neighbors)
        guess = db.yaw_guess(shift)
        r = api.Problem(tree, src, guess).align(setting, guess)
        row = {
            "frame": frame, "yaw_deg": yaw_deg, "index": i, "retrieved": keyframes[i], "shift": shift, "distance": float(res["distance"][0]),
            "rank": int(np.flatnonzero(order == keyframes.index(frame))[0]) if frame in keyframes else None,
            "place_error_m": float(np.linalg.norm(poses[i][:3, 3] - Tq[:3, 3])),
            "yaw_error_rad": float((float(res["yaw"][0]) - true_yaw + np.pi) % (2.0 * np.pi) - np.pi),
            "T": r.T_target_source, "converged": bool(r.converged), "pose_error": _pose_error(r.T_target_source, true), "T_true": true,
        }
        if from_identity:
            r0 = api.Problem(tree, src, np.eye(4)).align(setting, np.eye(4))
            row["identity_error"] = _pose_error(r0.T_target_source, true)
        out.append(row)
    return {"keyframes": len(keyframes), "revisits": out}


def _cpp_driver(source, workdir, num_frames):
    """Write the synthetic sequence as KITTI .bin files under workdir/velodyne (once) and compile examples/<source> against the in-tree
    library.  Returns (executable, dataset directory)."""
    import os
    import subprocess

    from . import _lib, synthetic

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    data = os.path.join(workdir, "velodyne")
    os.makedirs(data, exist_ok=True)
    for f in range(num_frames):
        name = os.path.join(data, "%06d.bin" % f)
        if os.path.exists(name):
            continue
        pts, _ = synthetic.kitti_like_scan(f)
        v = np.zeros((len(pts), 4), "<f4")
        v[:, :3] = pts[:, :3]
        v.tofile(name)
    exe = os.path.join(workdir, os.path.splitext(source)[0])
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", source), "-o", exe, "-L" + libdir, "-lsmall_gicp_amd",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"])
    return exe, data


def run_synthetic_movers(num_frames=8, radius=0.5, min_size=10, min_points=1, downsampling_resolution=0.25, ctx=None, **visibility):
    """Where did the mover go?  At the generator's poses (no registration): keyframe f - 1 is the voxel grid of scan f - 1 with the
    moving sphere (synthetic.with_moving_sphere at synthetic.mover_centre(f - 1)); raw scan f, with the sphere one step on, sees through
    the points the sphere left behind (PointCloud.visibility(keep="seen_through")), and PointCloud.clusters groups them into objects
    (DESIGN.md section 3.26).  Keyword arguments beyond the named ones go to visibility.  Returns one dict per frame f = 1 .. num_frames - 1:
    "frame", "centre" (the sphere's true centre at f - 1 in the keyframe's frame), "seen_through" (the number of such points),
    "detections" (a list of {"seed", "size", "box" (2,3)}), "labels" (of the seen-through points) and the objects behind them: "keyframe",
    "scan", "T" (scan f into keyframe f - 1), "seen" (the seen-through cloud) and "kept" (its points' indices in the keyframe)."""
    from . import synthetic

    ctx = ctx or api.default_context()
    out = []
    prev = None
    for f in range(num_frames):
        pts, Tws = synthetic.kitti_like_scan(f)
        pts, _ = synthetic.with_moving_sphere(pts, Tws, synthetic.mover_centre(f))
        scan = api.PointCloud(pts, ctx=ctx)
        if prev is not None:
            key, Tkey = prev
            T = np.linalg.inv(Tkey) @ Tws
            _, seen, kept = key.visibility(scan, T, keep="seen_through", return_kept=True, **visibility)
            found = seen.clusters(radius, min_points=min_points, min_size=min_size)
            Ti = np.linalg.inv(Tkey)
            out.append({
                "frame": f,
                "centre": Ti[:3, :3] @ synthetic.mover_centre(f - 1) + Ti[:3, 3],
                "seen_through": seen.size(),
                "detections": [{"seed": int(s), "size": int(n), "box": b} for s, n, b in zip(found["seeds"], found["sizes"], found["boxes"])],
                "labels": found["labels"],
                "keyframe": key,
                "scan": scan,
                "T": T,
                "seen": seen,
                "kept": kept,
            })
        prev = (api.voxelgrid_sampling(scan, downsampling_resolution), Tws)
    return out


def run_synthetic_occupancy(num_frames=8, mover=True, mode=0, leaf=0.5, extent=(50.0, 32.0, 6.0), offset=(-10.13, -15.87, -2.31), min_range=1.0, max_range=40.0, threshold=0.0, window=5, poses=None,
                            ctx=None, **scan):
    """What is free, what is occupied?  The raw synthetic scans (synthetic.kitti_like_scan, keyword arguments beyond the named ones go
    to it; mover: through synthetic.with_moving_sphere at synthetic.mover_centre(frame)) are ray-cast into ONE OccupancyGrid (DESIGN.md
    section 3.29) at the poses SubmapOdometry(window) estimates for them (poses: a list of 4x4 world poses to use in their place, e.g.
    the generator's).  The grid has cells of `leaf` metres over `extent` metres from the first sensor's position plus `offset`.  mode 1
    integrates the endpoints only: the baseline without free space.  Returns a dict: "mode", "frames", "cells" (the unknown / free /
    occupied counts and the epoch), "ghost_cells" — the occupied cells whose centre lies within one radius of the mover's centre at an
    EARLIER frame and outside 1.1 radii of its centre at the last: the trail it left in the map (0 without a mover) —, "ghost_indices"
    (their linear indices), "scan_stats" (per scan), "poses" (world) and the objects behind them: "grid"."""
    from . import synthetic

    ctx = ctx or api.default_context()
    raw = []
    for f in range(num_frames):
        pts, Tws = synthetic.kitti_like_scan(f, **scan)
        if mover:
            pts, _ = synthetic.with_moving_sphere(pts, Tws, synthetic.mover_centre(f))
        raw.append((pts, Tws))
    T0 = raw[0][1]
    if poses is None:
        odom = SubmapOdometry(window=window)
        poses = [T0 @ odom.estimate(pts) for pts, _ in raw]  # the estimates are in the first scan's frame
        odom.close()
    origin = T0[:3, 3] + np.asarray(offset, dtype=np.float64)
    dims = [max(1, int(np.ceil(e / leaf))) for e in extent]
    grid = api.OccupancyGrid(origin, leaf, dims, ctx=ctx)
    stats = [grid.integrate(api.PointCloud(pts, ctx=ctx), T, min_range, max_range, mode, return_stats=True) for (pts, _), T in zip(raw, poses)]
    found = grid.export(threshold, "occupied")
    ghosts = np.zeros(0, np.int64)
    if mover and num_frames > 1:
        radius = 1.0
        w = found["cloud"].xyz64()  # the centres, in the world
        trail = np.zeros(len(w), bool)
        for f in range(num_frames - 1):
            trail |= np.linalg.norm(w - synthetic.mover_centre(f), axis=1) <= radius
        ghosts = found["indices"][trail & (np.linalg.norm(w - synthetic.mover_centre(num_frames - 1), axis=1) > 1.1 * radius)]
    return {"mode": mode, "frames": num_frames, "cells": grid.stats(threshold), "ghost_cells": int(len(ghosts)), "ghost_indices": ghosts, "scan_stats": stats, "poses": list(poses), "grid": grid}


def run_synthetic_ground(num_frames=4, distance_threshold=0.1, iterations=256, seed=0, max_angle_degrees=15.0, downsampling_resolution=0.25, radius=0.5, min_size=10, ctx=None):
    """The objects that stand on the ground.  For each raw synthetic.kitti_like_scan(f): the ground is the plane PointCloud.segment_plane
    finds under the constraint axis = +z within max_angle_degrees (keep="rest"), the rest is downsampled at
    downsampling_resolution and grouped by PointCloud.clusters(radius, min_size=min_size).  Returns one dict per frame: "frame", "plane"
    ((4,) n and d, sensor frame), "ground" (the plane's points), "ground_share" (of the scan), "inliers", "rmse", "best_hypothesis",
    "hypothesis_inliers", "scored", "refit", "rest_points" (after the voxel grid), "objects" (their number), "sizes", "boxes"
    ((C, 2, 3)), "largest_share" (the largest object's share of the downsampled rest) and the objects behind them: "scan", "rest" (the
    cloud without the ground), "kept" (its points' indices in the scan) and "labels" (of the downsampled rest)."""
    from . import synthetic

    ctx = ctx or api.default_context()
    out = []
    for f in range(num_frames):
        pts, _ = synthetic.kitti_like_scan(f)
        scan = api.PointCloud(pts, ctx=ctx)
        seg = scan.segment_plane(distance_threshold, iterations, seed, axis=(0.0, 0.0, 1.0), max_angle=np.radians(max_angle_degrees), keep="rest", return_kept=True)
        down = api.voxelgrid_sampling(seg["cloud"], downsampling_resolution)
        found = down.clusters(radius, min_size=min_size)
        sizes = found["sizes"]
        out.append({
            "frame": f,
            "plane": seg["plane"],
            "ground": seg["inliers"],
            "ground_share": seg["inliers"] / max(1, scan.size()),
            "inliers": seg["inliers"],
            "rmse": seg["rmse"],
            "best_hypothesis": seg["best_hypothesis"],
            "hypothesis_inliers": seg["hypothesis_inliers"],
            "scored": seg["scored"],
            "refit": seg["refit"],
            "rest_points": down.size(),
            "objects": found["num_clusters"],
            "sizes": sizes,
            "boxes": found["boxes"],
            "largest_share": (float(sizes.max()) / max(1, down.size())) if len(sizes) else 0.0,
            "scan": scan,
            "rest": seg["cloud"],
            "kept": seg["kept"],
            "labels": found["labels"],
        })
    return out


def _read_trajectory(path):
    poses = []
    for ln in open(path):
        T = np.eye(4)
        T[:3, :4] = np.array(ln.split(), dtype=np.float64).reshape(3, 4)
        poses.append(T)
    return poses


def run_synthetic_cpp(num_frames=20, workdir=None, downsampling_resolution=0.25, num_neighbors=20):
    """The same sequence through the C++ driver examples/odometry_benchmark.cpp (the reference's benchmark protocol over
    include/small_gicp_amd.hpp): writes the scans as KITTI .bin files, compiles the driver with g++ against the in-tree library, runs it and
    parses its report and trajectory.  Returns registration / total ms per scan as the driver measured them and the poses."""
    import re
    import shutil
    import subprocess
    import tempfile

    own = workdir is None
    workdir = workdir or tempfile.mkdtemp(prefix="sga_odom_cpp_")
    try:
        exe, data = _cpp_driver("odometry_benchmark.cpp", workdir, num_frames)
        traj = os.path.join(workdir, "traj.txt")
        p = subprocess.run([exe, data, traj, "--num_neighbors", str(num_neighbors), "--downsampling_resolution", str(downsampling_resolution), "--max_frames", str(num_frames)], capture_output=True, text=True, timeout=600)
        if p.returncode != 0:
            raise RuntimeError("odometry_benchmark failed: " + p.stdout[-1000:] + p.stderr[-1000:])
        m = re.search(r"registration_time_stats=([0-9.eE+-]+) \+- ([0-9.eE+-]+) \[msec/scan\]\s+total_throughput=([0-9.eE+-]+) \+- ([0-9.eE+-]+) \[msec/scan\]\s+mean_iterations=([0-9.eE+-]+)", p.stdout)
        if m is None:
            raise RuntimeError("no report in the driver's output: " + p.stdout[-1000:])
        return {"frames": num_frames, "registration_ms_per_scan": float(m.group(1)), "registration_ms_std": float(m.group(2)), "total_ms_per_scan": float(m.group(3)), "mean_iterations": float(m.group(5)),
                "estimated": _read_trajectory(traj), "driver": "examples/odometry_benchmark.cpp (C++ over include/small_gicp_amd.hpp), all scans read into host memory first"}
    finally:
        if own:
            shutil.rmtree(workdir, ignore_errors=True)


def run_synthetic_cpp_flow(num_frames=20, workdir=None, downsampling_resolution=0.25, num_neighbors=20, preprocess_workers=2, registration_workers=2, pinned=False, repeat=3, env=None):
    """The same sequence through the C++ FLOW driver examples/odometry_benchmark_flow.cpp — the throughput protocol of the reference's TBB
    flow-graph engine (odometry_benchmark_small_gicp_tbb_flow.cpp:50-141): preprocessing and registration stages on threads with a HIP
    stream each, pairs registered side by side, poses multiplied up in frame order.  Returns the best total_throughput [ms/scan] of the runs
    after the first (which carries code-object loads and first allocations), every run's figure and the trajectory of the last run."""
    import re
    import shutil
    import subprocess
    import tempfile

    own = workdir is None
    workdir = workdir or tempfile.mkdtemp(prefix="sga_odom_flow_")
    try:
        exe, data = _cpp_driver("odometry_benchmark_flow.cpp", workdir, num_frames)
        traj = os.path.join(workdir, "traj_flow.txt")
        cmd = [exe, data, traj, "--num_neighbors", str(num_neighbors), "--downsampling_resolution", str(downsampling_resolution), "--max_frames", str(num_frames), "--preprocess_workers", str(preprocess_workers),
               "--registration_workers", str(registration_workers), "--repeat", str(max(2, repeat))] + (["--pinned"] if pinned else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, **(env or {})))
        if p.returncode != 0:
            raise RuntimeError("odometry_benchmark_flow failed: " + p.stdout[-1000:] + p.stderr[-1000:])
        runs = [(float(a), float(b), float(c)) for a, b, c in re.findall(r"total_throughput=([0-9.eE+-]+) \[msec/scan\]\s+frame_latency=([0-9.eE+-]+) \[msec\]\s+mean_iterations=([0-9.eE+-]+)", p.stdout)]
        if len(runs) < 2:
            raise RuntimeError("no report in the driver's output: " + p.stdout[-1000:])
        best = min(runs[1:])
        return {"frames": num_frames, "ms_per_scan": best[0], "frame_latency_ms": best[1], "mean_iterations": best[2], "runs_ms_per_scan": [r[0] for r in runs], "preprocess_workers": preprocess_workers,
                "registration_workers": registration_workers, "scans_in_pinned_host_memory": bool(pinned), "estimated": _read_trajectory(traj),
                "driver": "examples/odometry_benchmark_flow.cpp (C++ threads over include/small_gicp_amd.hpp, a HIP stream per worker), all scans read into host memory first; best of the runs after the first"}
    finally:
        if own:
            shutil.rmtree(workdir, ignore_errors=True)


class Summarizer:
    """mean +- std (last=...) of a stream, formatted like benchmark.hpp:36-79."""

    def __init__(self):
        self.n, self.sum, self.sq, self.last = 0, 0.0, 0.0, 0.0

    def push(self, x):
        self.n += 1
        self.sum += x
        self.sq += x * x
        self.last = x

    def __str__(self):
        if self.n == 0:
            return "nan +- nan (last=nan)"
        mean = self.sum / self.n
        var = max(0.0, (self.sq - mean * self.sum) / self.n)
        return "%.3f +- %.3f (last=%.3f)" % (mean, var ** 0.5, self.last)


def run_kitti(dataset_path, output_path=None, num_frames=None, downsampling_resolution=0.25, num_neighbors=20, quiet=False):
    """The reference's odometry benchmark on a directory of KITTI `.bin` scans (src/benchmark/odometry_benchmark.cpp:20-97 with the
    small_gicp engine, odometry_benchmark_small_gicp_omp.cpp:16-57): prints the same parameter / report lines and writes the
    trajectory in the KITTI text format.  Returns the list of poses T_world_sensor."""
    from . import io

    names = io.list_kitti_scans(dataset_path, num_frames or 1000000)
    if not quiet:
        print("dataset_path=%s" % dataset_path)
        print("registration_engine=small_gicp_amd")
        print("num_neighbors=%d" % num_neighbors)
        print("downsampling_resolution=%g" % downsampling_resolution)
        print("num_frames=%d" % len(names))
    odom = OnlineOdometry(downsampling_resolution=downsampling_resolution, num_neighbors=num_neighbors)
    reg, tot = Summarizer(), Summarizer()
    traj = []
    for i, name in enumerate(names):
        if i and i % 256 == 0 and not quiet:
            print("registration_time_stats=%s [msec/scan]  total_throughput=%s [msec/scan]" % (reg, tot))
        pts = io.read_points(name)
        traj.append(odom.estimate(pts[:, :3]))
        reg.push(odom.reg_ms[-1])
        tot.push(odom.total_ms[-1])
    if not quiet:
        print("done!")
        print("registration_time_stats=%s [msec/scan]  total_throughput=%s [msec/scan]" % (reg, tot))
    if output_path:
        io.write_trajectory(output_path, traj)
    return traj


def main(argv=None):
    import argparse

    ap = argparse.ArgumentParser(description="scan-to-scan GICP odometry on the GPU: odometry <dataset_path> <output_path> [options]")
    ap.add_argument("dataset_path", help="directory of KITTI .bin scans, or 'synthetic' for the frozen synthetic sequence")
    ap.add_argument("output_path", nargs="?", default=None, help="trajectory file (KITTI text format)")
    ap.add_argument("--num_frames", type=int, default=None)
    ap.add_argument("--num_neighbors", type=int, default=20)
    ap.add_argument("--downsampling_resolution", type=float, default=0.25)
    a = ap.parse_args(argv)
    if a.dataset_path == "synthetic":
        from . import io

        r = run_synthetic(a.num_frames or 20, downsampling_resolution=a.downsampling_resolution, num_neighbors=a.num_neighbors)
        print("registration_time=%.3f [msec/scan]  total=%.3f [msec/scan]  rpe_trans=%.4f m  rpe_rot=%.5f rad" % (r["registration_ms_per_scan"], r["total_ms_per_scan"], r["rpe_trans_m_mean"], r["rpe_rot_rad_mean"]))
        if a.output_path:
            io.write_trajectory(a.output_path, r["estimated"])
    else:
        run_kitti(a.dataset_path, a.output_path, a.num_frames, a.downsampling_resolution, a.num_neighbors)


if __name__ == "__main__":
    main()

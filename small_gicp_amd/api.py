"""Python host layer over the C-ABI, mirroring the reference's Python module surface
(src/python/{pointcloud,kdtree,voxelmap,preprocess,align,result}.cpp of /root/reference): PointCloud, KdTree,
GaussianVoxelMap, voxelgrid_sampling, estimate_*, preprocess_points, align, RegistrationResult.
All compute happens in the HIP library; numpy only carries host buffers in and out.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GICP, ICP, PLANE_ICP, FactorParams, RegistrationSettingC, ResultC, check, load

_FACTOR_BY_NAME = {"ICP": ICP, "PLANE_ICP": PLANE_ICP, "GICP": GICP, "VGICP": GICP}


def _fp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _T16(T):
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64).reshape(4, 4)
    return np.ascontiguousarray(T.T).reshape(16)  # column-major


class Context:
    """One GPU + one HIP stream (sga_context)."""

    def __init__(self, device=0, stream=None):
        self.h = C.c_void_p()
        L = load()
        if stream is None:
            check(L.sga_context_create(int(device), C.byref(self.h)))
        else:
            check(L.sga_context_create_on_stream(int(device), C.c_void_p(int(stream)), C.byref(self.h)))
        self.device = device

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_context_destroy(self.h)
            self.h = C.c_void_p()

    def synchronize(self):
        check(load().sga_context_synchronize(self.h))

    @staticmethod
    def comm_unique_id():
        """128-byte RCCL unique id (create on rank 0, hand to the other ranks out of band)."""
        buf = (C.c_ubyte * 128)()
        check(load().sga_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id):
        """Join the RCCL communicator: afterwards linearize/error/align all-reduce their accumulators over the ranks."""
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check(load().sga_comm_init(self.h, int(nranks), int(rank), buf))

    def comm_init_callback(self, nranks, rank, allreduce):
        """The same protocol with the caller's transport: allreduce(values) must return the element-wise sum over all ranks of the
        numpy array it is given (e.g. a torch.distributed / MPI all-reduce on the host)."""
        from ._lib import ALLREDUCE_FN

        def _cb(_user, ptr, count):
            try:
                a = np.ctypeslib.as_array(ptr, shape=(count,))
                a[:] = np.asarray(allreduce(a.copy()), dtype=np.float64).reshape(count)
                return 0
            except Exception:  # noqa: BLE001
                import traceback

                traceback.print_exc()
                return 1

        self._allreduce_cb = ALLREDUCE_FN(_cb)  # keep alive as long as the context
        check(load().sga_comm_init_callback(self.h, int(nranks), int(rank), self._allreduce_cb, None))

    def comm_destroy(self):
        check(load().sga_comm_destroy(self.h))

    def set_stream_ordered(self, enabled=True):
        """Index builds and normal / covariance estimation return once enqueued (results ordered for later calls on this context; a
        consumer on another context waits for the producer's event).  Returns the previous mode."""
        prev = getattr(self, "stream_ordered", False)
        check(load().sga_context_set_stream_ordered(self.h, int(enabled)))
        self.stream_ordered = bool(enabled)
        return prev

    def _set_voxelgrid_epoch(self, epoch):
        """Diagnostics (sga_debug_set_voxelgrid_epoch): the launch epoch of this context's voxel-grid calls; forwards only."""
        check(load().sga_debug_set_voxelgrid_epoch(self.h, int(epoch)))

    def gpu_time_ms(self, fn):
        """GPU time (HIP events on the context's stream) of whatever fn() enqueues; returns (milliseconds, fn's result)."""
        check(load().sga_debug_timer_start(self.h))
        r = fn()
        ms = C.c_double()
        check(load().sga_debug_timer_stop(self.h, C.byref(ms)))
        return ms.value, r

    def set_profiling(self, enabled=True):
        check(load().sga_context_set_profiling(self.h, int(enabled)))

    def kernel_ms(self):
        lm, em = C.c_double(), C.c_double()
        lc, ec = C.c_uint64(), C.c_uint64()
        check(load().sga_context_get_kernel_ms(self.h, C.byref(lm), C.byref(lc), C.byref(em), C.byref(ec)))
        sm, sc = C.c_double(), C.c_uint64()
        check(load().sga_context_get_search_ms(self.h, C.byref(sm), C.byref(sc)))
        cm, wm = C.c_double(), C.c_double()
        cc, wc = C.c_uint64(), C.c_uint64()
        wf = C.c_double()
        check(load().sga_context_get_pass_ms(self.h, C.byref(cm), C.byref(cc), C.byref(wm), C.byref(wc), C.byref(wf)))
        km, kc = C.c_double(), C.c_uint64()
        check(load().sga_context_get_comm_ms(self.h, C.byref(km), C.byref(kc)))
        return {"linearize_ms": lm.value, "linearize_calls": lc.value, "error_ms": em.value, "error_calls": ec.value, "search_ms": sm.value, "search_calls": sc.value,
                "cold_ms": cm.value, "cold_calls": cc.value, "warm_ms": wm.value, "warm_calls": wc.value, "warm_search_ms": wf.value,
                "comm_ms": km.value, "comm_calls": kc.value}


_DEFAULT_CTX = None


def default_context():
    global _DEFAULT_CTX
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = Context(0)
    return _DEFAULT_CTX


def sym6_from_mats(covs):
    """(N,3,3) or (N,4,4) symmetric -> (N,6) xx,xy,xz,yy,yz,zz"""
    c = np.asarray(covs)
    return np.stack([c[:, 0, 0], c[:, 0, 1], c[:, 0, 2], c[:, 1, 1], c[:, 1, 2], c[:, 2, 2]], axis=1)


def mats_from_sym6(c6):
    c6 = np.asarray(c6)
    m = np.empty((len(c6), 3, 3), dtype=c6.dtype)
    m[:, 0, 0], m[:, 0, 1], m[:, 0, 2] = c6[:, 0], c6[:, 1], c6[:, 2]
    m[:, 1, 0], m[:, 1, 1], m[:, 1, 2] = c6[:, 1], c6[:, 3], c6[:, 4]
    m[:, 2, 0], m[:, 2, 1], m[:, 2, 2] = c6[:, 2], c6[:, 4], c6[:, 5]
    return m


class _PinnedBlock:
    """Owner of one sga_host_alloc block (freed when the last array viewing it is gone)."""

    def __init__(self, nbytes):
        self.p = C.c_void_p()
        check(load().sga_host_alloc(int(nbytes), C.byref(self.p)))
        self.nbytes = int(nbytes)

    def __del__(self):
        if getattr(self, "p", None) and self.p.value:
            load().sga_host_free(self.p)
            self.p = C.c_void_p()


def pinned_empty(shape, dtype=np.float32):
    """A numpy array in pinned host memory (sga_host_alloc).  Scans read into such arrays are uploaded without a CPU copy: the device reads
    them in place (PointCloud(points) recognises them) — what a driver that preloads its scans into host memory should use
    (benchmark/benchmark_odom.hpp:36-47 keeps every scan in host memory before the timed loop).  The block is freed with the last array
    that views it."""
    dt = np.dtype(dtype)
    count = int(np.prod(shape)) if np.ndim(shape) else int(shape)
    block = _PinnedBlock(max(1, count * dt.itemsize))
    buf = (C.c_char * block.nbytes).from_address(block.p.value)
    buf._sga_block = block  # np.frombuffer keeps `buf` alive, `buf` keeps the block
    return np.frombuffer(buf, dtype=dt, count=count).reshape(shape)


def pinned_copy(a, dtype=np.float32):
    """`a` copied into pinned host memory (C-contiguous, `dtype`)."""
    a = np.asarray(a)
    out = pinned_empty(a.shape, dtype)
    out[...] = a
    return out


class PointCloud:
    """Device-resident point cloud (points [+ normals] [+ covariances]); mirrors small_gicp.PointCloud."""

    def __init__(self, points=None, normals=None, covs=None, ctx=None, _handle=None):
        self.ctx = ctx or default_context()
        if _handle is not None:
            self.h = _handle
            return
        pts = np.zeros((0, 3), np.float32) if points is None else np.asarray(points)
        if pts.ndim != 2 or pts.shape[1] not in (3, 4):
            raise ValueError("points must be (N,3) or (N,4)")
        nrm = None if normals is None else np.ascontiguousarray(np.asarray(normals)[:, :3], dtype=np.float32)
        c6 = None
        if covs is not None:
            covs = np.asarray(covs)
            c6 = covs if covs.ndim == 2 and covs.shape[1] == 6 else sym6_from_mats(covs)
            c6 = np.ascontiguousarray(c6, dtype=np.float32)
        self.h = C.c_void_p()
        if pts.dtype == np.float64 and len(pts) > 0:
            # double input (the reference's PointCloud is double, points/point_cloud.hpp:69-71): the device keeps fp32 records RELATIVE to an
            # origin (small_gicp_amd.h, "device frames"); the subtraction happens here, in double, so a geo-referenced cloud keeps its millimetres
            p3 = pts[:, :3]
            fin = np.isfinite(p3)
            lo = np.where(fin, p3, np.inf).min(axis=0).astype(np.float64)
            hi = np.where(fin, p3, -np.inf).max(axis=0).astype(np.float64)
            origin = np.zeros(3)
            load().sga_choose_origin(_dp(np.ascontiguousarray(lo)), _dp(np.ascontiguousarray(hi)), _dp(origin))
            rel = np.ascontiguousarray(p3 - origin if origin.any() else p3, dtype=np.float32)
            check(load().sga_cloud_create_f32_origin(self.ctx.h, _fp(rel), _fp(nrm), _fp(c6), len(rel), _dp(origin), C.byref(self.h)))
        else:
            # (an (N,3) float32 C-contiguous array — e.g. one from pinned_empty — goes down as it is: no copy on this side)
            xyz = pts if (pts.shape[1] == 3 and pts.dtype == np.float32 and pts.flags.c_contiguous) else np.ascontiguousarray(pts[:, :3], dtype=np.float32)
            check(load().sga_cloud_create_f32(self.ctx.h, _fp(xyz), _fp(nrm), _fp(c6), len(xyz), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_cloud_destroy(self.h)
            self.h = C.c_void_p()

    @staticmethod
    def from_torch(points, normals=None, covs=None, ctx=None, origin=None, relative=False, stream=None):
        """A cloud from torch tensors on the context's device, without a copy and without touching the host (sga_cloud_create_device):
        points (N,3) float32 / float64 — or a view such as scan[:, :3] of an (N,4) tensor: any row stride, last-dimension stride 1 —,
        normals (N,3), covs (N,6), (N,3,3) or (N,4,4).  origin None: chosen by the library as for host arrays; origin given: the points
        are recentred about it in double; relative=True: the points are relative to origin already.  stream: the hipStream_t the tensors
        were produced on (default: torch's current stream of the device); the library orders its reads behind it and the stream's later
        work behind its reads.  ValueError, before the library is called, for a CPU tensor, another device, another dtype or a
        transposed view."""
        return _cloud_from_torch(points, normals, covs, ctx, origin, relative, stream)

    @staticmethod
    def from_device_pointer(ptr, n, dtype=np.float32, stride=3, normals_ptr=None, normals_stride=3, covs_ptr=None, covs_cols=6, covs_stride=None, ctx=None, origin=None, relative=False, stream=0):
        """from_torch for callers without torch: ptr is device memory of the context's device (hipMalloc) holding n rows of `stride`
        elements of `dtype`, the first three of each a point; normals_ptr / covs_ptr likewise.  stream: the hipStream_t the memory was
        written on (0: the null stream)."""
        return _cloud_from_device_pointer(ptr, n, dtype, stride, normals_ptr, normals_stride, covs_ptr, covs_cols, covs_stride, ctx, origin, relative, stream)

    def to_torch(self, points=True, normals=False, covs=False, dtype=None, stream=None, out=None):
        """New tensors on the cloud's device written by the library (sga_cloud_export_device): points (N,3) in the caller's frame
        (origin added in double, rounded to dtype: torch.float32 by default, or torch.float64), normals (N,3), covs (N,6); one tensor, or
        a tuple in that order.  out: an (N,3) tensor or view (any row stride) to write the points into instead.  The tensors are ready
        for work on `stream` (default: torch's current stream)."""
        return _cloud_to_torch(self, points, normals, covs, dtype, stream, out)

    def origin(self):
        """Origin of the cloud's device frame (the device holds fl32(p - origin)); zero for clouds centred within 64 m of the origin."""
        o = np.zeros(3)
        check(load().sga_cloud_origin(self.h, _dp(o)))
        return o

    def size(self):
        n = C.c_size_t()
        check(load().sga_cloud_size(self.h, C.byref(n)))
        return n.value

    __len__ = size

    def point(self, i):
        """pointcloud.cpp: the i-th point as a homogeneous 4-vector (points/point_cloud.hpp:49)."""
        return self.points()[int(i)]

    def normal(self, i):
        return self.normals()[int(i)]

    def cov(self, i):
        return self.covs()[int(i)]

    def slice(self, first, count):
        """A new device cloud holding points [first, first + count) with their normals / covariances (sga_cloud_slice): the source
        shard of one rank when a registration is spread over GPUs."""
        h = C.c_void_p()
        check(load().sga_cloud_slice(self.ctx.h, self.h, int(first), int(count), C.byref(h)))
        return PointCloud(ctx=self.ctx, _handle=h)

    def transformed(self, T, origin=None):
        """A new cloud holding this one's points, normals and covariances posed by T (4x4; sga_cloud_transform): merge_clouds of one member."""
        return merge_clouds([self], [T], origin)

    def deskewed(self, times, twist, ref_time=1.0, stream=None):
        """This raw sweep with the sensor's motion undone, as a new cloud (sga_cloud_deskew): point i, measured at
        times[i] in the sensor frame of that instant, becomes exp((times[i] - ref_time) twist) p_i — the sensor frame at ref_time.  twist:
        the motion per unit of time, [rx ry rz tx ty tz] (se3_log of the sweep's relative pose when the times run from 0 to 1).  times: a
        numpy array (N,), or a torch tensor on the cloud's device — float32 or float64, 1-D with any stride, e.g. a column scan[:, 4] —
        which the device reads where it is (sga_cloud_deskew_device; stream: the hipStream_t it was produced on, default torch's current
        stream).  Normals and covariances are rotated along; the cloud keeps its origin."""
        xi = np.ascontiguousarray(np.asarray(twist, dtype=np.float64).reshape(6))
        h = C.c_void_p()
        if isinstance(times, np.ndarray) or not type(times).__module__.startswith("torch"):
            t = np.ascontiguousarray(np.asarray(times, dtype=np.float32).reshape(-1))
            if len(t) != self.size():
                raise ValueError(f"{len(t)} times for a cloud of {self.size()} points")
            check(load().sga_cloud_deskew(self.ctx.h, self.h, _fp(t), _dp(xi), float(ref_time), C.byref(h)))
        else:
            ta = _torch_times(times, self.size(), self.ctx)
            check(load().sga_cloud_deskew_device(self.ctx.h, self.h, C.byref(ta), _dp(xi), float(ref_time), C.c_void_p(_torch_stream(self.ctx, stream)), 0, C.byref(h)))
        return PointCloud(ctx=self.ctx, _handle=h)

    def cropped(self, min_range=0.0, max_range=np.inf, center=None, box=None, box_mode="inside", return_kept=False, stream=None):
        """This cloud without the returns nobody wants, as a new cloud (sga_cloud_crop): a point p (caller's
        frame) is kept when it is finite, min_range <= |p - center| <= max_range (center None: the origin of the caller's frame) and —
        box = (lo, hi), closed per axis — it lies inside the box (box_mode "inside") or not inside it ("outside": an ego-vehicle box).
        The defaults keep every finite point.  The order of the points, their normals and covariances and the cloud's origin are kept.
        return_kept: also the indices kept, ascending — (cloud, kept) — so that times, intensities or labels follow: a numpy int64
        array, or, when stream is given (a torch.cuda.Stream or a hipStream_t the caller works on: sga_cloud_crop_device), a torch int64
        tensor on the cloud's device that never touches the host."""
        cr = _crop(min_range, max_range, center, box, box_mode)
        n = self.size()
        h = C.c_void_p()
        if stream is None:
            kept = np.empty(n, np.int64) if return_kept else None
            check(load().sga_cloud_crop(self.ctx.h, self.h, C.byref(cr), None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(h)))
            out = PointCloud(ctx=self.ctx, _handle=h)
            return (out, kept[: out.size()].copy()) if return_kept else out
        import torch

        dev = torch.device("cuda", int(self.ctx.device))
        s = _torch_stream(self.ctx, stream)
        kept = None
        if return_kept:
            with torch.cuda.stream(torch.cuda.ExternalStream(s, device=dev)):  # (allocated on `stream`: torch's allocator orders its reuse behind it)
                kept = torch.empty((n,), dtype=torch.int64, device=dev)
        check(load().sga_cloud_crop_device(self.ctx.h, self.h, C.byref(cr), C.c_void_p(kept.data_ptr() if kept is not None and n > 0 else None), C.c_void_p(s), 0, C.byref(h)))
        out = PointCloud(ctx=self.ctx, _handle=h)
        return (out, kept[: out.size()]) if return_kept else out

    def without_outliers(self, k=10, std_mul=1.0, radius=None, tree=None, return_kept=False, return_stats=False):
        """This cloud without its isolated returns, as a new cloud (sga_cloud_remove_outliers).  Statistical
        mode (radius None): a point is kept when the mean distance to its k nearest neighbours is at most mean + std_mul * stddev of
        that figure over the cloud.  Radius mode (radius given): a point is kept when at least k other points lie within radius.
        tree: the KdTree over this cloud (None: a temporary one is built).  The order of the points, their normals and covariances and
        the cloud's origin are kept.  A cloud with a non-finite coordinate is refused: crop first (cropped() removes such points).
        return_kept: also the indices kept (numpy int64, ascending); return_stats: also a dict with the per-point statistic "stat"
        (numpy float64, this cloud's order), "mean", "stddev", "threshold" and "kept" — (cloud[, kept][, stats])."""
        f = _outlier_filter(k, std_mul, radius)
        n = self.size()
        kept = np.empty(n, np.int64) if return_kept else None
        stat = np.empty(n, np.float64) if return_stats else None
        st = _lib.OutlierStats() if return_stats else None
        h = C.c_void_p()
        check(load().sga_cloud_remove_outliers(self.ctx.h, self.h, None if tree is None else tree.h, C.byref(f), None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64)),
                                               None if stat is None else _dp(stat), None if st is None else C.byref(st), C.byref(h)))
        out = PointCloud(ctx=self.ctx, _handle=h)
        res = [out]
        if return_kept:
            res.append(kept[: out.size()].copy())
        if return_stats:
            res.append({"stat": stat, "mean": st.mean, "stddev": st.stddev, "threshold": st.threshold, "kept": int(st.kept)})
        return res[0] if len(res) == 1 else tuple(res)

    def clusters(self, radius, min_points=1, min_size=1, max_size=None, tree=None, keep=None, return_table=True, table_capacity=None):
        """The objects of this cloud (sga_cloud_cluster): DBSCAN with a deterministic border rule.  A point with
        at least min_points records within radius (itself included; d2 <= radius^2 in double) is a core point; core points within
        radius of each other share a cluster; a non-core point joins the cluster of its nearest core point within radius (ties: the
        lowest index) or is noise; clusters of fewer than min_size or more than max_size (None: no limit) members are dropped; the
        kept ones are numbered in ascending order of their seed, the lowest index among their core points.  tree: the KdTree over this
        cloud (None: a temporary one).  A cloud with a non-finite coordinate is refused: crop first.  Returns a dict: "labels" (numpy
        int32, -1 for noise and dropped), "num_clusters", "noise", "dropped" and — with return_table — "seeds", "sizes" (int64) and
        "boxes" ((C, 2, 3) float64: min and max corner, caller's frame) of the first table_capacity clusters (None: all of them, by a
        second call when more than 1024 are found), and "cloud" — the clustered points or the others — when keep is "clustered" or
        "rest" (this cloud's order, normals, covariances and origin), then also "kept" (numpy int64: their indices)."""
        p = _cluster_params(radius, min_points, min_size, max_size, keep)
        n = self.size()
        cap = 0 if not return_table else (1024 if table_capacity is None else int(table_capacity))
        lib = load()
        while True:
            labels = np.empty(n, np.int32)
            rows = (_lib.ClusterRow * max(1, cap))()
            kept = np.empty(n, np.int64) if p.keep != 0 else None
            res = _lib.ClusterResult()
            h = C.c_void_p()
            check(lib.sga_cloud_cluster(self.ctx.h, self.h, None if tree is None else tree.h, C.byref(p), labels.ctypes.data_as(C.POINTER(C.c_int32)), rows if cap > 0 else None, cap,
                                        None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(res), C.byref(h) if p.keep != 0 else None))
            cloud = PointCloud(ctx=self.ctx, _handle=h) if p.keep != 0 else None
            if return_table and table_capacity is None and res.clusters > res.rows:
                cap = int(res.clusters)  # (the labels are a function of the records: the second call gives the same ones)
                continue
            break
        out = {"labels": labels, "num_clusters": int(res.clusters), "noise": int(res.noise), "dropped": int(res.dropped)}
        if return_table:
            table = np.frombuffer(rows, dtype=CLUSTER_ROW_DTYPE, count=int(res.rows)) if res.rows else np.zeros(0, CLUSTER_ROW_DTYPE)
            out["seeds"], out["sizes"] = table["seed"].copy(), table["size"].copy()
            out["boxes"] = np.stack([table["lo"], table["hi"]], axis=1).astype(np.float64).reshape(-1, 2, 3)
        if cloud is not None:
            out["cloud"], out["kept"] = cloud, kept[: cloud.size()].copy()
        return out

    def segment_plane(self, distance_threshold=0.1, iterations=1000, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, keep=None, return_kept=False, return_scores=False):
        """The dominant plane of this cloud (sga_cloud_segment_plane): RANSAC over `iterations` triples drawn by
        the counter-based generator under `seed`, scored by the records within distance_threshold, the best one refitted to its inliers
        (refit).  axis, max_angle: only planes whose normal lies within max_angle (radians) of +-axis are considered, and the normal
        is turned towards the axis; without an axis the normal's first non-zero of (z, y, x) is positive.  A plane is reported only
        with at least min_inliers points on the best hypothesis.  The result is a function of the records, the arguments and the seed
        alone.  Returns a dict: "plane" ((4,) float64: n and d with n . p + d = 0 in the caller's frame; zeros when none is found),
        "inliers", "rmse", "hypothesis_inliers", "best_hypothesis", "scored", "refit"; with keep "plane" or "rest" also "cloud" — the
        plane's points or all the others, records with a non-finite coordinate among the others (this cloud's order, normals,
        covariances and origin) — and, with return_kept, "kept" (numpy int64: their indices); with return_scores "scores" (numpy
        uint32 per hypothesis, 0xFFFFFFFF for a dropped one)."""
        p = _plane_params(distance_threshold, iterations, seed, axis, max_angle, min_inliers, refit, keep)
        n = self.size()
        plane = np.zeros(4, np.float64)
        scores = np.empty(max(int(p.iterations), 1) if 0 < p.iterations <= (1 << 20) else 1, np.uint32) if return_scores else None
        kept = np.empty(n, np.int64) if (return_kept and p.keep != 0) else None
        res = _lib.PlaneResult()
        h = C.c_void_p()
        check(load().sga_cloud_segment_plane(self.ctx.h, self.h, C.byref(p), _dp(plane), None if scores is None else scores.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(h) if p.keep != 0 else None, C.byref(res)))
        out = {"plane": plane, "inliers": int(res.inliers), "rmse": float(res.rmse), "hypothesis_inliers": int(res.hypothesis_inliers), "best_hypothesis": int(res.best_hypothesis),
               "scored": int(res.scored), "refit": int(res.refit)}
        if p.keep != 0:
            out["cloud"] = PointCloud(ctx=self.ctx, _handle=h)
            if kept is not None:
                out["kept"] = kept[: out["cloud"].size()].copy()
        if return_scores:
            out["scores"] = scores
        return out

    def iss_keypoints(self, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, tree=None, keep=False, return_saliency=False):
        """The salient points of this cloud (sga_cloud_iss_keypoints): Intrinsic Shape Signatures.  With the
        eigenvalues l1 >= l2 >= l3 of the unweighted covariance of the records within salient_radius (the point included; d2 <=
        radius^2 in double), a point's saliency is l3 when it has at least min_neighbors such records, l2 < gamma_21 l1, l3 <
        gamma_32 l2 and l3 > 1e-9 l1, and 0 otherwise; a keypoint is a salient point with at least min_neighbors records within
        non_max_radius none of which has a greater saliency (ties: the lowest index).  tree: the KdTree over this cloud (None: a
        temporary one).  A cloud with a non-finite coordinate is refused: crop first.  Returns a dict: "indices" (numpy int64,
        ascending), "count", with keep "cloud" (the keypoints with this cloud's normals, covariances and origin), with
        return_saliency "saliency" (numpy float64 per point)."""
        p = _iss_params(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, keep)
        n = self.size()
        kept = np.empty(n, np.int64)
        sal = np.empty(n, np.float64) if return_saliency else None
        cnt = C.c_size_t()
        h = C.c_void_p()
        check(load().sga_cloud_iss_keypoints(self.ctx.h, self.h, None if tree is None else tree.h, C.byref(p), _dp(sal) if n else None, kept.ctypes.data_as(C.POINTER(C.c_int64)) if n else None, C.byref(cnt),
                                             C.byref(h) if p.keep != 0 else None))
        out = {"indices": kept[: cnt.value].copy(), "count": int(cnt.value)}
        if p.keep != 0:
            out["cloud"] = PointCloud(ctx=self.ctx, _handle=h)
        if return_saliency:
            out["saliency"] = sal
        return out

    def fpfh(self, tree=None, k=20, viewpoint=(0.0, 0.0, 0.0)):
        """One 33-bin Fast Point Feature Histogram per point, as Features on the device (sga_cloud_fpfh).  The
        cloud needs normals.  tree: the KdTree over this cloud (None: a temporary one is built).  k: neighbours per point, 2 .. 63.
        viewpoint: a point of the caller's frame the normals are turned towards for the descriptor (nothing is written back); None:
        the normals as stored."""
        vp = None if viewpoint is None else np.ascontiguousarray(np.asarray(viewpoint, dtype=np.float64).reshape(3))
        h = C.c_void_p()
        check(load().sga_cloud_fpfh(self.ctx.h, self.h, None if tree is None else tree.h, int(k), _dp(vp), C.byref(h)))
        return Features(ctx=self.ctx, _handle=h)

    def scan_context(self, rings=None, sectors=None, max_range=None, height=None, center=None):
        """The Scan Context descriptor of this cloud (sga_cloud_scan_context): an (rings, sectors) float32 image
        of the greatest height + `height` per polar cell about `center` (the sensor's position in the cloud's coordinates; None:
        zeros), out to max_range.  None: the library's default (20, 60, 80.0, 2.0)."""
        p = _place_params(rings=rings, sectors=sectors, max_range=max_range, height=height)
        out = np.empty((p.rings, p.sectors), np.float32) if 0 < p.rings * p.sectors <= 4096 else np.empty((1, 1), np.float32)
        check(load().sga_cloud_scan_context(self.ctx.h, self.h, C.byref(p), _dp(_center3(center)), _fp(out)))
        return out

    def overlap(self, target, T=None, max_distance=1.0, keep=None, return_dist=False, return_nearest=False, return_kept=False, ctx=None):
        """How much of this cloud, posed by T (4x4, cloud -> target; None: the identity), the target already explains, and which points
        are new (sga_cloud_overlap).  target: a KdTree, a GaussianVoxelMap or a flat map.  A point is matched
        when its nearest target record (kd-tree: the exact nearest point; maps: the lookup over the map's search offsets) lies within
        max_distance.  Returns a dict — "points", "matched", "fitness" = matched / points, "rmse" and "mean_distance" over the matched —
        followed, as requested and in this order, by the cloud of the matched or the unmatched points (keep="matched" | "unmatched":
        this cloud's order, normals, covariances and origin; points with a non-finite coordinate are in neither), "dist" (numpy
        float64: the distance per point, +inf where unmatched), "nearest" (numpy int64: the target point's index, the voxel id, or
        voxel * 16 + slot for a flat map; -1 where unmatched) and "kept" (numpy int64: the indices of the output cloud's points,
        ascending; needs keep).  ctx: the context the call runs on (default: this cloud's)."""
        p = _overlap_params(max_distance, keep)
        ctx = ctx or self.ctx
        n = self.size()
        t16 = None if T is None else _T16(T)
        dist = np.empty(n, np.float64) if return_dist else None
        nearest = np.empty(n, np.int64) if return_nearest else None
        kept = np.empty(n, np.int64) if return_kept else None
        st = _lib.OverlapStats()
        h = C.c_void_p()
        _i64 = C.POINTER(C.c_int64)
        check(load().sga_cloud_overlap(ctx.h, self.h, target.h, _dp(t16), C.byref(p), _dp(dist), None if nearest is None else nearest.ctypes.data_as(_i64),
                                       None if kept is None else kept.ctypes.data_as(_i64), C.byref(st), C.byref(h) if p.keep != 0 else None))
        res = [{"points": int(st.points), "matched": int(st.matched), "fitness": st.fitness, "rmse": st.rmse, "mean_distance": st.mean_distance}]
        out = None
        if p.keep != 0:
            out = PointCloud(ctx=ctx, _handle=h)
            res.append(out)
        if return_dist:
            res.append(dist)
        if return_nearest:
            res.append(nearest)
        if return_kept:
            res.append(kept[: out.size()].copy())
        return res[0] if len(res) == 1 else tuple(res)

    def visibility(self, scan, T=None, *, width=None, height=None, fov_up=None, fov_down=None, min_range=None, max_range=None, margin=None, margin_ratio=None, window_h=None, window_v=None, keep=None,
                   return_state=False, return_clearance=False, return_image=False, return_kept=False, params=None, ctx=None):
        """The free-space check with this cloud as the map (sga_cloud_visibility): which of its points does `scan`,
        posed by T (4x4: the scan's sensor frame — x forward, y left, z up — into this cloud's frame; None: the identity), see through?
        The scan's returns form a range image of width x height cells over [fov_down, fov_up] (radians) holding the least range from
        min_range on; a map point is unobserved (state 0: out of the image, out of [min_range, max_range], no return in its window of
        (2 window_h + 1) x (2 window_v + 1) cells), seen through (3: every return of the window lies more than margin + margin_ratio *
        range behind it), occluded (2: it lies more than that behind every return) or consistent (1).  Returns a dict — "points",
        "unobserved", "consistent", "occluded", "seen_through" — followed, as requested and in this order, by the cloud of the seen-through
        points or of all the others (keep="seen_through" | "rest": this cloud's order, normals, covariances and origin; points with a
        non-finite coordinate are in neither), "state" (numpy uint8), "clearance" (numpy float64: the window's least range minus the
        point's, NaN where unobserved), "image" (numpy float64 (height, width), +inf where empty) and "kept" (numpy int64: the indices of
        the output cloud's points, ascending; needs keep).  A parameter left at None takes the library's default (sga_visibility_default:
        1024 x 64 over [-25, +3] degrees, ranges 0.5 .. 60 m, margin 0.2 m + 1 %, window 1 x 1).  params: a dict of the keyword arguments
        above, in their place.  ctx: the context the call runs on (default: this cloud's)."""
        given = dict(width=width, height=height, fov_up=fov_up, fov_down=fov_down, min_range=min_range, max_range=max_range, margin=margin, margin_ratio=margin_ratio, window_h=window_h, window_v=window_v)
        given.update(params or {})
        given = {name: value for name, value in given.items() if value is not None}
        p = _visibility_params(keep=keep, **given)
        ctx = ctx or self.ctx
        n = self.size()
        t16 = None if T is None else _T16(T)
        state = np.empty(n, np.uint8) if return_state else None
        clearance = np.empty(n, np.float64) if return_clearance else None
        image = np.empty((p.height, p.width), np.float64) if return_image else None
        kept = np.empty(n, np.int64) if return_kept else None
        st = _lib.VisibilityStats()
        h = C.c_void_p()
        check(load().sga_cloud_visibility(ctx.h, self.h, scan.h, _dp(t16), C.byref(p), None if state is None else state.ctypes.data_as(C.POINTER(C.c_uint8)), _dp(clearance), _dp(image),
                                          None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st), C.byref(h) if p.keep != 0 else None))
        res = [{"points": int(st.points), "unobserved": int(st.unobserved), "consistent": int(st.consistent), "occluded": int(st.occluded), "seen_through": int(st.seen_through)}]
        out = None
        if p.keep != 0:
            out = PointCloud(ctx=ctx, _handle=h)
            res.append(out)
        if return_state:
            res.append(state)
        if return_clearance:
            res.append(clearance)
        if return_image:
            res.append(image)
        if return_kept:
            res.append(kept[: out.size()].copy())
        return res[0] if len(res) == 1 else tuple(res)

    def selected(self, indices):
        """A new cloud whose point j is this cloud's point indices[j], with its normal and covariance (sga_cloud_select: one launch).
        Repeats are allowed, the order is as given, the origin is kept; an index outside [0, size) is refused and named by its position."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        h = C.c_void_p()
        check(load().sga_cloud_select(self.ctx.h, self.h, idx.ctypes.data_as(C.POINTER(C.c_int64)), len(idx), C.byref(h)))
        return PointCloud(ctx=self.ctx, _handle=h)

    def empty(self):
        return self.size() == 0

    def _voxelgrid_plan(self, leaf):
        """Diagnostics (sga_debug_voxelgrid_plan): what voxelgrid_sampling(self, leaf) would do — key_bytes (4 / 8), bits (x, y, z), total,
        box (the key layout comes from the cloud's box), sort (0 / 1 / 2: csrc/sort_util.hpp sort_path), tiles of ds_segments_kernel,
        speculative (the centroid kernel is launched before the voxel count is known).  All 0 for an empty cloud."""
        out = (C.c_int * 9)()
        check(load().sga_debug_voxelgrid_plan(self.h, float(leaf), out))
        return {"key_bytes": out[0], "bits": (out[1], out[2], out[3]), "total": out[4], "box": bool(out[5]), "sort": out[6], "tiles": out[7], "speculative": bool(out[8])}

    def _box(self):
        """Diagnostics (sga_debug_cloud_box): (lo (3,), hi (3,)) float32, the box of the finite records in the device frame that the cloud
        carries, or None when it carries none."""
        has, lo, hi = C.c_int(), np.zeros(3, np.float32), np.zeros(3, np.float32)
        check(load().sga_debug_cloud_box(self.h, C.byref(has), _fp(lo), _fp(hi)))
        return (lo, hi) if has.value else None

    def _has(self):
        a, b = C.c_int(), C.c_int()
        check(load().sga_cloud_has(self.h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def points(self):
        """(N,4) float64 homogeneous points, like the reference binding."""
        n = self.size()
        xyz = np.empty((n, 3), np.float64)
        check(load().sga_cloud_download_f64(self.ctx.h, self.h, _dp(xyz), None, None))  # device record + origin, added in double
        return np.concatenate([xyz, np.ones((n, 1))], axis=1)

    def xyz64(self):
        n = self.size()
        xyz = np.empty((n, 3), np.float64)
        check(load().sga_cloud_download_f64(self.ctx.h, self.h, _dp(xyz), None, None))
        return xyz

    def xyz(self):
        n = self.size()
        xyz = np.empty((n, 3), np.float32)
        check(load().sga_cloud_download(self.ctx.h, self.h, _fp(xyz), None, None))
        return xyz

    def normals(self):
        n = self.size()
        if not self._has()[0]:
            return np.zeros((n, 4))
        nr = np.empty((n, 3), np.float32)
        check(load().sga_cloud_download(self.ctx.h, self.h, None, _fp(nr), None))
        return np.concatenate([nr.astype(np.float64), np.zeros((n, 1))], axis=1)

    def covs(self):
        """(N,4,4) float64 with zero padding, like the reference binding."""
        n = self.size()
        out = np.zeros((n, 4, 4))
        if self._has()[1]:
            c6 = np.empty((n, 6), np.float32)
            check(load().sga_cloud_download(self.ctx.h, self.h, None, None, _fp(c6)))
            out[:, :3, :3] = mats_from_sym6(c6.astype(np.float64))
        return out


class KdTree:
    """Exact nearest-neighbour index over a PointCloud (small_gicp.KdTree): an implicit balanced kd-tree built on the GPU
    (sga_index_build_kdtree)."""

    def __init__(self, points, num_threads=1, _handle=None, **_ignored):
        if not isinstance(points, PointCloud):
            points = PointCloud(points)
        self.cloud = points
        self.ctx = points.ctx
        if _handle is not None:  # an index built over `points` already (build_kdtrees)
            self.h = _handle
            return
        self.h = C.c_void_p()
        check(load().sga_index_build_kdtree(self.ctx.h, points.h, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_index_destroy(self.h)
            self.h = C.c_void_p()

    def size(self):
        n = C.c_size_t()
        check(load().sga_index_size(self.h, C.byref(n)))
        return n.value

    __len__ = size

    def spacing(self):
        """The index's own length scale (geometric mean leaf diagonal; sga_index_spacing): what the pass routing measures motions in."""
        v = C.c_double()
        check(load().sga_index_spacing(self.h, C.byref(v)))
        return v.value

    def _tree(self):
        """Diagnostics (sga_debug_kd_tree): (depth D, thresholds (2^D,) float32, axes (2^D,) int32 — entry 2^d + k is node k of depth d,
        entry 0 unused, never written —, points (n, 3) float32 in kd order and in the cloud's device frame, order (n,) int64: their original indices)."""
        lib, depth = load(), C.c_int()
        check(lib.sga_debug_kd_tree(self.ctx.h, self.h, C.byref(depth), None, None))
        nodes = np.zeros((1 << depth.value, 2), np.float32)
        xyzw = np.zeros((self.size(), 4), np.float32)
        check(lib.sga_debug_kd_tree(self.ctx.h, self.h, C.byref(depth), nodes.ctypes.data_as(C.c_void_p), xyzw.ctypes.data_as(C.c_void_p)))
        return depth.value, nodes[:, 0].copy(), nodes[:, 1].view(np.int32).copy(), xyzw[:, :3].copy(), xyzw[:, 3].view(np.uint32).astype(np.int64)

    def _bbox(self):
        """Diagnostics (sga_debug_index_bbox): (lo (3,), hi (3,)) float32, the box of the points in the cloud's device frame as the build stored it."""
        lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
        check(load().sga_debug_index_bbox(self.h, _fp(lo), _fp(hi)))
        return lo, hi

    def refresh_attributes(self):
        """Pull the cloud's current normals / covariances into the index (needed when they were set after the index was built)."""
        check(load().sga_index_refresh_attributes(self.ctx.h, self.h, self.cloud.h))

    def batch_knn_search(self, pts, k, max_sq_dist=-1.0, num_threads=1):
        """kdtree.cpp:128-205: (indices (m,k) int64, squared distances (m,k) float64) — double distances like the reference's
        (sga_index_knn_f64: the search runs in fp32, the distances of the neighbours found are evaluated in double)."""
        q = np.ascontiguousarray(np.asarray(pts)[:, :3], dtype=np.float64)
        idx = np.empty((len(q), k), np.int64)
        d2 = np.empty((len(q), k), np.float64)
        check(load().sga_index_knn_f64(self.ctx.h, self.h, _dp(q), len(q), int(k), float(max_sq_dist), idx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(d2)))
        return idx, d2

    def batch_nearest_neighbor_search(self, pts, num_threads=1):
        idx, d2 = self.batch_knn_search(pts, 1)
        return idx[:, 0], d2[:, 0]

    def batch_knn_search_torch(self, queries, k, max_sq_dist=-1.0, stream=None):
        """batch_knn_search for queries in device memory (sga_index_knn_device): a (m,3) or (m,4) float32 / float64 tensor on the
        index's device -> (indices (m,k) int64, squared distances (m,k) float32) tensors; -1 / inf = none."""
        return _knn_torch(self, queries, k, max_sq_dist, stream)

    def knn_search(self, pt, k):
        idx, d2 = self.batch_knn_search(np.asarray(pt, dtype=np.float64).reshape(1, -1), k)
        return idx[0], d2[0]

    def nearest_neighbor_search(self, pt):
        idx, d2 = self.knn_search(pt, 1)
        return (1 if idx[0] >= 0 else 0), int(idx[0]), float(d2[0])

    def radius_search(self, queries, radius, return_lists=True, capacity=None):
        """The points of the indexed cloud within radius of every query (sga_index_radius_search): record j is a
        neighbour of query q iff d2(q, j) <= radius * radius, in double from the fp32 records.  queries: a PointCloud of the tree's
        context (the indexed cloud itself is one) or an (M,3|4) array (uploaded first).  Returns counts (M,) int64 — and, with
        return_lists, CSR lists: offsets (M + 1,) int64, indices (total,) int64 (positions in the indexed cloud) and sq_dists (total,)
        float64, in the walk's order within a list.  capacity: the room of the lists in entries for the first call (None: the counts
        are taken first); the call is repeated with room for the total when they do not fit."""
        q = queries if isinstance(queries, PointCloud) else PointCloud(queries, ctx=self.ctx)
        m = q.size()
        _i64 = C.POINTER(C.c_int64)
        counts = np.zeros(m, np.int64)
        res = _lib.RadiusResult()
        lib = load()
        if not return_lists:
            check(lib.sga_index_radius_search(self.ctx.h, self.h, q.h, float(radius), 0, counts.ctypes.data_as(_i64), None, None, None, C.byref(res)))
            return counts
        offsets = np.zeros(m + 1, np.int64)
        if capacity is None:
            check(lib.sga_index_radius_search(self.ctx.h, self.h, q.h, float(radius), 0, counts.ctypes.data_as(_i64), None, None, None, C.byref(res)))
            capacity = int(res.total)
        while True:
            indices, sq = np.empty(max(1, int(capacity)), np.int64), np.empty(max(1, int(capacity)), np.float64)
            check(lib.sga_index_radius_search(self.ctx.h, self.h, q.h, float(radius), int(capacity), counts.ctypes.data_as(_i64), offsets.ctypes.data_as(_i64), indices.ctypes.data_as(_i64), _dp(sq), C.byref(res)))
            if not res.overflow:
                return counts, offsets, indices[: int(res.total)].copy(), sq[: int(res.total)].copy()
            capacity = int(res.total)


class ProjectiveSearch:
    """ProjectiveSearch<PointCloud>(width, height, points) (ann/projective_search.hpp:158-183): the equirectangular index image of the
    points (y down, z forward), searched over a window of (2 h + 1) x (2 v + 1) pixels around the query's pixel (sga_index_build_projective).
    border_h / border_v: "repeat" (BorderRepeat, wraps once) or "clamp" (BorderClamp, out-of-range pixels skipped).  A target for
    Problem / align like a KdTree; indices are the cloud's own."""

    _BORDERS = {"repeat": 1, "clamp": 0}

    def __init__(self, points, width, height, search_window_h=10, search_window_v=5, border_h="repeat", border_v="clamp"):
        if not isinstance(points, PointCloud):
            points = PointCloud(points)
        if border_h not in self._BORDERS or border_v not in self._BORDERS:
            raise ValueError("border modes are 'repeat' or 'clamp'")
        self.cloud = points
        self.ctx = points.ctx
        self.width, self.height = int(width), int(height)
        self.h = C.c_void_p()
        check(load().sga_index_build_projective(self.ctx.h, points.h, self.width, self.height, C.byref(self.h)))
        self.set_search_window(search_window_h, search_window_v)
        self.set_border_modes(border_h, border_v)

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_index_destroy(self.h)
            self.h = C.c_void_p()

    def set_search_window(self, h, v):
        check(load().sga_projective_set_search_window(self.h, int(h), int(v)))
        self.search_window_h, self.search_window_v = int(h), int(v)

    def set_border_modes(self, border_h, border_v):
        check(load().sga_projective_set_border_modes(self.h, self._BORDERS[border_h], self._BORDERS[border_v]))
        self.border_h, self.border_v = border_h, border_v

    def size(self):
        n = C.c_size_t()
        check(load().sga_index_size(self.h, C.byref(n)))
        return n.value

    __len__ = size

    def origin(self):
        o = np.empty(3)
        check(load().sga_index_origin(self.h, _dp(o)))
        return o

    def index_map(self):
        """index_map (projective_search.hpp:152): (height, width) uint32, [v][u] = the point owning pixel (u, v), 0xFFFFFFFF = none."""
        out = np.empty((self.height, self.width), np.uint32)
        check(load().sga_projective_download_map(self.ctx.h, self.h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def refresh_attributes(self):
        """Pull the cloud's current normals / covariances into the index (needed when they were set after the index was built)."""
        check(load().sga_index_refresh_attributes(self.ctx.h, self.h, self.cloud.h))

    def batch_knn_search(self, pts, k, max_sq_dist=-1.0, num_threads=1):
        """(indices (m,k) int64, squared distances (m,k) float64): the reference's scan with double distances (sga_index_knn_f64); -1 / inf = none."""
        q = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, np.shape(pts)[-1])[:, :3])
        idx = np.empty((len(q), k), np.int64)
        d2 = np.empty((len(q), k), np.float64)
        check(load().sga_index_knn_f64(self.ctx.h, self.h, _dp(q), len(q), int(k), float(max_sq_dist), idx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(d2)))
        return idx, d2

    def batch_nearest_neighbor_search(self, pts, num_threads=1):
        idx, d2 = self.batch_knn_search(pts, 1)
        return idx[:, 0], d2[:, 0]

    def knn_search(self, pt, k):
        idx, d2 = self.batch_knn_search(np.asarray(pt, dtype=np.float64).reshape(1, -1), k)
        return idx[0], d2[0]

    def nearest_neighbor_search(self, pt):
        idx, d2 = self.knn_search(pt, 1)
        return (1 if idx[0] >= 0 else 0), int(idx[0]), float(d2[0])


class GaussianVoxelMap:
    """small_gicp.GaussianVoxelMap (src/python/voxelmap.cpp:20-140): `GaussianVoxelMap(leaf_size)`, then any number of
    `insert(cloud_with_covs, T)`; `set_lru(horizon, clear_cycle)`; `size()`, `voxel_points()`, `voxel_covs()`.
    Device side: the incremental map of csrc/voxelmap.hip."""

    def __init__(self, leaf_size, ctx=None):
        self.leaf = float(leaf_size)
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        check(load().sga_voxelmap_create(self.ctx.h, self.leaf, C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_index_destroy(self.h)
            self.h = C.c_void_p()

    @classmethod
    def from_voxels(cls, leaf_size, coords, means, cov6, ctx=None):
        """A map from voxels that exist on the host in the reference's flat order (sga_index_create_voxelmap_from_voxels: what
        ParallelReductionHIP uploads for a GaussianVoxelMap target).  A search target only: insert() needs the running sums."""
        self = cls.__new__(cls)
        self.leaf = float(leaf_size)
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        coords = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3)
        means = np.ascontiguousarray(means, dtype=np.float64).reshape(-1, 3)
        cov6 = np.ascontiguousarray(cov6, dtype=np.float64).reshape(-1, 6)
        if not (len(coords) == len(means) == len(cov6)):
            raise ValueError("coords, means and cov6 must have one row per voxel")
        check(load().sga_index_create_voxelmap_from_voxels(self.ctx.h, self.leaf, coords.ctypes.data_as(C.c_void_p), _dp(means), _dp(cov6), len(coords), C.byref(self.h)))
        return self

    @classmethod
    def _adopt(cls, leaf_size, ctx, handle):
        self = cls.__new__(cls)
        self.leaf = float(leaf_size)
        self.ctx = ctx
        self.h = handle
        return self

    @classmethod
    def from_cloud(cls, cloud, leaf_size):
        """The one-shot map of a cloud with covariances (sga_index_build_gaussian_voxelmap: create_gaussian_voxelmap's target, voxel ids
        in first-insertion order), on the cloud's context.  A search target only: insert() reports the library's refusal."""
        if not isinstance(cloud, PointCloud):
            raise TypeError("from_cloud takes a PointCloud")
        h = C.c_void_p()
        check(load().sga_index_build_gaussian_voxelmap(cloud.ctx.h, cloud.h, float(leaf_size), C.byref(h)))
        return cls._adopt(leaf_size, cloud.ctx, h)

    def insert(self, cloud, T=None):
        t16 = None if T is None else _T16(T)
        check(load().sga_voxelmap_insert(self.ctx.h, self.h, cloud.h, None if t16 is None else _dp(t16)))

    def set_lru(self, horizon=100, clear_cycle=10):
        check(load().sga_voxelmap_set_lru(self.h, int(horizon), int(clear_cycle)))

    def set_search_offsets(self, num_offsets):
        """incremental_voxelmap.hpp:157-186: 1 (the query's own voxel), 7 or 27 voxels offer their Gaussians, the nearest mean wins."""
        check(load().sga_voxelmap_set_search_offsets(self.h, int(num_offsets)))

    def batch_knn_search(self, pts, k, max_sq_dist=-1.0):
        return _voxelmap_knn(self, pts, k, max_sq_dist)

    def batch_knn_search_torch(self, queries, k, max_sq_dist=-1.0, stream=None):
        """batch_knn_search for queries in device memory (sga_index_knn_device): a (m,3) or (m,4) float32 / float64 tensor on the
        index's device -> (indices (m,k) int64, squared distances (m,k) float32) tensors; -1 / inf = none."""
        return _knn_torch(self, queries, k, max_sq_dist, stream)

    def knn_search(self, pt, k):
        idx, d2 = _voxelmap_knn(self, np.asarray(pt, dtype=np.float64).reshape(1, -1), k)
        return idx[0], d2[0]

    def __len__(self):
        return self.size()

    def size(self):
        if not self.h.value:
            return 0
        n = C.c_size_t()
        check(load().sga_index_size(self.h, C.byref(n)))
        return n.value

    def download(self):
        n = self.size()
        coords = np.empty((n, 3), np.int32)
        means = np.empty((n, 3), np.float32)
        c6 = np.empty((n, 6), np.float32)
        counts = np.empty(n, np.uint32)
        check(load().sga_index_voxelmap_download(self.ctx.h, self.h, coords.ctypes.data_as(C.POINTER(C.c_int32)), _fp(means), _fp(c6), counts.ctypes.data_as(C.POINTER(C.c_uint32))))
        return coords, means, c6, counts

    def voxel_points(self):
        m = self.download()[1].astype(np.float64)
        return np.concatenate([m, np.ones((len(m), 1))], axis=1)

    def voxel_covs(self):
        c6 = self.download()[2].astype(np.float64)
        out = np.zeros((len(c6), 4, 4))
        out[:, :3, :3] = mats_from_sym6(c6)
        return out


class _FlatVoxelMap:
    """IncrementalVoxelMap<FlatContainer<HasNormals, HasCovs>> (ann/flat_container.hpp:18-58; src/python/voxelmap.cpp:146-151): voxels keep
    up to `max_num_points_in_cell` of the inserted points and, where the kind keeps them, the normals R n and covariances R C R^T of the
    points they keep.  `insert(cloud, T)` (the cloud needs exactly the attributes the map keeps), `set_lru`, `set_setting`,
    `set_search_offsets(1 | 7 | 27)`, `size()` / `len()`, `voxel_points()`, `knn_search` / `batch_knn_search`, `download()`, `from_voxels`.
    Targets: ICP for every kind, PLANE_ICP where the map keeps normals, GICP where it keeps covariances."""

    FLAT_CAP = 16
    CONTENTS = 0  # _lib.FLAT_NORMALS | _lib.FLAT_COVS bits

    def __init__(self, leaf_size, ctx=None):
        self.leaf = float(leaf_size)
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        self.contents = self.CONTENTS
        check(load().sga_flatmap_create_contents(self.ctx.h, self.leaf, int(self.CONTENTS), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_index_destroy(self.h)
            self.h = C.c_void_p()

    def insert(self, cloud, T=None):
        t16 = None if T is None else _T16(T)
        check(load().sga_voxelmap_insert(self.ctx.h, self.h, cloud.h, None if t16 is None else _dp(t16)))

    def set_lru(self, horizon=100, clear_cycle=10):
        check(load().sga_voxelmap_set_lru(self.h, int(horizon), int(clear_cycle)))

    def batch_knn_search(self, pts, k, max_sq_dist=-1.0):
        return _voxelmap_knn(self, pts, k, max_sq_dist)

    def batch_knn_search_torch(self, queries, k, max_sq_dist=-1.0, stream=None):
        """batch_knn_search for queries in device memory (sga_index_knn_device): a (m,3) or (m,4) float32 / float64 tensor on the
        index's device -> (indices (m,k) int64, squared distances (m,k) float32) tensors; -1 / inf = none."""
        return _knn_torch(self, queries, k, max_sq_dist, stream)

    def knn_search(self, pt, k):
        idx, d2 = _voxelmap_knn(self, np.asarray(pt, dtype=np.float64).reshape(1, -1), k)
        return idx[0], d2[0]

    @classmethod
    def _from_voxels(cls, leaf_size, coords, counts, points, normals, cov6, search_offsets, ctx):
        self = cls.__new__(cls)
        self.leaf = float(leaf_size)
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        coords = np.ascontiguousarray(coords, dtype=np.int32).reshape(-1, 3)
        counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1)
        points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        n = len(coords)
        if len(counts) != n or int(counts.sum()) != len(points) or (n and counts.max() > cls.FLAT_CAP):
            raise ValueError("counts must have one entry per voxel (<= %d) and sum to the number of points" % cls.FLAT_CAP)
        valid = np.arange(cls.FLAT_CAP)[None, :] < counts[:, None]

        def slots(a, width):
            if a is None:
                return None
            out = np.zeros((n, cls.FLAT_CAP, width))
            out[valid] = np.asarray(a, dtype=np.float64).reshape(-1, np.asarray(a).shape[-1])[:, :width]
            return out

        p16, n16, c16 = slots(points, 3), slots(normals, 3), slots(cov6, 6)
        self.contents = (_lib.FLAT_NORMALS if n16 is not None else 0) | (_lib.FLAT_COVS if c16 is not None else 0)
        check(load().sga_index_create_flatmap_from_voxels_contents(self.ctx.h, self.leaf, coords.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p), _dp(p16), None if n16 is None else _dp(n16),
                                                                   None if c16 is None else _dp(c16), int(search_offsets), n, C.byref(self.h)))
        return self

    @classmethod
    def from_voxels(cls, leaf_size, coords, counts, points, cov6=None, search_offsets=1, ctx=None, normals=None):
        """A map from voxels that exist on the host in the reference's flat order (sga_index_create_flatmap_from_voxels_contents: what
        ParallelReductionHIP uploads for an IncrementalVoxelMap<FlatContainer*> target): coords (V, 3), counts (V,), points (P, 3), normals
        (P, 3 or 4) and cov6 (P, 6) with the points of voxel 0 first, then voxel 1, ... like download().  The map keeps what is given.  A
        search target only."""
        return cls._from_voxels(leaf_size, coords, counts, points, normals, cov6, search_offsets, ctx)

    def set_setting(self, min_sq_dist_in_cell=0.01, max_num_points_in_cell=10):
        check(load().sga_flatmap_set_setting(self.h, float(min_sq_dist_in_cell), int(max_num_points_in_cell)))

    def set_search_offsets(self, num_offsets):
        check(load().sga_voxelmap_set_search_offsets(self.h, int(num_offsets)))

    def size(self):
        n = C.c_size_t()
        check(load().sga_index_size(self.h, C.byref(n)))
        return n.value

    __len__ = size

    def _download(self, normals, covs):
        n = self.size()
        coords = np.empty((n, 3), np.int32)
        counts = np.empty(n, np.uint32)
        pts = np.empty((n, self.FLAT_CAP, 3), np.float32)
        nr = np.empty((n, self.FLAT_CAP, 3), np.float32) if normals else None
        c6 = np.empty((n, self.FLAT_CAP, 6), np.float32) if covs else None
        check(load().sga_flatmap_download_contents(self.ctx.h, self.h, coords.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(pts), None if nr is None else _fp(nr),
                                                   None if c6 is None else _fp(c6)))
        valid = np.arange(self.FLAT_CAP)[None, :] < counts[:, None]
        return coords, counts, pts[valid], None if nr is None else nr[valid], None if c6 is None else c6[valid]

    def download(self):
        """coords (V,3), counts (V,), points (P,3), then normals (P,3) and cov6 (P,6) where the map keeps them: the points of voxel 0 first,
        then voxel 1, ... (P = sum of counts)."""
        coords, counts, pts, nr, c6 = self._download(self.contents & _lib.FLAT_NORMALS, self.contents & _lib.FLAT_COVS)
        return (coords, counts, pts) + tuple(a for a in (nr, c6) if a is not None)

    def voxel_points(self):
        p = self._download(False, False)[2].astype(np.float64)
        return np.concatenate([p, np.ones((len(p), 1))], axis=1)

    def _voxel_normals(self):
        nr = self._download(True, False)[3].astype(np.float64)
        return np.concatenate([nr, np.zeros((len(nr), 1))], axis=1)

    def _voxel_covs(self):
        c6 = self._download(False, True)[4].astype(np.float64)
        out = np.zeros((len(c6), 4, 4))
        out[:, :3, :3] = mats_from_sym6(c6)
        return out


class IncrementalVoxelMap(_FlatVoxelMap):
    """small_gicp.IncrementalVoxelMap = IncrementalVoxelMap<FlatContainerPoints>: points only, the plain scan-to-model ICP target."""

    CONTENTS = 0


class IncrementalVoxelMapNormal(_FlatVoxelMap):
    """small_gicp.IncrementalVoxelMapNormal = IncrementalVoxelMap<FlatContainerNormal>: points with normals, the scan-to-model
    point-to-plane target (Faster-LIO's linear iVox).  `voxel_normals()`: P x 4, w = 0."""

    CONTENTS = _lib.FLAT_NORMALS

    def voxel_normals(self):
        return self._voxel_normals()


class IncrementalVoxelMapNormalCov(_FlatVoxelMap):
    """small_gicp.IncrementalVoxelMapNormalCov = IncrementalVoxelMap<FlatContainerNormalCov>: points with normals and covariances."""

    CONTENTS = _lib.FLAT_NORMALS | _lib.FLAT_COVS

    def voxel_normals(self):
        return self._voxel_normals()

    def voxel_covs(self):
        return self._voxel_covs()


class IncrementalVoxelMapCov(_FlatVoxelMap):
    """small_gicp.IncrementalVoxelMapCov (src/python/voxelmap.cpp:110-140) = IncrementalVoxelMap<FlatContainerCov>: voxels keep up
    to `max_num_points_in_cell` of the inserted points (with covariances); the scan-to-model GICP target.  `insert(cloud, T)`,
    `set_lru`, `set_search_offsets(1 | 7 | 27)`, `size()`, `voxel_points()`, `voxel_covs()`."""

    CONTENTS = _lib.FLAT_COVS

    @classmethod
    def from_voxels(cls, leaf_size, coords, counts, points, cov6=None, search_offsets=1, ctx=None):
        """A map from voxels that exist on the host in the reference's flat order (sga_index_create_flatmap_from_voxels: what
        ParallelReductionHIP uploads for an IncrementalVoxelMap<FlatContainer*> target): coords (V, 3), counts (V,), points (P, 3) and
        cov6 (P, 6) with the points of voxel 0 first, then voxel 1, ... like download().  A search target only."""
        return cls._from_voxels(leaf_size, coords, counts, points, None, cov6, search_offsets, ctx)

    def download(self):
        """coords (V,3), counts (V,), points (P,3), cov6 (P,6): the points of voxel 0 first, then voxel 1, ... (P = sum of counts)."""
        n = self.size()
        coords = np.empty((n, 3), np.int32)
        counts = np.empty(n, np.uint32)
        pts = np.empty((n, self.FLAT_CAP, 3), np.float32)
        c6 = np.empty((n, self.FLAT_CAP, 6), np.float32)
        check(load().sga_flatmap_download(self.ctx.h, self.h, coords.ctypes.data_as(C.POINTER(C.c_int32)), counts.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(pts), _fp(c6)))
        valid = np.arange(self.FLAT_CAP)[None, :] < counts[:, None]
        return coords, counts, pts[valid], c6[valid]

    def voxel_covs(self):
        c6 = self.download()[3].astype(np.float64)
        out = np.zeros((len(c6), 4, 4))
        out[:, :3, :3] = mats_from_sym6(c6)
        return out


class RegistrationResult:
    """registration_result.hpp:11-30, field for field."""

    def __init__(self, rc=None):
        if rc is None:
            self.T_target_source = np.eye(4)
            self.converged, self.iterations, self.num_inliers = False, 0, 0
            self.H, self.b, self.error = np.zeros((6, 6)), np.zeros(6), 0.0
        else:
            self.T_target_source = np.array(rc.T_target_source).reshape(4, 4).T.copy()
            self.converged = bool(rc.converged)
            self.iterations = int(rc.iterations)
            self.num_inliers = int(rc.num_inliers)
            self.H = np.array(rc.H).reshape(6, 6)
            self.b = np.array(rc.b)
            self.error = float(rc.error)

    def __repr__(self):
        return f"RegistrationResult(converged={self.converged}, iterations={self.iterations}, num_inliers={self.num_inliers}, error={self.error:.6g})"


def make_setting(
    registration_type="GICP",
    max_correspondence_distance=1.0,
    max_iterations=20,
    rotation_eps=0.1 * np.pi / 180.0,
    translation_eps=1e-3,
    robust_kernel=None,
    robust_c=1.0,
    optimizer="LM",
    math_mode="fp32",
    verbose=False,
    max_inner_iterations=10,
    init_lambda=1e-3,
    lambda_factor=10.0,
    gn_lambda=1e-6,
    restrict_dof_lambda=0.0,
    restrict_dof_mask=None,
):
    s = RegistrationSettingC()
    load().sga_registration_setting_default(C.byref(s))
    s.factor.factor_kind = _FACTOR_BY_NAME[registration_type] if isinstance(registration_type, str) else int(registration_type)
    # None: no rejector (NullRejector, rejector.hpp:11-16).  Any number, negative ones included, is squared like the reference does
    # (registration_helper.cpp:90,100,110; src/python/align.cpp:246): DistanceRejector with max_dist_sq = d * d
    s.factor.max_dist_sq = -1.0 if max_correspondence_distance is None else float(max_correspondence_distance) ** 2
    s.factor.robust_kind = {None: 0, "NONE": 0, "HUBER": 1, "CAUCHY": 2}[robust_kernel if robust_kernel is None else robust_kernel.upper()]
    s.factor.robust_c = float(robust_c)
    s.factor.math_mode = {"fp32": 0, "fp64": 1}[math_mode]
    s.optimizer = {"LM": 0, "GN": 1}[optimizer]
    s.max_iterations = int(max_iterations)
    s.max_inner_iterations = int(max_inner_iterations)
    s.init_lambda, s.lambda_factor, s.gn_lambda = float(init_lambda), float(lambda_factor), float(gn_lambda)
    s.rotation_eps, s.translation_eps = float(rotation_eps), float(translation_eps)
    s.verbose = int(verbose)
    s.restrict_dof_lambda = float(restrict_dof_lambda)
    if restrict_dof_mask is not None:
        for i in range(6):
            s.restrict_dof_mask[i] = float(restrict_dof_mask[i])
    return s


class Problem:
    """(target index, source cloud) pairing with device-resident factor state: the Reduction slot of Registration<>."""

    def __init__(self, target, source, init_T=None, ctx=None, _handle=None):
        self.target, self.source = target, source
        self.ctx = ctx or source.ctx  # a problem may run on another context (stream) of the same device than the one that built its inputs
        self.h = C.c_void_p()
        if _handle is not None:  # a problem made by create_problems: adopted as it is
            self.h = _handle
            return
        t16 = _T16(init_T)
        if isinstance(source, (KdTree, ProjectiveSearch)):  # the source by its own index: its kd order is taken as it is (no sort; a projective search is refused)
            check(load().sga_problem_create_from_index(self.ctx.h, target.h, source.h, _dp(t16), C.byref(self.h)))
        else:
            check(load().sga_problem_create(self.ctx.h, target.h, source.h, _dp(t16), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_problem_destroy(self.h)
            self.h = C.c_void_p()

    def linearize(self, factor_params, T):
        H, b = np.empty(36), np.empty(6)
        e, ninl = C.c_double(), C.c_uint64()
        t16 = _T16(T)
        check(load().sga_linearize(self.ctx.h, self.h, C.byref(factor_params), _dp(t16), _dp(H), _dp(b), C.byref(e), C.byref(ninl)))
        return H.reshape(6, 6), b, e.value, ninl.value

    def error(self, factor_params, T):
        e = C.c_double()
        t16 = _T16(T)
        check(load().sga_error(self.ctx.h, self.h, C.byref(factor_params), _dp(t16), C.byref(e)))
        return e.value

    def linearize_async(self, factor_params, T, d_out_ptr):
        t16 = _T16(T)
        check(load().sga_linearize_async(self.ctx.h, self.h, C.byref(factor_params), _dp(t16), C.c_void_p(int(d_out_ptr))))

    def error_async(self, factor_params, T, d_out_ptr):
        t16 = _T16(T)
        check(load().sga_error_async(self.ctx.h, self.h, C.byref(factor_params), _dp(t16), C.c_void_p(int(d_out_ptr))))

    def set_rejector(self, fn):
        """A custom CorrespondenceRejector (rejector.hpp:11-28) as a batch callback: fn(T 4x4, target_index (n,) int64, sq_dist (n,)
        float32) -> boolean array, True = reject.  None restores the built-in distance rejector."""
        if fn is None:
            self._rejector_cb = _lib.REJECTOR_FN()  # NULL function pointer
        else:
            def cb(_user, T16, n, idx_p, d2_p, rej_p):
                try:
                    T = np.ctypeslib.as_array(T16, (16,)).reshape(4, 4).T.copy()
                    idx = np.ctypeslib.as_array(idx_p, (n,))
                    d2 = np.ctypeslib.as_array(d2_p, (n,))
                    out = np.ctypeslib.as_array(rej_p, (n,))
                    out[:] = np.asarray(fn(T, idx, d2), dtype=bool)
                    return 0
                except Exception:  # noqa: BLE001
                    import traceback

                    traceback.print_exc()
                    return 1

            self._rejector_cb = _lib.REJECTOR_FN(cb)
        check(load().sga_problem_set_rejector(self.h, self._rejector_cb, None))

    def linearize_per_point(self, factor_params, T):
        """sga_linearize_per_point: (inlier (n,) bool, H (n,6,6), b (n,6), e (n,)) for every source point in the caller's order."""
        n = self.source.size()
        vals = np.zeros((n, 28))
        ok = np.zeros(n, np.uint8)
        t16 = _T16(T)
        check(load().sga_linearize_per_point(self.ctx.h, self.h, C.byref(factor_params), _dp(t16), _dp(vals), ok.ctypes.data_as(C.POINTER(C.c_ubyte))))
        H = np.zeros((n, 6, 6))
        iu = np.triu_indices(6)
        H[:, iu[0], iu[1]] = vals[:, :21]
        H[:, iu[1], iu[0]] = vals[:, :21]
        return ok.astype(bool), H, vals[:, 21:27].copy(), vals[:, 27].copy()

    def factors(self):
        n = self.source.size()
        ti = np.empty(n, np.int64)
        m6 = np.empty((n, 6), np.float32)
        check(load().sga_problem_get_factors(self.ctx.h, self.h, ti.ctypes.data_as(C.POINTER(C.c_int64)), _fp(m6)))
        return ti, m6

    def factors_torch(self, stream=None):
        """factors() as tensors on the problem's device (sga_problem_get_factors_device): (target_index (n,) int64, mahalanobis6 (n,6) float32)."""
        return _factors_torch(self, stream)

    ROUTES = ("factors", "grid", "certify", "fused_lane", "fused_queue", "queue", "lane")  # enum class Route (csrc/linearize.hip)

    def last_plan(self):
        """Diagnostics (sga_problem_get_last_plan): the plan of the last linearization pass — its route by name, warm, grid, points per
        lane, tail, chunk_tiles, and the rows and workgroups of the row reduction (0 when the factor kernel summed the rows itself)."""
        out = (C.c_int * 8)()
        check(load().sga_problem_get_last_plan(self.h, out))
        v = list(out)
        return {"route": self.ROUTES[v[0]], "warm": bool(v[1]), "grid": bool(v[2]), "pts": v[3], "tail": bool(v[4]), "chunk_tiles": v[5], "reduce_rows": v[6], "reduce_groups": v[7]}

    def align(self, setting, init_T=None):
        res = ResultC()
        t16 = _T16(init_T)
        check(load().sga_align_problem(self.ctx.h, self.h, _dp(t16), C.byref(setting), C.byref(res)))
        return RegistrationResult(res)

    def search_stats(self, enable=None):
        """Diagnostics: enable / disable the per-point record of leaves scanned, or (enable=None) fetch the last pass's counts."""
        if enable is not None:
            check(load().sga_problem_set_search_stats(self.ctx.h, self.h, 1 if enable else 0))
            return None
        out = np.zeros(len(self.source), dtype=np.int32)
        check(load().sga_problem_get_search_stats(self.ctx.h, self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def sorted_points(self):
        """Diagnostics: the source points in the engine's order (n x 4 float32; the 4th column holds the original index as bits)."""
        out = np.zeros((len(self.source), 4), dtype=np.float32)
        check(load().sga_problem_get_sorted_points(self.ctx.h, self.h, out.ctypes.data_as(C.c_void_p)))
        return out

    def pass_stats(self):
        """Linearization passes since creation by kind (cold = full search, warm = certified neighbours) and the source points
        the warm passes had to search again."""
        c, w, f = C.c_uint64(), C.c_uint64(), C.c_uint64()
        check(load().sga_problem_get_pass_stats(self.ctx.h, self.h, C.byref(c), C.byref(w), C.byref(f)))
        g = (C.c_uint64 * 6)()
        check(load().sga_problem_get_grid_stats(self.h, g))
        return {"cold_passes": c.value, "warm_passes": w.value, "walked_points": f.value, "grid_passes": g[0], "grid_open": g[1], "grid_rings": g[2], "grid_cell_m": g[3] * 1e-6,
                "adj_queries": g[4], "adj_unsettled": g[5]}


def _T16s(Ts, count):
    """count poses (None: identities) as a contiguous (count, 16) array, each column-major"""
    if Ts is None:
        Ts = [None] * count
    if len(Ts) != count:
        raise ValueError(f"{len(Ts)} poses for {count} pairs")
    return np.ascontiguousarray(np.stack([_T16(T) for T in Ts]).reshape(count, 16)) if count else np.zeros((0, 16))


class BatchProblem:
    """sga_batch: several independent Problems of ONE context linearized by one search + factor launch, one row reduction and one
    hand-off to the host per round, each pair at its own pose (small_gicp_amd.h).  The targets are all KdTrees, all GaussianVoxelMaps
    (VGICP) or all flat maps (IncrementalVoxelMap*; any leaf sizes, search offsets and contents, a map may serve several problems) — a
    mix of kinds is refused; ICP, PLANE_ICP or GICP (against maps as Problem takes them) in fp32 arithmetic, no robust kernel, no host
    rejector.  The problems are borrowed: after a call each holds what a lone pass leaves."""

    def __init__(self, problems):
        self.problems = list(problems)  # (keeps them alive: the batch must go first)
        self.ctx = self.problems[0].ctx if self.problems else default_context()
        hs = (C.c_void_p * max(1, len(self.problems)))(*[p.h.value for p in self.problems])
        self.h = C.c_void_p()
        check(load().sga_batch_create(self.ctx.h, hs, len(self.problems), C.byref(self.h)))

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __len__(self):
        return len(self.problems)

    def linearize(self, factor_params, Ts, active=None, out=None):
        """Reduction::linearize for every active pair: (H (B, 6, 6), b (B, 6), e (B,), num_inliers (B,)).  Entries of inactive pairs keep
        what `out` (a tuple of such arrays) held, zeros without it."""
        B = len(self.problems)
        H, b, e, n = out if out is not None else (np.zeros((B, 6, 6)), np.zeros((B, 6)), np.zeros(B), np.zeros(B, np.uint64))
        t = _T16s(Ts, B)
        act = None if active is None else np.ascontiguousarray(np.asarray(active, dtype=bool).astype(np.uint8))
        if act is not None and len(act) != B:
            raise ValueError(f"{len(act)} flags for {B} pairs")
        check(load().sga_batch_linearize(self.ctx.h, self.h, C.byref(factor_params), _dp(t), None if act is None else act.ctypes.data_as(C.POINTER(C.c_ubyte)), _dp(H), _dp(b), _dp(e), n.ctypes.data_as(C.POINTER(C.c_uint64))))
        return H, b, e, n

    def align(self, setting, init_Ts=None):
        """Registration<>::align for every pair in lock-step rounds -> [RegistrationResult] in the problems' order."""
        B = len(self.problems)
        res = (ResultC * max(1, B))()
        t = _T16s(init_Ts, B)
        check(load().sga_align_batch(self.ctx.h, self.h, _dp(t) if B else None, C.byref(setting), res))
        return [RegistrationResult(res[k]) for k in range(B)]


def _problem_members(targets, sources, ctx):
    targets, sources = list(targets), list(sources)
    if len(targets) != len(sources):
        raise ValueError(f"{len(targets)} targets for {len(sources)} sources")
    for t in targets:
        if not isinstance(t, (KdTree, ProjectiveSearch, GaussianVoxelMap, _FlatVoxelMap)):
            raise TypeError("create_problems takes KdTree / ProjectiveSearch / GaussianVoxelMap / IncrementalVoxelMap* targets")
    for s in sources:
        if not isinstance(s, PointCloud):
            raise TypeError("create_problems takes PointCloud sources (a KdTree source: Problem(target, tree))")
    ctx = ctx or (sources[0].ctx if sources else default_context())
    ts = (C.c_void_p * max(1, len(targets)))(*[t.h.value for t in targets])
    ss = (C.c_void_p * max(1, len(sources)))(*[s.h.value for s in sources])
    return targets, sources, ctx, ts, ss


def create_problems(targets, sources, init_Ts=None, ctx=None):
    """sga_problem_create_batch: [Problem(targets[k], sources[k], init_Ts[k], ctx) for all k] (init_Ts None: identities) by one chain of
    launches — one table copy, one keys launch, one stable sort, one gather / state / bounding-box launch — and one host wait, whatever
    the number of pairs.  Every problem is an ordinary Problem, its source in the lone call's order bit for bit.  PointCloud sources of at
    most 262144 points against KdTree, GaussianVoxelMap or IncrementalVoxelMap* targets share the chain; larger clouds, projective
    targets and empty sources are paired one by one inside the call.  ctx: the context the problems run on (default: the first source's)."""
    targets, sources, ctx, ts, ss = _problem_members(targets, sources, ctx)
    t16 = None if init_Ts is None else _T16s(init_Ts, len(targets))
    out = (C.c_void_p * max(1, len(targets)))()
    check(load().sga_problem_create_batch(ctx.h, ts, ss, None if t16 is None else _dp(t16), len(targets), out))
    return [Problem(t, s, ctx=ctx, _handle=C.c_void_p(out[k])) for k, (t, s) in enumerate(zip(targets, sources))]


def _problem_batch_plan(targets, sources):
    """Diagnostics (sga_debug_problem_batch_plan): what create_problems(targets, sources) would do — forest (members of the shared chain),
    lone (members through the lone routine), empty (members with an empty source), points of the concatenation."""
    targets, _, _, ts, ss = _problem_members(targets, sources, None)
    out = (C.c_int * 4)()
    check(load().sga_debug_problem_batch_plan(ts, ss, len(targets), out))
    return {"forest": out[0], "lone": out[1], "empty": out[2], "points": out[3]}


def problem_batch_launches():
    """Diagnostics (sga_debug_problem_batch_launches): the table copies, kernels and sort calls enqueued so far by the shared chain of
    create_problems."""
    v = C.c_ulonglong()
    check(load().sga_debug_problem_batch_launches(C.byref(v)))
    return v.value


def align_batch(targets, sources, init_Ts=None, setting=None):
    """Register sources[k] (a PointCloud, or a KdTree taken in its own order) against targets[k] for all k in one batch; the targets are
    all KdTrees, all GaussianVoxelMaps or all flat maps (IncrementalVoxelMap*), and one target may appear several times.
    setting: make_setting(...) (default GICP, 1 m).  The problems live for the call only.

    VGICP, four scans against one model map:
        model = GaussianVoxelMap(1.0); model.insert(map_cloud)
        results = align_batch([model] * 4, scans, init_Ts=guesses)"""
    if len(targets) != len(sources):
        raise ValueError("as many targets as sources")
    init = [None] * len(targets) if init_Ts is None else init_Ts
    batched = len(targets) > 0 and all(isinstance(s, PointCloud) and s.ctx is sources[0].ctx for s in sources)
    if batched and all(isinstance(t, (KdTree, ProjectiveSearch, GaussianVoxelMap, _FlatVoxelMap)) for t in targets):
        problems = create_problems(targets, sources, init_Ts)  # one chain for all pairs; the same bits as the lone calls
    else:
        problems = [Problem(t, s, T) for t, s, T in zip(targets, sources, init)]
    batch = BatchProblem(problems)
    try:
        return batch.align(setting if setting is not None else make_setting("GICP"), init_Ts)
    finally:
        batch.__del__()  # before its problems


def optimize_batch(setting, init_Ts, linearize, error):
    """sga_optimize_batch: the lock-step host LM / GN over python callbacks linearize(k, T) -> (H, b, e, num_inliers) and
    error(k, T) -> e, each asked per active pair k in ascending order within a round.  -> [RegistrationResult]"""
    B = len(init_Ts)
    exc = []

    def _lin(user, count, active, T, H, b, e, n):
        try:
            for k in range(count):
                if not active[k]:
                    continue
                Tm = np.ctypeslib.as_array(T, shape=(count * 16,))[16 * k : 16 * k + 16].reshape(4, 4).T
                h, bb, ee, nn = linearize(k, Tm.copy())
                np.ctypeslib.as_array(H, shape=(count * 36,))[36 * k : 36 * k + 36] = np.asarray(h, dtype=np.float64).reshape(36)
                np.ctypeslib.as_array(b, shape=(count * 6,))[6 * k : 6 * k + 6] = np.asarray(bb, dtype=np.float64).reshape(6)
                e[k] = float(ee)
                n[k] = int(nn)
            return 0
        except Exception as ex:  # noqa: BLE001
            exc.append(ex)
            return 1

    def _err(user, count, active, T, e):
        try:
            for k in range(count):
                if active[k]:
                    Tm = np.ctypeslib.as_array(T, shape=(count * 16,))[16 * k : 16 * k + 16].reshape(4, 4).T
                    e[k] = float(error(k, Tm.copy()))
            return 0
        except Exception as ex:  # noqa: BLE001
            exc.append(ex)
            return 1

    res = (ResultC * max(1, B))()
    t = _T16s(init_Ts, B)
    rc = load().sga_optimize_batch(C.byref(setting), B, _dp(t) if B else None, _lib.BATCH_LINEARIZE_FN(_lin), _lib.BATCH_ERROR_FN(_err), None, res)
    if exc:
        raise exc[0]
    check(rc)
    return [RegistrationResult(res[k]) for k in range(B)]


class MultiProblem:
    """sga_multi: one registration over several GPUs of this process (source sharded, target replicated; small_gicp_amd.h).  `devices`
    may name a device more than once (logical shards on one GPU).  Clouds are given as host arrays: points (n, 3), normals (n, 3) or
    None, covariances (n, 3, 3) or None."""

    def __init__(self, devices, target, source, init_T=None):
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self.h = C.c_void_p()
        check(load().sga_multi_create(devs, len(devices), C.byref(self.h)))
        tp, tn, tc = self._pack(*target)
        check(load().sga_multi_set_target_f64(self.h, _dp(tp), _dp(tn) if tn is not None else None, _dp(tc) if tc is not None else None, len(tp)))
        sp, sn, sc = self._pack(*source)
        self.n_source = len(sp)
        check(load().sga_multi_set_source_f64(self.h, _dp(sp), _dp(sn) if sn is not None else None, _dp(sc) if sc is not None else None, len(sp), _dp(_T16(np.eye(4) if init_T is None else init_T))))

    @staticmethod
    def _pack(points, normals=None, covs=None):
        p = np.ones((len(points), 4))
        p[:, :3] = np.asarray(points, dtype=np.float64)[:, :3]
        nr = cv = None
        if normals is not None:
            nr = np.zeros((len(points), 4))
            nr[:, :3] = np.asarray(normals, dtype=np.float64)[:, :3]
        if covs is not None:
            cv = np.zeros((len(points), 4, 4))
            cv[:, :3, :3] = np.asarray(covs, dtype=np.float64)[:, :3, :3]
            cv = np.ascontiguousarray(cv.transpose(0, 2, 1))  # column-major 4x4 (symmetric: the same numbers)
        return np.ascontiguousarray(p), nr, cv

    def __del__(self):
        if getattr(self, "h", None):
            load().sga_multi_destroy(self.h)
            self.h = None

    def linearize(self, factor_params, T):
        H, b, e, n = np.zeros(36), np.zeros(6), C.c_double(), C.c_uint64()
        check(load().sga_multi_linearize(self.h, C.byref(factor_params), _dp(_T16(T)), _dp(H), _dp(b), C.byref(e), C.byref(n)))
        return H.reshape(6, 6), b, e.value, n.value

    def error(self, factor_params, T):
        e = C.c_double()
        check(load().sga_multi_error(self.h, C.byref(factor_params), _dp(_T16(T)), C.byref(e)))
        return e.value

    def align(self, setting, init_T=None):
        res = ResultC()
        check(load().sga_multi_align(self.h, _dp(_T16(np.eye(4) if init_T is None else init_T)), C.byref(setting), C.byref(res)))
        return RegistrationResult(res)

    def factors(self):
        idx = np.empty(self.n_source, np.int64)
        check(load().sga_multi_get_factors(self.h, idx.ctypes.data_as(C.c_void_p), None))
        return idx


def _voxelmap_knn(vm, pts, k, max_sq_dist=-1.0):
    """traits::knn_search of a voxel map (incremental_voxelmap.hpp:127-149) for m queries: global indices (voxel_id << 32) | point_id
    (-1 = none) and squared distances ascending (inf = none), each (m, k)."""
    q = np.ascontiguousarray(np.asarray(pts, dtype=np.float64).reshape(-1, np.asarray(pts).shape[-1])[:, :3])
    idx = np.empty((len(q), k), np.int64)
    d2 = np.empty((len(q), k), np.float64)
    check(load().sga_index_knn_f64(vm.ctx.h, vm.h, _dp(q), len(q), int(k), float(max_sq_dist), idx.ctypes.data_as(C.POINTER(C.c_int64)), _dp(d2)))
    return idx, d2


# ---- device-resident data (sga_*_device) -----------------------------------------------------------------------
# torch is imported inside these functions only: the package itself does not need it.
_IO_DTYPES = {"float32": _lib.F32, "float64": _lib.F64}


def _device_array(ptr, dtype, cols, stride):
    a = _lib.DeviceArray()
    a.data, a.dtype, a.cols, a.stride = int(ptr), int(dtype), int(cols), int(stride)
    return a


def _torch_rows(t, what, ctx, cols_allowed):
    """A tensor of strided rows -> (sga_device_array, rows): 2-D (or (N,3,3) / (N,4,4) covariances whose matrices are contiguous),
    float32 / float64, last-dimension stride 1, any row stride, on the device of `ctx` (None: any GPU; the caller compares later).
    ValueError for anything else, before a context or the library is needed."""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what} must be a torch.Tensor")
    if t.dim() == 3:  # (N,3,3) / (N,4,4): the matrices row-major and contiguous
        if t.shape[1] != t.shape[2] or (t.shape[0] > 0 and (t.stride(2) != 1 or t.stride(1) != t.shape[2])):
            raise ValueError(f"{what}: (N,3,3) or (N,4,4) with contiguous matrices")
        cols, stride = t.shape[1] * t.shape[2], t.stride(0)
    elif t.dim() == 2:
        cols, stride = t.shape[1], t.stride(0)
        if t.shape[0] > 0 and t.stride(1) != 1:
            raise ValueError(f"{what}: the last dimension must have stride 1 (a transposed view does not)")
    else:
        raise ValueError(f"{what} must be 2-D, not {t.dim()}-D")
    name = str(t.dtype).replace("torch.", "")
    if name not in _IO_DTYPES:
        raise ValueError(f"{what} must be float32 or float64, not {t.dtype}")
    if cols not in cols_allowed:
        raise ValueError(f"{what}: {cols} columns, expected one of {sorted(cols_allowed)}")
    if t.shape[0] > 1 and stride < cols:
        raise ValueError(f"{what}: row stride {stride} < {cols} columns")
    if not t.is_cuda:
        raise ValueError(f"{what} is a CPU tensor: it must live on the context's device (host arrays: PointCloud(points))")
    if ctx is not None and t.device.index != int(ctx.device):
        raise ValueError(f"{what} lives on {t.device}, the context on cuda:{ctx.device}")
    return _device_array(t.data_ptr(), _IO_DTYPES[name], cols, stride if t.shape[0] > 1 else cols), t.shape[0]


def _torch_times(t, n, ctx):
    """A tensor of n times -> sga_device_array: 1-D (or (N,1)), float32 / float64, any stride, on the context's device"""
    import torch

    if not isinstance(t, torch.Tensor):
        raise ValueError("times must be a numpy array or a torch.Tensor")
    if t.dim() == 2 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() != 1 or t.shape[0] != n:
        raise ValueError(f"times of shape {tuple(t.shape)} for a cloud of {n} points")
    name = str(t.dtype).replace("torch.", "")
    if name not in _IO_DTYPES:
        raise ValueError(f"times must be float32 or float64, not {t.dtype}")
    if n > 1 and t.stride(0) < 1:
        raise ValueError(f"times: stride {t.stride(0)} (an expanded or reversed view)")
    if not t.is_cuda:
        raise ValueError("times is a CPU tensor: hand it over as a numpy array (times.numpy())")
    if t.device.index != int(ctx.device):
        raise ValueError(f"times lives on {t.device}, the context on cuda:{ctx.device}")
    return _device_array(t.data_ptr(), _IO_DTYPES[name], 1, t.stride(0) if n > 1 else 1)


def _torch_stream(ctx, stream):
    import torch

    if stream is None:
        stream = torch.cuda.current_stream(int(ctx.device))
    return int(getattr(stream, "cuda_stream", stream))  # a torch.cuda.Stream, or the hipStream_t as an integer


def _cloud_from_device_arrays(ctx, pa, na, ca, n, origin, relative, stream):
    if relative and origin is None:
        raise ValueError("relative=True needs an origin")
    o = None if origin is None else np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
    if n == 0:
        return PointCloud(ctx=ctx)
    h = C.c_void_p()
    ref = lambda a: None if a is None else C.byref(a)  # noqa: E731
    check(load().sga_cloud_create_device(ctx.h, ref(pa), ref(na), ref(ca), int(n), _dp(o), C.c_void_p(int(stream)), _lib.IO_RELATIVE if relative else 0, C.byref(h)))
    return PointCloud(ctx=ctx, _handle=h)


def _cloud_from_torch(points, normals=None, covs=None, ctx=None, origin=None, relative=False, stream=None):
    pa, n = _torch_rows(points, "points", ctx, (3,))
    if ctx is None:  # (after the first checks: a tensor that cannot be taken is refused without a device)
        ctx = default_context()
        _torch_rows(points, "points", ctx, (3,))
    na = ca = None
    if normals is not None:
        na, nn = _torch_rows(normals, "normals", ctx, (3,))
        if nn != n:
            raise ValueError("normals must have one row per point")
    if covs is not None:
        ca, nc = _torch_rows(covs, "covs", ctx, (6, 9, 16))
        if nc != n:
            raise ValueError("covs must have one row per point")
    return _cloud_from_device_arrays(ctx, pa, na, ca, n, origin, relative, _torch_stream(ctx, stream))


def _cloud_from_device_pointer(ptr, n, dtype=np.float32, stride=3, normals_ptr=None, normals_stride=3, covs_ptr=None, covs_cols=6, covs_stride=None, ctx=None, origin=None, relative=False, stream=0):
    name = np.dtype(dtype).name
    if name not in _IO_DTYPES:
        raise ValueError("dtype must be float32 or float64")
    ctx = ctx or default_context()
    dt = _IO_DTYPES[name]
    pa = _device_array(ptr, dt, 3, stride)
    na = None if normals_ptr is None else _device_array(normals_ptr, dt, 3, normals_stride)
    ca = None if covs_ptr is None else _device_array(covs_ptr, dt, covs_cols, covs_cols if covs_stride is None else covs_stride)
    return _cloud_from_device_arrays(ctx, pa, na, ca, n, origin, relative, stream or 0)


def _cloud_to_torch(self, points=True, normals=False, covs=False, dtype=None, stream=None, out=None):
    """PointCloud.to_torch: the result tensors are allocated on `stream`, so torch's allocator orders their reuse behind it."""
    import torch

    dtype = torch.float32 if dtype is None else dtype
    name = str(dtype).replace("torch.", "")
    if name not in _IO_DTYPES:
        raise ValueError("dtype must be torch.float32 or torch.float64")
    n = self.size()
    dev = torch.device("cuda", int(self.ctx.device))
    s = _torch_stream(self.ctx, stream)
    res, arrs = [], [None, None, None]
    with torch.cuda.stream(torch.cuda.ExternalStream(s, device=dev)) if stream is not None else torch.cuda.device(dev):
        for slot, (want, cols) in enumerate(((points, 3), (normals, 3), (covs, 6))):
            if not want:
                continue
            if slot == 0 and out is not None:
                t = out
                if t.dtype != dtype or t.shape[0] != n:
                    raise ValueError("out must have one row per point and the requested dtype")
            else:
                t = torch.empty((n, cols), dtype=dtype, device=dev)
            arrs[slot] = _torch_rows(t, ("points", "normals", "covs")[slot], self.ctx, (cols,))[0]
            res.append(t)
    if n > 0 and res:
        ref = lambda a: None if a is None else C.byref(a)  # noqa: E731
        check(load().sga_cloud_export_device(self.ctx.h, self.h, ref(arrs[0]), ref(arrs[1]), ref(arrs[2]), C.c_void_p(s), 0))
    return res[0] if len(res) == 1 else tuple(res)


def _knn_torch(self, queries, k, max_sq_dist=-1.0, stream=None):
    import torch

    qa, m = _torch_rows(queries, "queries", self.ctx, (3, 4))
    qa.cols = 3  # an (m,4) tensor of homogeneous points: the first three columns of every row
    k = int(k)
    dev = torch.device("cuda", int(self.ctx.device))
    s = _torch_stream(self.ctx, stream)
    with torch.cuda.stream(torch.cuda.ExternalStream(s, device=dev)) if stream is not None else torch.cuda.device(dev):
        idx = torch.empty((m, k), dtype=torch.int64, device=dev)
        d2 = torch.empty((m, k), dtype=torch.float32, device=dev)
    if m > 0:
        check(load().sga_index_knn_device(self.ctx.h, self.h, C.byref(qa), int(m), k, float(max_sq_dist), C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr()), C.c_void_p(s), 0))
    return idx, d2


def _factors_torch(self, stream=None):
    import torch

    n = self.source.size()
    dev = torch.device("cuda", int(self.ctx.device))
    s = _torch_stream(self.ctx, stream)
    with torch.cuda.stream(torch.cuda.ExternalStream(s, device=dev)) if stream is not None else torch.cuda.device(dev):
        ti = torch.empty((n,), dtype=torch.int64, device=dev)
        m6 = torch.empty((n, 6), dtype=torch.float32, device=dev)
    if n > 0:
        check(load().sga_problem_get_factors_device(self.ctx.h, self.h, C.c_void_p(ti.data_ptr()), C.c_void_p(m6.data_ptr()), C.c_void_p(s), 0))
    return ti, m6


def set_warm_limit(warm_delta_m):
    """sga_set_warm_limit: a negative limit makes every linearization pass walk in full (used by tests to compare the two kinds of pass)."""
    load().sga_set_warm_limit(float(warm_delta_m))


def set_error_model(enabled):
    """sga_set_error_model: False makes every error pass run the error kernel instead of the quadratic model of the last linearization."""
    load().sga_set_error_model(1 if enabled else 0)


def set_search_mode(queue=2, chunk_tiles_cold=0, chunk_tiles_warm=0):
    """sga_set_search_mode: 1 / True = queue-fed search kernel, 0 / False = one query per lane, 2 = automatic (default); tiles of 64
    source points per wave of the queue-fed kernel."""
    load().sga_set_search_mode(int(queue), int(chunk_tiles_cold), int(chunk_tiles_warm))


def set_grid_mode(mode=-1, min_points=-1):
    """sga_set_grid_mode (small_gicp_amd_debug.h): what the cell grid is used for (0 nothing, 1 default: the walkers of warm passes, 2 also
    cold passes but a registration's first, 3 the first too, 4 every pass) and from how many target points on an index gets one.  Results
    do not depend on it."""
    load().sga_set_grid_mode(int(mode), int(min_points))


def get_warm_limit():
    return float(load().sga_get_warm_limit())


def unpack_accumulator(acc30):
    a = np.ascontiguousarray(acc30, dtype=np.float64)
    H, b = np.empty(36), np.empty(6)
    e, n = C.c_double(), C.c_uint64()
    load().sga_unpack_accumulator(_dp(a), _dp(H), _dp(b), C.byref(e), C.byref(n))
    return H.reshape(6, 6), b, e.value, n.value


def error_model_eval(acc96, T_lin, T):
    """sga_error_model_eval (host only): the error at trial pose T from the 96-double accumulator of a linearization at T_lin."""
    a = np.ascontiguousarray(acc96, dtype=np.float64)
    assert a.size >= 96
    tl, t = _T16(T_lin), _T16(T)
    e = C.c_double()
    check(load().sga_error_model_eval(_dp(a), _dp(tl), _dp(t), C.byref(e)))
    return e.value


def optimize(setting, init_T, linearize, error):
    """sga_optimize: the host LM/GN over python callbacks linearize(T)->(H,b,e,num_inliers), error(T)->e.  T is 4x4 row-major numpy."""

    def _lin(user, T, H, b, e, n):
        try:
            Tm = np.ctypeslib.as_array(T, shape=(16,)).reshape(4, 4).T
            h, bb, ee, nn = linearize(Tm.copy())
            np.ctypeslib.as_array(H, shape=(36,))[:] = np.asarray(h, dtype=np.float64).reshape(36)
            np.ctypeslib.as_array(b, shape=(6,))[:] = np.asarray(bb, dtype=np.float64).reshape(6)
            e[0] = float(ee)
            n[0] = int(nn)
            return 0
        except Exception as ex:  # noqa: BLE001
            _lin.exc = ex
            return 1

    def _err(user, T, e):
        try:
            Tm = np.ctypeslib.as_array(T, shape=(16,)).reshape(4, 4).T
            e[0] = float(error(Tm.copy()))
            return 0
        except Exception as ex:  # noqa: BLE001
            _lin.exc = ex
            return 1

    _lin.exc = None
    res = ResultC()
    t16 = _T16(init_T)
    rc = load().sga_optimize(C.byref(setting), _dp(t16), _lib.LINEARIZE_FN(_lin), _lib.ERROR_FN(_err), None, C.byref(res))
    if _lin.exc is not None:
        raise _lin.exc
    check(rc)
    return RegistrationResult(res)


# ---- preprocessing (src/python/preprocess.cpp) -----------------------------------------------------------------------------
def voxelgrid_sampling(points, downsampling_resolution, num_threads=1):
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    out = C.c_void_p()
    check(load().sga_voxelgrid_sampling(cloud.ctx.h, cloud.h, float(downsampling_resolution), C.byref(out)))
    return PointCloud(ctx=cloud.ctx, _handle=out)


def _estimate(cloud, tree, num_neighbors, flags):
    check(load().sga_estimate_normals_covariances(cloud.ctx.h, cloud.h, tree.h if tree is not None else None, int(num_neighbors), flags))


def estimate_normals(points, tree=None, num_neighbors=20, num_threads=1):
    _estimate(points, tree, num_neighbors, 1)


def estimate_covariances(points, tree=None, num_neighbors=20, num_threads=1):
    _estimate(points, tree, num_neighbors, 2)


def estimate_normals_covariances(points, tree=None, num_neighbors=20, num_threads=1):
    _estimate(points, tree, num_neighbors, 3)


def _one_context(clouds):
    for c in clouds:
        if not isinstance(c, PointCloud):
            raise TypeError("a batch takes PointCloud objects")
    ctx = clouds[0].ctx if clouds else default_context()
    if any(c.ctx is not ctx for c in clouds):
        raise ValueError("the clouds of a batch must belong to one context")
    return ctx


def build_kdtrees(clouds):
    """sga_index_build_kdtree_batch: [KdTree(c) for c in clouds] in one chain of launches (clouds of one context).  Every tree is an
    ordinary KdTree, bit-identical to the lone build's; clouds of at most 32768 points share the launches, others are built one by one."""
    clouds = list(clouds)
    ctx = _one_context(clouds)
    hs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    out = (C.c_void_p * max(1, len(clouds)))()
    check(load().sga_index_build_kdtree_batch(ctx.h, hs, len(clouds), out))
    return [KdTree(c, _handle=C.c_void_p(out[k])) for k, c in enumerate(clouds)]


def _estimate_batch(clouds, trees, num_neighbors, flags):
    clouds, trees = list(clouds), list(trees)
    if len(clouds) != len(trees):
        raise ValueError("as many trees as clouds")
    ctx = _one_context(clouds)
    for t in trees:
        if not isinstance(t, KdTree):
            raise TypeError("a batched estimation takes the KdTree of every cloud")
    cs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    ts = (C.c_void_p * max(1, len(trees)))(*[t.h.value for t in trees])
    check(load().sga_estimate_normals_covariances_batch(ctx.h, cs, ts, len(clouds), int(num_neighbors), flags))


def estimate_normals_batch(clouds, trees, num_neighbors=20):
    """estimate_normals(clouds[k], trees[k], num_neighbors) for all k in one chain of launches (sga_estimate_normals_covariances_batch)."""
    _estimate_batch(clouds, trees, num_neighbors, 1)


def estimate_covariances_batch(clouds, trees, num_neighbors=20):
    """estimate_covariances(clouds[k], trees[k], num_neighbors) for all k in one chain of launches."""
    _estimate_batch(clouds, trees, num_neighbors, 2)


def estimate_normals_covariances_batch(clouds, trees, num_neighbors=20):
    """estimate_normals_covariances(clouds[k], trees[k], num_neighbors) for all k in one chain of launches."""
    _estimate_batch(clouds, trees, num_neighbors, 3)


def preprocess_batch(clouds, num_neighbors=20):
    """The kd-trees and the covariances of several (downsampled) clouds of one context, each made by one batched call:
    [(cloud, tree)] with what KdTree(cloud) and estimate_covariances(cloud, tree, num_neighbors) give every pair, bit for bit."""
    clouds = list(clouds)
    trees = build_kdtrees(clouds)
    estimate_covariances_batch(clouds, trees, num_neighbors)
    return list(zip(clouds, trees))


def voxelgrid_sampling_batch(clouds, resolution):
    """sga_voxelgrid_sampling_batch: [voxelgrid_sampling(c, resolution) for c in clouds] in one chain of launches (PointCloud objects of one
    context).  Every output is an ordinary PointCloud, bit-identical to the lone call's; uploaded clouds of at most 262144 points share
    the launches, others (clouds made on the device, larger ones) are downsampled one by one inside the call."""
    clouds = list(clouds)
    ctx = _one_context(clouds)
    hs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    out = (C.c_void_p * max(1, len(clouds)))()
    check(load().sga_voxelgrid_sampling_batch(ctx.h, hs, len(clouds), float(resolution), out))
    return [PointCloud(ctx=ctx, _handle=C.c_void_p(out[k])) for k in range(len(clouds))]


def preprocess_points_batch(clouds, downsampling_resolution=0.25, num_neighbors=10):
    """preprocess_points for several raw clouds of one context, every stage batched: voxelgrid_sampling_batch, then preprocess_batch.
    [(downsampled cloud, tree)], each pair what the lone calls give, bit for bit."""
    return preprocess_batch(voxelgrid_sampling_batch(clouds, downsampling_resolution), num_neighbors)


def build_gaussian_voxelmaps(clouds, leaf_size):
    """sga_index_build_gaussian_voxelmap_batch: [GaussianVoxelMap.from_cloud(c, leaf_size) for c in clouds] in one chain of launches and
    one host wait (PointCloud objects with covariances, of one context).  Every map is an ordinary one-shot GaussianVoxelMap, its contents
    bit-identical to the lone build's; clouds of at most 262144 points share the launches, others — and clouds that span 65536 or more
    voxels along an axis — are built one by one inside the call."""
    clouds = list(clouds)
    ctx = _one_context(clouds)
    hs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    out = (C.c_void_p * max(1, len(clouds)))()
    check(load().sga_index_build_gaussian_voxelmap_batch(ctx.h, hs, len(clouds), float(leaf_size), out))
    return [GaussianVoxelMap._adopt(leaf_size, ctx, C.c_void_p(out[k])) for k in range(len(clouds))]


def _voxelmap_batch_plan(clouds, leaf_size):
    """Diagnostics (sga_debug_voxelmap_batch_plan): what build_gaussian_voxelmaps(clouds, leaf_size) would do — forest (members of the
    shared chain), lone (members through the lone routine), empty, member_bits, end_bit of the chain's sort, points of the concatenation."""
    clouds = list(clouds)
    _one_context(clouds)
    hs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    out = (C.c_int * 6)()
    check(load().sga_debug_voxelmap_batch_plan(hs, len(clouds), float(leaf_size), out))
    return {"forest": out[0], "lone": out[1], "empty": out[2], "member_bits": out[3], "end_bit": out[4], "points": out[5]}


def merge_clouds(clouds, Ts=None, origin=None, ctx=None):
    """sga_cloud_merge: the clouds posed by Ts (4x4 each; None: identities) joined into one PointCloud — the last K keyframes at their
    estimated poses as one registration target — by one table copy and one launch, whatever their number.  The output holds clouds[0]'s
    points, then clouds[1]'s, ...; a record r of a member with pose (R, t) and origin o_m becomes fl32(R r + ((R o_m + t) - o)), evaluated
    in double; normals R n and covariances R C R^T ride along, each kept only if every non-empty member has it.  origin: the output's
    device-frame origin o (None: chosen by the library from the bounding box of the posed points, which costs the one host wait).  The
    members may belong to several contexts of one device (another device: the library refuses); ctx: the context the merge runs on
    (default: the first cloud's)."""
    clouds = list(clouds)
    for c in clouds:
        if not isinstance(c, PointCloud):
            raise TypeError("merge_clouds takes PointCloud objects")
    ctx = ctx or (clouds[0].ctx if clouds else default_context())
    hs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    t16 = None if Ts is None else _T16s(Ts, len(clouds))
    o = None if origin is None else np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    h = C.c_void_p()
    check(load().sga_cloud_merge(ctx.h, hs, None if t16 is None else _dp(t16), len(clouds), _dp(o), C.byref(h)))
    return PointCloud(ctx=ctx, _handle=h)


def se3_exp(twist):
    """sga_se3_exp: the 4x4 pose of a twist [rx ry rz tx ty tz] (rotation first), evaluated without cancellation at small angles."""
    xi = np.ascontiguousarray(np.asarray(twist, dtype=np.float64).reshape(6))
    T = np.empty(16)
    load().sga_se3_exp(_dp(xi), _dp(T))
    return T.reshape(4, 4).T.copy()


def se3_log(T):
    """sga_se3_log: the twist whose se3_exp is the rigid transform T (rotation angle below pi)."""
    t16 = _T16(T)
    xi = np.empty(6)
    load().sga_se3_log(_dp(t16), _dp(xi))
    return xi


def deskew_clouds(clouds, times, twists, ref_times=None, ctx=None):
    """sga_cloud_deskew_batch: PointCloud.deskewed for B sweeps — times[k] a numpy array of clouds[k].size() values, twists (B, 6),
    ref_times (B,) or None (1.0 each) — by one table copy and one launch, whatever B is.  Returns the B deskewed clouds.  The members may
    belong to several contexts of one device; ctx: the context the call runs on (default: the first cloud's)."""
    clouds = list(clouds)
    for c in clouds:
        if not isinstance(c, PointCloud):
            raise TypeError("deskew_clouds takes PointCloud objects")
    B = len(clouds)
    times = list(times)
    if len(times) != B:
        raise ValueError(f"{len(times)} time arrays for {B} clouds")
    if B == 0:
        return []  # (count == 0 is no device work: no context is needed)
    ts = [np.ascontiguousarray(np.asarray(t, dtype=np.float32).reshape(-1)) for t in times]
    for k, (c, t) in enumerate(zip(clouds, ts)):
        if len(t) != c.size():
            raise ValueError(f"times[{k}]: {len(t)} times for a cloud of {c.size()} points")
    xi = np.ascontiguousarray(np.asarray(twists, dtype=np.float64).reshape(B, 6))
    rt = None if ref_times is None else np.ascontiguousarray(np.asarray(ref_times, dtype=np.float64).reshape(B))
    ctx = ctx or clouds[0].ctx
    hs = (C.c_void_p * B)(*[c.h.value for c in clouds])
    tp = (C.c_void_p * B)(*[t.ctypes.data if len(t) else C.addressof(_NO_TIMES) for t in ts])
    out = (C.c_void_p * B)()
    check(load().sga_cloud_deskew_batch(ctx.h, hs, tp, _dp(xi), _dp(rt), B, out))
    return [PointCloud(ctx=ctx, _handle=C.c_void_p(out[k])) for k in range(B)]


_NO_TIMES = C.c_float()  # what an empty member's times point at (never read)


_BOX_MODES = {"inside": 1, "outside": 2}


def _crop(min_range=0.0, max_range=np.inf, center=None, box=None, box_mode="inside"):
    """The sga_crop of PointCloud.cropped's arguments (an sga_crop is passed through).  The library judges the values."""
    if isinstance(min_range, _lib.Crop):
        return min_range
    cr = _lib.Crop()
    load().sga_crop_default(C.byref(cr))
    cr.min_range, cr.max_range = float(min_range), float(max_range)
    if center is not None:
        cr.center[:] = [float(v) for v in np.asarray(center, dtype=np.float64).reshape(3)]
    if box is not None:
        if box_mode not in _BOX_MODES:
            raise ValueError('box_mode must be "inside" or "outside"')
        lo, hi = box
        cr.box_lo[:] = [float(v) for v in np.asarray(lo, dtype=np.float64).reshape(3)]
        cr.box_hi[:] = [float(v) for v in np.asarray(hi, dtype=np.float64).reshape(3)]
        cr.box_mode = _BOX_MODES[box_mode]
    return cr


def _outlier_filter(k=10, std_mul=1.0, radius=None):
    """The sga_outlier_filter of PointCloud.without_outliers' arguments (one is passed through).  The library judges the values."""
    if isinstance(k, _lib.OutlierFilter):
        return k
    f = _lib.OutlierFilter()
    load().sga_outlier_filter_default(C.byref(f))
    f.k = int(k)
    if radius is None:
        f.std_mul = float(std_mul)
    else:
        f.mode, f.radius = 1, float(radius)
    return f


def remove_outliers(points, k=10, std_mul=1.0, radius=None, tree=None, return_kept=False, return_stats=False):
    """PointCloud.without_outliers of a PointCloud or of an (N,3|4) array (uploaded first)."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    return cloud.without_outliers(k, std_mul, radius, tree, return_kept, return_stats)


def cloud_outliers_launches():
    """Diagnostics (sga_debug_cloud_outliers_launches): commands enqueued so far by PointCloud.without_outliers (the statistic, the
    threshold, the compaction's table copy, the compaction; a temporary tree's build is not counted)."""
    v = C.c_ulonglong()
    check(load().sga_debug_cloud_outliers_launches(C.byref(v)))
    return v.value


_OVERLAP_KEEP = {None: 0, "matched": 1, "unmatched": 2}


class Features:
    """n rows of dim float32 values on the device (sga_features): FPFH descriptors (PointCloud.fpfh), or a caller's own."""

    def __init__(self, ctx=None, _handle=None):
        self.ctx = ctx or default_context()
        self.h = _handle if _handle is not None else C.c_void_p()

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_features_destroy(self.h)
            self.h = C.c_void_p()

    @staticmethod
    def from_array(rows, ctx=None):
        """Features from an (n, dim) array, 1 <= dim <= 128 (sga_features_create)."""
        a = np.ascontiguousarray(np.asarray(rows), dtype=np.float32)
        if a.ndim != 2:
            raise ValueError("rows must be (n, dim)")
        f = Features(ctx)
        check(load().sga_features_create(f.ctx.h, _fp(a) if len(a) else None, a.shape[0], a.shape[1], C.byref(f.h)))
        return f

    @staticmethod
    def from_torch(rows, ctx=None, stream=None):
        """Features from an (n,) / (n, dim) float32 / float64 tensor on the context's device, any row stride (sga_features_create_device:
        one launch, nothing touches the host; a double is rounded to float32 once)."""
        t = rows[:, None] if getattr(rows, "dim", lambda: 0)() == 1 else rows
        a, n = _torch_rows(t, "rows", ctx, range(1, 129))
        f = Features(ctx)
        _torch_rows(t, "rows", f.ctx, range(1, 129))
        check(load().sga_features_create_device(f.ctx.h, C.byref(a), int(n), C.c_void_p(_torch_stream(f.ctx, stream)), 0, C.byref(f.h)))
        return f

    def to_torch(self, dtype=None, stream=None):
        """The rows as an (n, dim) tensor on the context's device (sga_features_export_device), allocated on `stream`."""
        import torch

        dtype = torch.float32 if dtype is None else dtype
        if str(dtype).replace("torch.", "") not in _IO_DTYPES:
            raise ValueError("dtype must be torch.float32 or torch.float64")
        n, d = self._shape()
        dev = torch.device("cuda", int(self.ctx.device))
        s = _torch_stream(self.ctx, stream)
        with torch.cuda.stream(torch.cuda.ExternalStream(s, device=dev)) if stream is not None else torch.cuda.device(dev):
            t = torch.empty((n, d), dtype=dtype, device=dev)
        if n > 0:
            a = _torch_rows(t, "rows", self.ctx, (d,))[0]
            check(load().sga_features_export_device(self.ctx.h, self.h, C.byref(a), C.c_void_p(s), 0))
        return t

    def _shape(self):
        n, d = C.c_size_t(), C.c_int()
        check(load().sga_features_size(self.h, C.byref(n), C.byref(d)))
        return n.value, d.value

    def size(self):
        return self._shape()[0]

    __len__ = size

    @property
    def dim(self):
        return self._shape()[1]

    def numpy(self):
        n, d = self._shape()
        out = np.empty((n, d), np.float32)
        check(load().sga_features_download(self.ctx.h, self.h, _fp(out) if n else None))
        return out

    def selected(self, indices):
        """New Features whose row j is this one's row indices[j] (sga_features_select: one launch, no host wait); repeats are allowed,
        an index outside the rows is refused and named by its position."""
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64).reshape(-1))
        h = C.c_void_p()
        check(load().sga_features_select(self.ctx.h, self.h, idx.ctypes.data_as(C.POINTER(C.c_int64)) if len(idx) else None, len(idx), C.byref(h)))
        return Features(ctx=self.ctx, _handle=h)


REDUCE = {"mean": _lib.REDUCE_MEAN, "min": _lib.REDUCE_MIN, "max": _lib.REDUCE_MAX, "first": _lib.REDUCE_FIRST, "nearest": _lib.REDUCE_NEAREST}


def _reduce_ops(reduce, dim):
    names = [reduce] * dim if isinstance(reduce, (str, int, np.integer)) else list(reduce)
    if len(names) != dim:
        raise ValueError(f"reduce names {len(names)} columns, the fields have {dim}")
    ops = []
    for c, r in enumerate(names):
        if isinstance(r, str):
            if r.lower() not in REDUCE:
                raise ValueError(f"reduce of column {c}: {r!r} is none of {sorted(REDUCE)}")
            r = REDUCE[r.lower()]
        ops.append(int(r))
    return (C.c_int * dim)(*ops)


def voxelgrid_sampling_fields(cloud, fields, resolution, reduce="mean", return_counts=False, return_voxel_of=False, stream=None):
    """voxelgrid_sampling(cloud, resolution) with per-point columns carried through the merge (sga_voxelgrid_sampling_fields): row v of
    the returned Features reduces, column by column, the rows of `fields` of the points that fell into voxel v — "mean", "min", "max",
    "first" (the member of lowest index) or "nearest" (the member nearest the centroid: a time or a label that must come from one real
    return); one name for all columns or one per column.  fields: a numpy (n,) / (n, dim) array, a Features, a torch tensor on the
    context's device (a view such as scan[:, 3:4] goes down as it is; counts / voxel_of are then tensors too), or None: membership only.
    Returns (PointCloud, Features | None[, counts (M,) int32][, voxel_of (n,) int64: the row of every input point, -1 for a dropped one])."""
    if not isinstance(cloud, PointCloud):
        cloud = PointCloud(cloud)
    ctx, n = cloud.ctx, cloud.size()
    out, out_f = C.c_void_p(), C.c_void_p()
    is_torch = fields is not None and not isinstance(fields, (Features, np.ndarray, list, tuple)) and hasattr(fields, "data_ptr")
    if is_torch:
        import torch

        t = fields[:, None] if fields.dim() == 1 else fields
        fa, rows = _torch_rows(t, "fields", ctx, range(1, 33))
        if rows != n:
            raise ValueError(f"fields have {rows} rows, the cloud has {n} points")
        ops = _reduce_ops(reduce, fa.cols)
        dev = torch.device("cuda", int(ctx.device))
        s = _torch_stream(ctx, stream)
        with torch.cuda.stream(torch.cuda.ExternalStream(s, device=dev)) if stream is not None else torch.cuda.device(dev):
            counts = torch.empty(n, dtype=torch.int32, device=dev) if return_counts else None
            voxel_of = torch.empty(n, dtype=torch.int64, device=dev) if return_voxel_of else None
        ptr = lambda x: C.c_void_p(x.data_ptr() if x is not None and n > 0 else None)  # noqa: E731
        check(load().sga_voxelgrid_sampling_fields_device(ctx.h, cloud.h, C.byref(fa), ops, float(resolution), C.byref(out), C.byref(out_f), ptr(counts), ptr(voxel_of), C.c_void_p(s), 0))
        res = [PointCloud(ctx=ctx, _handle=out), Features(ctx=ctx, _handle=out_f)]
        if return_counts:
            res.append(counts[: res[0].size()])
    else:
        keep = None
        if fields is not None and not isinstance(fields, Features):
            a = np.asarray(fields)
            keep = fields = Features.from_array(a.reshape(len(a), -1) if a.ndim != 2 else a, ctx)
        ops = None if fields is None else _reduce_ops(reduce, fields.dim)
        counts = np.empty(n, np.int32) if return_counts else None
        voxel_of = np.empty(n, np.int64) if return_voxel_of else None
        check(load().sga_voxelgrid_sampling_fields(ctx.h, cloud.h, None if fields is None else fields.h, ops, float(resolution), C.byref(out), None if fields is None else C.byref(out_f),
                                                   None if counts is None else counts.ctypes.data_as(C.POINTER(C.c_int32)), None if voxel_of is None else voxel_of.ctypes.data_as(C.POINTER(C.c_int64))))
        del keep
        res = [PointCloud(ctx=ctx, _handle=out), None if fields is None else Features(ctx=ctx, _handle=out_f)]
        if return_counts:
            res.append(counts[: res[0].size()].copy())
    if return_voxel_of:
        res.append(voxel_of)
    return tuple(res)


def voxelgrid_fields_launches():
    """Diagnostics (sga_debug_voxelgrid_fields_launches): launches enqueued so far by voxelgrid_sampling_fields, four per call."""
    return _launches("sga_debug_voxelgrid_fields_launches")


def compute_fpfh(points, tree=None, k=20, viewpoint=(0.0, 0.0, 0.0)):
    """PointCloud.fpfh of a PointCloud with normals."""
    return points.fpfh(tree, k, viewpoint)


def match_features(src, tgt, mutual=True, return_dist=False):
    """For every row of src the nearest row of tgt in squared L2 distance (sga_features_match; ties to the lowest index); mutual: only the
    pairs that are each other's nearest.  Returns the pairs, (M, 2) int64 (source row, target row), ascending in the source row
    [, and the distances (M,) float64]."""
    n = src.size()
    match = np.empty(n, np.int64)
    dist = np.empty(n, np.float64) if return_dist else None
    cnt = C.c_size_t()
    check(load().sga_features_match(src.ctx.h, src.h, tgt.h, 1 if mutual else 0, match.ctypes.data_as(C.POINTER(C.c_int64)), _dp(dist), C.byref(cnt)))
    keep = np.nonzero(match >= 0)[0]
    pairs = np.ascontiguousarray(np.stack([keep.astype(np.int64), match[keep]], axis=1))
    return (pairs, dist[keep]) if return_dist else pairs


def _ransac_params(**fields):
    p = _lib.Ransac()
    load().sga_ransac_default(C.byref(p))
    for name, value in fields.items():
        if value is not None:
            setattr(p, name, value)
    return p


def ransac_correspondences(source, target, pairs, max_distance=None, iterations=None, seed=None, edge_similarity=None, min_edge=None):
    """The rigid motion most of the index pairs (M, 2) (source point, target point) agree on (sga_ransac_correspondences; DESIGN.md
    section 3.24); None: the library's default (1.0, 20000, 0, 0.9, 0.0).  Returns a dict: "T" (4x4, source -> target), "inliers",
    "inlier_rmse", "best_hypothesis", "scored", "refit"."""
    pr = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2))
    p = _ransac_params(max_distance=max_distance, iterations=None if iterations is None else int(iterations), seed=None if seed is None else int(seed), edge_similarity=edge_similarity, min_edge=min_edge)
    T = np.empty(16)
    r = _lib.RansacResult()
    check(load().sga_ransac_correspondences(source.ctx.h, source.h, target.h, pr.ctypes.data_as(C.POINTER(C.c_int64)) if len(pr) else None, len(pr), C.byref(p), _dp(T), C.byref(r)))
    return {"T": T.reshape(4, 4).T.copy(), "inliers": int(r.inliers), "inlier_rmse": r.inlier_rmse, "best_hypothesis": int(r.best_hypothesis), "scored": int(r.scored), "refit": int(r.refit)}


def _iss_params(salient_radius, non_max_radius=None, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, keep=False):
    """The sga_iss_params of PointCloud.iss_keypoints' arguments (one is passed through).  The library judges the values."""
    if isinstance(salient_radius, _lib.IssParams):
        return salient_radius
    p = _lib.IssParams()
    load().sga_iss_default(C.byref(p))
    p.salient_radius, p.non_max_radius, p.gamma_21, p.gamma_32, p.min_neighbors, p.keep = float(salient_radius), float(non_max_radius), float(gamma_21), float(gamma_32), int(min_neighbors), 1 if keep else 0
    return p


def iss_keypoints(points, salient_radius, non_max_radius, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, tree=None, keep=False, return_saliency=False):
    """PointCloud.iss_keypoints of a PointCloud or of an (N,3|4) array (uploaded first)."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    return cloud.iss_keypoints(salient_radius, non_max_radius, gamma_21, gamma_32, min_neighbors, tree, keep, return_saliency)


def iss_launches():
    """Diagnostics (sga_debug_iss_launches): commands enqueued so far by PointCloud.iss_keypoints — three per call, four when a cloud is
    made; the build of a temporary tree is not counted."""
    return _launches("sga_debug_iss_launches")


def iss_waits():
    """Diagnostics (sga_debug_iss_waits): host waits so far of PointCloud.iss_keypoints, one per call."""
    return _launches("sga_debug_iss_waits")


def global_align(target_points, source_points, voxel_size, k=20, iterations=20000, seed=0, refine=True, setting=None, viewpoint=(0.0, 0.0, 0.0), keypoints=None):
    """A pose from geometry alone, then the local registration from it: voxel grid at voxel_size, trees, normals
    and covariances, FPFH with the viewpoint at each cloud's sensor origin (viewpoint, in each cloud's own frame; default (0, 0, 0)), mutual matching, RANSAC with max_distance = 1.5
    voxel_size and min_edge = 2 voxel_size, and — refine — GICP (setting: a make_setting; default "GICP") from the coarse pose.
    keypoints: None — every point is described and matched; True, or a dict of PointCloud.iss_keypoints'
    arguments (True: salient_radius = 3 voxel_size, non_max_radius = 1.5 voxel_size) — only the ISS keypoints of both clouds are
    matched (FPFH is still computed over the whole clouds), the pairs name points of the clouds, and RANSAC and the refinement
    run over the full clouds as without.
    Returns (coarse, refined): the dict of ransac_correspondences with "pairs" added (and, with keypoints, "keypoints": their numbers
    (source, target)), and the RegistrationResult (None without refine)."""
    if keypoints is not None and keypoints is not True and not isinstance(keypoints, dict):
        raise ValueError("keypoints must be None, True or a dict of iss_keypoints' arguments")
    tgt, ttree = preprocess_points(target_points, voxel_size, k)
    src, stree = preprocess_points(source_points, voxel_size, k)
    if keypoints is None:
        pairs = match_features(src.fpfh(stree, k, viewpoint), tgt.fpfh(ttree, k, viewpoint), mutual=True)
    else:
        args = dict(salient_radius=3.0 * voxel_size, non_max_radius=1.5 * voxel_size) if keypoints is True else dict(keypoints)
        if {"tree", "keep", "return_saliency"} & set(args):
            raise ValueError("keypoints: tree, keep and return_saliency are global_align's own")
        ks, kt = src.iss_keypoints(tree=stree, **args)["indices"], tgt.iss_keypoints(tree=ttree, **args)["indices"]
        rows = match_features(src.fpfh(stree, k, viewpoint).selected(ks), tgt.fpfh(ttree, k, viewpoint).selected(kt), mutual=True)
        pairs = np.ascontiguousarray(np.stack([ks[rows[:, 0]], kt[rows[:, 1]]], axis=1))  # keypoint rows -> cloud indices
    coarse = ransac_correspondences(src, tgt, pairs, max_distance=1.5 * voxel_size, iterations=iterations, seed=seed, min_edge=2.0 * voxel_size)
    coarse["pairs"] = pairs
    if keypoints is not None:
        coarse["keypoints"] = (len(ks), len(kt))
    refined = None
    if refine:
        refined = Problem(ttree, src, coarse["T"]).align(setting or make_setting("GICP"), coarse["T"])
    return coarse, refined


def _place_params(**fields):
    p = _lib.PlaceParams()
    load().sga_place_params_default(C.byref(p))
    for name, value in fields.items():
        if value is not None:
            setattr(p, name, value)
    return p


def _center3(center):
    return None if center is None else np.ascontiguousarray(np.asarray(center, dtype=np.float64).reshape(3))


PLACE_MATCH_DTYPE = np.dtype([("index", np.int64), ("shift", np.int32), ("reserved", np.int32), ("distance", np.float64)])


class PlaceDatabase:
    """Scan Context descriptors of keyframes on the device, searched exhaustively at every column shift (sga_places_*; DESIGN.md
    section 3.25).  add() forms a descriptor on the device, where it stays; query() returns the nearest entries with the column shift
    that aligns them, which is the yaw between the two visits in units of 2 pi / sectors."""

    def __init__(self, ctx=None, rings=20, sectors=60, max_range=80.0, height=2.0):
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        p = _place_params(rings=int(rings), sectors=int(sectors), max_range=float(max_range), height=float(height))
        check(load().sga_places_create(self.ctx.h, C.byref(p), C.byref(self.h)))
        self.rings, self.sectors, self.max_range, self.height = p.rings, p.sectors, p.max_range, p.height

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_places_destroy(self.h)
            self.h = C.c_void_p()

    def __len__(self):
        n = C.c_size_t()
        check(load().sga_places_size(self.h, C.byref(n)))
        return n.value

    def _image(self, image):
        a = np.ascontiguousarray(np.asarray(image), dtype=np.float32)
        if a.shape != (self.rings, self.sectors):
            raise ValueError(f"image must be ({self.rings}, {self.sectors}), not {a.shape}")
        return a

    def add(self, cloud, center=None):
        """The descriptor of a PointCloud becomes the next entry; returns its index.  center: the sensor's position in the cloud's
        coordinates (None: zeros)."""
        i = C.c_size_t()
        check(load().sga_places_add(self.ctx.h, self.h, cloud.h, _dp(_center3(center)), C.byref(i)))
        return i.value

    def add_descriptor(self, image):
        """A (rings, sectors) image (finite, >= 0) becomes the next entry: crafted, or reloaded from descriptors(); returns its index."""
        i = C.c_size_t()
        check(load().sga_places_add_descriptor(self.ctx.h, self.h, _fp(self._image(image)), C.byref(i)))
        return i.value

    def descriptors(self, first=0, count=None):
        """The images of the entries [first, first + count) (count None: to the end), (count, rings, sectors) float32."""
        count = len(self) - first if count is None else count
        out = np.empty((max(count, 0), self.rings, self.sectors), np.float32)
        check(load().sga_places_download(self.ctx.h, self.h, first, count, _fp(out) if count > 0 else None))
        return out

    def query(self, cloud_or_image, k=1, exclude_recent=0, first=None, count=None, center=None, return_all=False):
        """The k entries nearest to a PointCloud's descriptor (center as in add) or to a (rings, sectors) image, among the entries
        [first, first + count): first None: 0; count None: to the end, less the exclude_recent latest entries (the keyframes a mapping
        loop has just added are no loop closures).  Returns a dict: "index" (m,) int64, "shift" (m,) int32, "distance" (m,) float64 —
        ascending in (distance, index), m = min(k, candidates) — and "yaw" = shift 2 pi / sectors; with return_all also "all_distance"
        and "all_shift" for every candidate."""
        n = len(self)
        first = 0 if first is None else int(first)
        count = max(n - first - int(exclude_recent), 0) if count is None else int(count)
        out = np.zeros(max(int(k), 1), PLACE_MATCH_DTYPE)
        found = C.c_size_t()
        all_d = np.empty(count, np.float64) if return_all else None
        all_s = np.empty(count, np.int32) if return_all else None
        tail = (first, count, int(k), out.ctypes.data_as(C.POINTER(_lib.PlaceMatch)), C.byref(found), _dp(all_d), None if all_s is None else all_s.ctypes.data_as(C.POINTER(C.c_int32)))
        if isinstance(cloud_or_image, PointCloud):
            check(load().sga_places_query(self.ctx.h, self.h, cloud_or_image.h, _dp(_center3(center)), *tail))
        else:
            check(load().sga_places_query_descriptor(self.ctx.h, self.h, _fp(self._image(cloud_or_image)), *tail))
        m = out[: found.value]
        res = {"index": m["index"].copy(), "shift": m["shift"].copy(), "distance": m["distance"].copy()}
        res["yaw"] = res["shift"].astype(np.float64) * (2.0 * np.pi / self.sectors)
        if return_all:
            res["all_distance"], res["all_shift"] = all_d, all_s
        return res

    def yaw_guess(self, shift):
        """The initial guess a shift stands for: the 4x4 rotation about z by shift 2 pi / sectors — T_entry^-1 T_query when the two
        visits differ by a turn alone."""
        a = float(shift) * (2.0 * np.pi / self.sectors)
        T = np.eye(4)
        T[0, 0], T[0, 1], T[1, 0], T[1, 1] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        return T


def scan_context_distance(q, c):
    """The shift-aligned distance of two (rings, sectors) images on the host, in numpy float64 (the rule of small_gicp_amd.h: the mean
    column cosine distance, least over all circular column shifts, ties to the lowest shift): (distance, shift).  A helper for users
    who hold descriptors; the device's search is PlaceDatabase.query."""
    q, c = np.asarray(q, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if q.ndim != 2 or q.shape != c.shape:
        raise ValueError("q and c must be (rings, sectors) images of one shape")
    S = q.shape[1]
    nq, nc = np.sqrt((q * q).sum(axis=0)), np.sqrt((c * c).sum(axis=0))
    best, shift = np.inf, 0
    for s in range(S):
        cs, ns = np.roll(c, -s, axis=1), np.roll(nc, -s)
        ok = (nq > 0) & (ns > 0)
        d = 1.0 - float(((q * cs).sum(axis=0)[ok] / (nq[ok] * ns[ok])).sum()) / ok.sum() if ok.any() else 1.0
        if d < best:
            best, shift = d, s
    return best, shift


def places_add_launches():
    """Diagnostics (sga_debug_places_add_launches): commands enqueued so far by PlaceDatabase.add (three per call), add_descriptor (one)
    and PointCloud.scan_context (three), plus one copy per growth of a database."""
    return _launches("sga_debug_places_add_launches")


def places_query_launches():
    """Diagnostics (sga_debug_places_query_launches): commands enqueued so far by PlaceDatabase.query (four by cloud, two by image)."""
    return _launches("sga_debug_places_query_launches")


def places_waits():
    """Diagnostics (sga_debug_places_waits): host waits so far of the place-recognition calls (a query: one; an add on a
    stream-ordered context: none)."""
    return _launches("sga_debug_places_waits")


OCCUPANCY_STATES = {"unknown": 1, "free": 2, "occupied": 4}


def _state_mask(what, name):
    """An int as it is, a state's name, or several of them: the bits of sga_occupancy_classify / export (1 unknown, 2 free, 4 occupied)."""
    if what is None:
        return 0
    if isinstance(what, (int, np.integer)):
        return int(what)
    names = [what] if isinstance(what, str) else list(what)
    for w in names:
        if w not in OCCUPANCY_STATES:
            raise ValueError("%s must name unknown, free or occupied, not %r" % (name, w))
    return sum({OCCUPANCY_STATES[w] for w in names})


def _occupancy_counts(c):
    return {"total": int(c.total), "unknown": int(c.unknown), "free": int(c.free), "occupied": int(c.occupied), "epoch": int(c.epoch)}


class OccupancyGrid:
    """A dense occupancy grid on the device (sga_occupancy_*): the box with the minimum corner `origin` (world),
    dims = (nx, ny, nz) cells of `leaf` metres; a cell holds a stamp (0: never observed) and an fp32 log-odds.  integrate() ray-casts a
    posed scan into it — free space along every beam, an endpoint at every return within range; classify() says unknown / free /
    occupied for the points of a posed cloud and hands back the kept ones; stats(), export() and download() read the cells.  The log-odds
    parameters are OctoMap's by default."""

    def __init__(self, origin, leaf, dims, l_hit=0.85, l_miss=-0.4, l_min=-2.0, l_max=3.5, ctx=None):
        self.ctx = ctx or default_context()
        self.h = C.c_void_p()
        p = _lib.OccupancyParams()
        load().sga_occupancy_params_default(C.byref(p))
        o, d = np.asarray(origin, dtype=np.float64).reshape(3), np.asarray(dims).reshape(3)
        for k in range(3):
            p.origin[k], p.dims[k] = float(o[k]), int(d[k])
        p.leaf, p.l_hit, p.l_miss, p.l_min, p.l_max = float(leaf), float(l_hit), float(l_miss), float(l_min), float(l_max)
        check(load().sga_occupancy_create(self.ctx.h, C.byref(p), C.byref(self.h)))
        self.origin, self.leaf, self.dims = o.copy(), p.leaf, (int(d[0]), int(d[1]), int(d[2]))
        self.cells = self.dims[0] * self.dims[1] * self.dims[2]

    def __del__(self):
        if getattr(self, "h", None) and self.h.value:
            load().sga_occupancy_destroy(self.h)
            self.h = C.c_void_p()

    @property
    def epoch(self):
        """The scans integrated since creation or the last clear()."""
        e = C.c_uint64()
        check(load().sga_occupancy_get(self.h, None, C.byref(e)))
        return e.value

    def clear(self, ctx=None):
        """Every cell back to never observed, the epoch to 0."""
        check(load().sga_occupancy_clear((ctx or self.ctx).h, self.h))

    def integrate(self, scan, T=None, min_range=0.5, max_range=60.0, mode=0, return_stats=False, ctx=None):
        """Ray-cast a PointCloud in its sensor frame, posed by T (4x4: sensor frame -> world; None: the identity): returns nearer than
        min_range are ignored, beams beyond max_range are cut there and mark free space only (max_range / leaf <= 4096).  mode 1: the
        endpoints only, no free space.  Two launches and no host wait; return_stats=True waits once and returns a dict — "beams",
        "ignored", "hits", "truncated", "cells_hit", "cells_freed"."""
        st = _lib.OccupancyScanStats() if return_stats else None
        t16 = None if T is None else _T16(T)
        check(load().sga_occupancy_integrate((ctx or self.ctx).h, self.h, scan.h, _dp(t16), float(min_range), float(max_range), int(mode), C.byref(st) if return_stats else None))
        if return_stats:
            return {name: int(getattr(st, name)) for name, _ in st._fields_}

    def classify(self, cloud, T=None, threshold=0.0, keep=None, return_state=False, return_kept=False, ctx=None):
        """The state of every point of a PointCloud posed by T (None: the identity): 0 unknown (outside the box, non-finite, never
        observed), 1 free (log-odds < threshold), 2 occupied.  Returns a dict — "total", "unknown", "free", "occupied", "epoch" —
        followed, as requested and in this order, by the cloud of the kept points (keep: a state's name, a list of names, or the bit
        mask 1 unknown | 2 free | 4 occupied; the cloud's order, normals, covariances and origin are kept: keep=("unknown", "occupied")
        is the cleaner a keyframe runs against accumulated evidence), "state" (numpy uint8) and "kept" (numpy int64, ascending; needs
        keep)."""
        ctx = ctx or self.ctx
        mask = _state_mask(keep, "keep")
        n = cloud.size()
        state = np.empty(n, np.uint8) if return_state else None
        kept = np.empty(n, np.int64) if return_kept else None
        c = _lib.OccupancyCounts()
        h = C.c_void_p()
        t16 = None if T is None else _T16(T)
        check(load().sga_occupancy_classify(ctx.h, self.h, cloud.h, _dp(t16), float(threshold), mask, None if state is None else state.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(c), C.byref(h) if mask != 0 else None))
        res = [_occupancy_counts(c)]
        out = None
        if mask != 0:
            out = PointCloud(ctx=ctx, _handle=h)
            res.append(out)
        if return_state:
            res.append(state)
        if return_kept:
            res.append(kept[: out.size()].copy())
        return res[0] if len(res) == 1 else tuple(res)

    def stats(self, threshold=0.0, ctx=None):
        """The cells per state and the epoch: a dict — "total", "unknown", "free", "occupied", "epoch"."""
        c = _lib.OccupancyCounts()
        check(load().sga_occupancy_stats((ctx or self.ctx).h, self.h, float(threshold), C.byref(c)))
        return _occupancy_counts(c)

    def export(self, threshold=0.0, which="occupied", capacity=None, return_cloud=True, ctx=None):
        """The selected cells (which: as classify's keep) in ascending linear index (z * ny + y) * nx + x: a dict — "count" (the number
        selected, whatever the capacity), "indices" (int64), "log_odds" (float32) and, with return_cloud, "cloud": the PointCloud of
        the cell centres at this grid's origin.  capacity None: the cells."""
        ctx = ctx or self.ctx
        cap = self.cells if capacity is None else int(capacity)
        idx, lo = np.empty(cap, np.int64), np.empty(cap, np.float32)
        count = C.c_size_t()
        h = C.c_void_p()
        check(load().sga_occupancy_export(ctx.h, self.h, float(threshold), _state_mask(which, "which"), cap, idx.ctypes.data_as(C.POINTER(C.c_int64)) if cap else None, _fp(lo) if cap else None, C.byref(count),
                                          C.byref(h) if return_cloud else None))
        m = min(count.value, cap)
        res = {"count": count.value, "indices": idx[:m].copy(), "log_odds": lo[:m].copy()}
        if return_cloud:
            res["cloud"] = PointCloud(ctx=ctx, _handle=h)
        return res

    def occupied_cloud(self, threshold=0.0, ctx=None):
        """The PointCloud of the centres of the occupied cells."""
        ctx = ctx or self.ctx
        count = C.c_size_t()
        h = C.c_void_p()
        check(load().sga_occupancy_export(ctx.h, self.h, float(threshold), OCCUPANCY_STATES["occupied"], self.cells, None, None, C.byref(count), C.byref(h)))
        return PointCloud(ctx=ctx, _handle=h)

    def download(self, ctx=None):
        """The raw arrays: (stamp (nz, ny, nx) uint32, log-odds (nz, ny, nx) float32)."""
        shape = (self.dims[2], self.dims[1], self.dims[0])
        stamp, lo = np.empty(shape, np.uint32), np.empty(shape, np.float32)
        check(load().sga_occupancy_download((ctx or self.ctx).h, self.h, stamp.ctypes.data_as(C.POINTER(C.c_uint32)), _fp(lo)))
        return stamp, lo


def occupancy_launches():
    """Diagnostics (sga_debug_occupancy_launches): commands enqueued so far by the OccupancyGrid calls (create two, clear one, integrate
    two — one with mode 1 —, classify one plus the compaction's two, stats one, export one plus two when it fills)."""
    return _launches("sga_debug_occupancy_launches")


def occupancy_waits():
    """Diagnostics (sga_debug_occupancy_waits): host waits so far of the OccupancyGrid calls (integrate: none, one with statistics)."""
    return _launches("sga_debug_occupancy_waits")


def _launches(name):
    v = C.c_ulonglong()
    check(getattr(load(), name)(C.byref(v)))
    return v.value


CLUSTER_ROW_DTYPE = np.dtype([("seed", np.int64), ("size", np.int64), ("lo", np.float64, (3,)), ("hi", np.float64, (3,))])  # sga_cluster_row
_CLUSTER_KEEP = {None: 0, "clustered": 1, "rest": 2}


def _cluster_params(radius=0.5, min_points=1, min_size=1, max_size=None, keep=None):
    """The sga_cluster_params of PointCloud.clusters' arguments (one is passed through).  The library judges the values."""
    if isinstance(radius, _lib.ClusterParams):
        return radius
    if keep not in _CLUSTER_KEEP:
        raise ValueError('keep must be None, "clustered" or "rest"')
    p = _lib.ClusterParams()
    load().sga_cluster_params_default(C.byref(p))
    p.radius, p.min_points, p.min_size, p.max_size, p.keep = float(radius), int(min_points), int(min_size), 0 if max_size is None else int(max_size), _CLUSTER_KEEP[keep]
    return p


def cluster_cloud(points, radius, min_points=1, min_size=1, max_size=None, tree=None, keep=None, return_table=True, table_capacity=None):
    """PointCloud.clusters of a PointCloud or of an (N,3|4) array (uploaded first)."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    return cloud.clusters(radius, min_points, min_size, max_size, tree, keep, return_table, table_capacity)


def cloud_cluster_launches():
    """Diagnostics (sga_debug_cloud_cluster_launches): commands enqueued so far by PointCloud.clusters — six per call, eight with
    min_points > 1, two more when a cloud is made; the build of a temporary tree is not counted."""
    return _launches("sga_debug_cloud_cluster_launches")


def radius_search_launches():
    """Diagnostics (sga_debug_radius_search_launches): commands enqueued so far by KdTree.radius_search — two per call for the counts,
    five with lists that fit."""
    return _launches("sga_debug_radius_search_launches")


def radius_waits():
    """Diagnostics (sga_debug_radius_waits): host waits so far of PointCloud.clusters (one per call) and KdTree.radius_search (one; two
    with lists)."""
    return _launches("sga_debug_radius_waits")


_PLANE_KEEP = {None: 0, "plane": 1, "rest": 2}


def _plane_params(distance_threshold=0.1, iterations=1000, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, keep=None):
    """The sga_plane_params of PointCloud.segment_plane's arguments (one is passed through).  The library judges the values."""
    if isinstance(distance_threshold, _lib.PlaneParams):
        return distance_threshold
    if keep not in _PLANE_KEEP:
        raise ValueError('keep must be None, "plane" or "rest"')
    p = _lib.PlaneParams()
    load().sga_plane_default(C.byref(p))
    p.distance_threshold, p.iterations, p.seed = float(distance_threshold), int(iterations), int(seed) & 0xFFFFFFFFFFFFFFFF
    ax = (0.0, 0.0, 0.0) if axis is None else tuple(float(v) for v in np.asarray(axis, dtype=np.float64).reshape(3))
    p.axis[0], p.axis[1], p.axis[2] = ax
    p.max_angle, p.min_inliers, p.refit, p.keep = float(max_angle), int(min_inliers), int(refit), _PLANE_KEEP[keep]
    return p


def segment_plane(points, distance_threshold=0.1, iterations=1000, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True, keep=None, return_kept=False, return_scores=False):
    """PointCloud.segment_plane of a PointCloud or of an (N,3|4) array (uploaded first)."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    return cloud.segment_plane(distance_threshold, iterations, seed, axis, max_angle, min_inliers, refit, keep, return_kept, return_scores)


def segment_planes(points, max_planes, distance_threshold=0.1, iterations=1000, seed=0, axis=None, max_angle=0.0, min_inliers=3, refit=True):
    """Up to max_planes planes of a PointCloud or an (N,3|4) array, one after the other (a host loop): round r
    calls segment_plane with seed + r and keep "rest" on what round r - 1 left, and stops at the first round that finds fewer than
    min_inliers points.  Returns a dict: "labels" (numpy int32 over the ORIGINAL cloud: the round that took the point, -1 for none),
    "planes" (a list of segment_plane's dicts without their clouds, in the order found), "rest" (the PointCloud left over) and
    "rest_indices" (numpy int64: its points' indices in the original cloud)."""
    rest = points if isinstance(points, PointCloud) else PointCloud(points)
    index = np.arange(rest.size(), dtype=np.int64)
    labels = np.full(rest.size(), -1, np.int32)
    planes = []
    for r in range(int(max_planes)):
        res = rest.segment_plane(distance_threshold, iterations, (int(seed) + r) & 0xFFFFFFFFFFFFFFFF, axis, max_angle, min_inliers, refit, "rest", True)
        if res["inliers"] < int(min_inliers):
            break
        taken = np.ones(len(index), bool)
        taken[res["kept"]] = False
        labels[index[taken]] = r
        index, rest = index[res["kept"]], res.pop("cloud")
        res.pop("kept")
        planes.append(res)
    return {"labels": labels, "planes": planes, "rest": rest, "rest_indices": index}


def segment_plane_launches():
    """Diagnostics (sga_debug_segment_plane_launches): commands enqueued so far by PointCloud.segment_plane — four per call, five when the
    refit succeeded or a cloud is made, two more (the compaction) with a cloud."""
    return _launches("sga_debug_segment_plane_launches")


def segment_plane_waits():
    """Diagnostics (sga_debug_segment_plane_waits): host waits so far of PointCloud.segment_plane (one; two when the refit succeeded or a
    cloud is made)."""
    return _launches("sga_debug_segment_plane_waits")


def cloud_fpfh_launches():
    """Diagnostics (sga_debug_cloud_fpfh_launches): commands enqueued so far by PointCloud.fpfh (three per call)."""
    return _launches("sga_debug_cloud_fpfh_launches")


def features_match_launches():
    """Diagnostics (sga_debug_features_match_launches): commands enqueued so far by match_features (two per call, three with mutual)."""
    return _launches("sga_debug_features_match_launches")


def ransac_launches():
    """Diagnostics (sga_debug_ransac_launches): commands enqueued so far by ransac_correspondences (four per call)."""
    return _launches("sga_debug_ransac_launches")


def _overlap_params(max_distance=1.0, keep=None):
    """The sga_overlap of PointCloud.overlap's arguments (one is passed through).  The library judges the values."""
    if isinstance(max_distance, _lib.OverlapParams):
        return max_distance
    if keep not in _OVERLAP_KEEP:
        raise ValueError('keep must be None, "matched" or "unmatched"')
    p = _lib.OverlapParams()
    load().sga_overlap_default(C.byref(p))
    p.max_distance, p.keep = float(max_distance), _OVERLAP_KEEP[keep]
    return p


def cloud_overlap(points, target, T=None, max_distance=1.0, keep=None, return_dist=False, return_nearest=False, return_kept=False, ctx=None):
    """PointCloud.overlap of a PointCloud or of an (N,3|4) array (uploaded first)."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    return cloud.overlap(target, T, max_distance, keep, return_dist, return_nearest, return_kept, ctx)


def cloud_overlap_launches():
    """Diagnostics (sga_debug_cloud_overlap_launches): commands enqueued so far by PointCloud.overlap (the distances and the sums; with
    an output cloud also the compaction's table copy and the compaction)."""
    v = C.c_ulonglong()
    check(load().sga_debug_cloud_overlap_launches(C.byref(v)))
    return v.value


_VISIBILITY_KEEP = {None: 0, "seen_through": 1, "rest": 2}


def _visibility_params(keep=None, **fields):
    """The sga_visibility of PointCloud.visibility's keyword arguments over the library's defaults.  The library judges the values."""
    if keep not in _VISIBILITY_KEEP:
        raise ValueError('keep must be None, "seen_through" or "rest"')
    p = _lib.VisibilityParams()
    load().sga_visibility_default(C.byref(p))
    for name, value in fields.items():
        if name not in ("width", "height", "fov_up", "fov_down", "min_range", "max_range", "margin", "margin_ratio", "window_h", "window_v"):
            raise TypeError("visibility has no parameter %r" % name)
        setattr(p, name, int(value) if name in ("width", "height", "window_h", "window_v") else float(value))
    p.keep = _VISIBILITY_KEEP[keep]
    return p


def cloud_visibility(map_points, scan_points, T=None, **kw):
    """PointCloud.visibility of PointClouds or of (N,3|4) arrays (uploaded first): the map, the scan, the pose, the keyword arguments."""
    cloud = map_points if isinstance(map_points, PointCloud) else PointCloud(map_points)
    scan = scan_points if isinstance(scan_points, PointCloud) else PointCloud(scan_points)
    return cloud.visibility(scan, T, **kw)


def cloud_visibility_launches():
    """Diagnostics (sga_debug_cloud_visibility_launches): commands enqueued so far by PointCloud.visibility (the fill, the image, the
    states, the counts; with an output cloud also the compaction's table copy and the compaction)."""
    v = C.c_ulonglong()
    check(load().sga_debug_cloud_visibility_launches(C.byref(v)))
    return v.value


def crop_clouds(clouds, crops, return_kept=False, ctx=None):
    """sga_cloud_crop_batch: PointCloud.cropped for B clouds — crops[k] a dict of cropped()'s keyword arguments (min_range, max_range,
    center, box, box_mode), or one dict for all — by one table copy and one launch, whatever B is.  Returns the B cropped clouds, or
    (clouds, kept) with kept[k] the numpy int64 indices kept of clouds[k].  The members may belong to several contexts of one device;
    ctx: the context the call runs on (default: the first cloud's)."""
    clouds = list(clouds)
    for c in clouds:
        if not isinstance(c, PointCloud):
            raise TypeError("crop_clouds takes PointCloud objects")
    B = len(clouds)
    crops = [crops] * B if isinstance(crops, (dict, _lib.Crop)) else list(crops)
    if len(crops) != B:
        raise ValueError(f"{len(crops)} crops for {B} clouds")
    if B == 0:
        return ([], []) if return_kept else []  # (count == 0 is no device work: no context is needed)
    cs = (_lib.Crop * B)(*[c if isinstance(c, _lib.Crop) else _crop(**c) for c in crops])
    ctx = ctx or clouds[0].ctx
    hs = (C.c_void_p * B)(*[c.h.value for c in clouds])
    kept = [np.empty(c.size(), np.int64) for c in clouds] if return_kept else None
    kp = None if kept is None else (C.c_void_p * B)(*[k.ctypes.data if len(k) else None for k in kept])
    out = (C.c_void_p * B)()
    check(load().sga_cloud_crop_batch(ctx.h, hs, cs, kp, B, out))
    res = [PointCloud(ctx=ctx, _handle=C.c_void_p(out[k])) for k in range(B)]
    return (res, [kept[k][: res[k].size()].copy() for k in range(B)]) if return_kept else res


def random_sampling_indices(n, num_samples, seed=None):
    """The choice behind random_sampling: num_samples distinct indices of range(n) in ascending order (util/downsampling.hpp: std::sample
    keeps the input's order), the same for the same seed; every index when num_samples >= n.  Pure host code."""
    n, num_samples = int(n), int(num_samples)
    if num_samples < 0:
        raise ValueError("num_samples must not be negative")
    if num_samples >= n:
        return np.arange(n, dtype=np.int64)
    return np.sort(np.random.default_rng(seed).choice(n, size=num_samples, replace=False)).astype(np.int64)


def random_sampling(points, num_samples, seed=None):
    """util/downsampling.hpp random_sampling: num_samples points of the cloud chosen at random, in the input's order, with their normals
    and covariances — the host picks the indices (random_sampling_indices), one PointCloud.selected follows.  num_samples >= size: the
    cloud as it is."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    n = cloud.size()
    if int(num_samples) >= n:
        return cloud
    return cloud.selected(random_sampling_indices(n, num_samples, seed))


def cloud_crop_launches():
    """Diagnostics (sga_debug_cloud_crop_launches): table copies and kernels enqueued so far by PointCloud.cropped / crop_clouds."""
    v = C.c_ulonglong()
    check(load().sga_debug_cloud_crop_launches(C.byref(v)))
    return v.value


def cloud_deskew_launches():
    """Diagnostics (sga_debug_cloud_deskew_launches): table copies and kernels enqueued so far by PointCloud.deskewed / deskew_clouds."""
    v = C.c_ulonglong()
    check(load().sga_debug_cloud_deskew_launches(C.byref(v)))
    return v.value


def cloud_merge_launches():
    """Diagnostics (sga_debug_cloud_merge_launches): table copies and kernels enqueued so far by merge_clouds / PointCloud.transformed."""
    v = C.c_ulonglong()
    check(load().sga_debug_cloud_merge_launches(C.byref(v)))
    return v.value


def voxelmap_batch_launches():
    """Diagnostics (sga_debug_voxelmap_batch_launches): kernels, sorts, scans and copy commands enqueued so far by the shared chain of
    build_gaussian_voxelmaps."""
    v = C.c_ulonglong()
    check(load().sga_debug_voxelmap_batch_launches(C.byref(v)))
    return v.value


def _insert_members(maps, clouds):
    maps, clouds = list(maps), list(clouds)
    if len(maps) != len(clouds):
        raise ValueError(f"{len(maps)} maps for {len(clouds)} clouds")
    for m in maps:
        if not isinstance(m, (GaussianVoxelMap, _FlatVoxelMap)):
            raise TypeError("insert_batch takes GaussianVoxelMap / IncrementalVoxelMap* objects")
    ctx = _one_context(clouds)
    if maps and any(m.ctx is not maps[0].ctx for m in maps):
        raise ValueError("the maps of a batch must belong to one context")
    ms = (C.c_void_p * max(1, len(maps)))(*[m.h.value for m in maps])
    cs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    return maps, clouds, (maps[0].ctx if maps else ctx), ms, cs


def insert_batch(maps, clouds, Ts=None):
    """sga_voxelmap_insert_batch: maps[k].insert(clouds[k], Ts[k]) for all k (Ts None: identities) — the maps of several scan-to-model
    streams updated by one chain of launches and one host wait.  Every map holds what the lone insert leaves, bit for bit.  Incremental
    GaussianVoxelMaps with clouds of at most 262144 points share the launches; flat maps, larger clouds and scans that span 65536 or more
    voxels along an axis are inserted one by one inside the call.  A map may appear once per call, a cloud several times."""
    maps, clouds, ctx, ms, cs = _insert_members(maps, clouds)
    t16 = None if Ts is None else _T16s(Ts, len(maps))
    check(load().sga_voxelmap_insert_batch(ctx.h, ms, cs, None if t16 is None else _dp(t16), len(maps)))


def _voxelmap_insert_batch_plan(maps, clouds):
    """Diagnostics (sga_debug_voxelmap_insert_batch_plan): what insert_batch(maps, clouds) would do — forest (members of the shared chain),
    lone (members through the lone routine), empty (Gaussian maps given an empty cloud), member_bits, end_bit of the chain's sort, points
    of the concatenation."""
    maps, clouds, _, ms, cs = _insert_members(maps, clouds)
    out = (C.c_int * 6)()
    check(load().sga_debug_voxelmap_insert_batch_plan(ms, cs, len(maps), out))
    return {"forest": out[0], "lone": out[1], "empty": out[2], "member_bits": out[3], "end_bit": out[4], "points": out[5]}


def voxelmap_insert_batch_launches():
    """Diagnostics (sga_debug_voxelmap_insert_batch_launches): kernels, sorts, scans and table copies enqueued so far by the shared chain
    of insert_batch."""
    v = C.c_ulonglong()
    check(load().sga_debug_voxelmap_insert_batch_launches(C.byref(v)))
    return v.value


def _voxelgrid_batch_plan(clouds, resolution):
    """Diagnostics (sga_debug_voxelgrid_batch_plan): what voxelgrid_sampling_batch(clouds, resolution) would do — key_bytes (4 / 8; 0: no
    shared chain), W (bits below the member number), member_bits, forest (members of the shared chain), lone (members through the lone
    routine; empty members are in neither), tiles of the runs kernel."""
    clouds = list(clouds)
    _one_context(clouds)
    hs = (C.c_void_p * max(1, len(clouds)))(*[c.h.value for c in clouds])
    out = (C.c_int * 6)()
    check(load().sga_debug_voxelgrid_batch_plan(hs, len(clouds), float(resolution), out))
    return {"key_bytes": out[0], "W": out[1], "member_bits": out[2], "forest": out[3], "lone": out[4], "tiles": out[5]}


def voxelgrid_batch_launches():
    """Diagnostics (sga_debug_voxelgrid_batch_launches): kernels and sorts enqueued so far by the shared chain of voxelgrid_sampling_batch."""
    v = C.c_ulonglong()
    check(load().sga_debug_voxelgrid_batch_launches(C.byref(v)))
    return v.value


def forest_launches():
    """Diagnostics (sga_debug_forest_launches): kernels enqueued so far by the forest form of the two batched preprocessing calls."""
    v = C.c_ulonglong()
    check(load().sga_debug_forest_launches(C.byref(v)))
    return v.value


def preprocess_points(points, downsampling_resolution=0.25, num_neighbors=10, num_threads=1):
    """registration_helper.cpp:22-34: downsample -> index -> normals + covariances.  Returns (PointCloud, KdTree)."""
    cloud = points if isinstance(points, PointCloud) else PointCloud(points)
    down = voxelgrid_sampling(cloud, downsampling_resolution)
    tree = KdTree(down)  # (built first: the estimation searches it and fills its kd-ordered attribute copies — one build, not two)
    estimate_normals_covariances(down, tree, num_neighbors)
    return down, tree


def align(
    target,
    source,
    target_tree=None,
    init_T_target_source=None,
    registration_type="GICP",
    voxel_resolution=1.0,
    downsampling_resolution=0.25,
    max_correspondence_distance=1.0,
    num_threads=1,
    max_iterations=20,
    verbose=False,
    **kw,
):
    """small_gicp.align (src/python/align.cpp:22-295), three call forms:
    align(target_numpy, source_numpy, ...)            -> preprocess both, then register          (registration_helper.cpp:57-69)
    align(target_cloud, source_cloud, target_tree)    -> ICP / PLANE_ICP / GICP                    (registration_helper.cpp:81-122)
    align(target_voxelmap, source_cloud)              -> VGICP                                      (registration_helper.cpp:125-137)
    """
    if isinstance(target, GaussianVoxelMap):
        # the Python binding's voxel-map overload DOES apply max_correspondence_distance (src/python/align.cpp:246), unlike the C++
        # helper align(GaussianVoxelMap, ...) of registration_helper.cpp:125-137 (mirrored in include/small_gicp_amd.hpp), which
        # leaves the rejector at 1.0 m^2: each layer mirrors its own counterpart
        setting = make_setting("GICP", max_correspondence_distance, max_iterations, verbose=verbose, **kw)
        return Problem(target, source, init_T_target_source).align(setting, init_T_target_source)
    if not isinstance(target, PointCloud):
        tgt, tree = preprocess_points(np.asarray(target), downsampling_resolution, 10)
        src, _ = preprocess_points(np.asarray(source), downsampling_resolution, 10)
        if registration_type == "VGICP":
            vm = GaussianVoxelMap(voxel_resolution, ctx=tgt.ctx)
            vm.insert(tgt)
            # registration_helper.cpp:130-136 leaves the rejector at its default 1.0 m^2 for VGICP
            setting = make_setting("GICP", 1.0, max_iterations, verbose=verbose, **kw)
            return Problem(vm, src, init_T_target_source).align(setting, init_T_target_source)
        target, source, target_tree = tgt, src, tree
    if target_tree is None:
        target_tree = KdTree(target)
    target_tree.refresh_attributes()
    setting = make_setting(registration_type, max_correspondence_distance, max_iterations, verbose=verbose, **kw)
    return Problem(target_tree, source, init_T_target_source).align(setting, init_T_target_source)


# ---- sweep registration: the pose and the twist of a raw sweep at once ------------------------------------------
class SweepResult:
    """sga_sweep_result: T_target_source (4x4, target <- sensor at ref_time), twist (6,), converged, iterations, num_inliers, H (12x12)
    and b (12) of the last linearization (order [pose | twist], the prior included) and error."""

    def __init__(self, rc=None):
        if rc is None:
            self.T_target_source, self.twist = np.eye(4), np.zeros(6)
            self.converged, self.iterations, self.num_inliers = False, 0, 0
            self.H, self.b, self.error = np.zeros((12, 12)), np.zeros(12), 0.0
        else:
            self.T_target_source = np.array(rc.T_target_source).reshape(4, 4).T.copy()
            self.twist = np.array(rc.twist)
            self.converged = bool(rc.converged)
            self.iterations = int(rc.iterations)
            self.num_inliers = int(rc.num_inliers)
            self.H = np.array(rc.H).reshape(12, 12)
            self.b = np.array(rc.b)
            self.error = float(rc.error)

    def __repr__(self):
        return f"SweepResult(converged={self.converged}, iterations={self.iterations}, num_inliers={self.num_inliers}, error={self.error:.6g})"


def _sweep_inputs(target, source, times, target_tree, registration_type):
    """The clouds, the tree and the times of a sweep call.  Arrays are uploaded as they are (no voxel grid: it cannot carry times) and
    given what the factor needs (10 neighbours, as align's preprocessing); PointClouds are taken as they are."""
    kind = _FACTOR_BY_NAME[registration_type] if isinstance(registration_type, str) else int(registration_type)
    made_target = not isinstance(target, PointCloud)
    if made_target:
        target = PointCloud(np.asarray(target))
    if not isinstance(source, PointCloud):
        source = PointCloud(np.asarray(source), ctx=target.ctx)
        if kind == GICP and source.size() > 0:
            estimate_covariances(source, None, 10)
    if target_tree is None:
        target_tree = KdTree(target)
        if made_target and target.size() > 0 and kind != ICP:
            _estimate(target, target_tree, 10, 3)
    target_tree.refresh_attributes()
    t = np.ascontiguousarray(np.asarray(times, dtype=np.float32).reshape(-1))
    if len(t) != source.size():
        raise ValueError(f"{len(t)} times for a cloud of {source.size()} points")
    if len(t) == 0:
        t = np.zeros(1, np.float32)  # (a pointer that is not NULL; nothing is read)
    return target_tree, source, t


def _twist6(twist):
    return np.zeros(6) if twist is None else np.ascontiguousarray(np.asarray(twist, dtype=np.float64).reshape(6))


def linearize_sweep(target, source, times, target_tree=None, T=None, twist=None, ref_time=1.0, registration_type="GICP", max_correspondence_distance=1.0, setting=None, return_nearest=True):
    """sga_sweep_linearize at the state (T, twist): (H (12,12), b (12,), e, num_inliers, nearest) — nearest (N,) int64, the pair's index
    in the target's own order, -1 without a pair (None with return_nearest=False)."""
    tree, source, t = _sweep_inputs(target, source, times, target_tree, registration_type)
    fp = setting.factor if setting is not None else make_setting(registration_type, max_correspondence_distance).factor
    H, b = np.empty(144), np.empty(12)
    e, ninl = C.c_double(), C.c_uint64()
    nearest = np.empty(source.size(), np.int64) if return_nearest else None
    t16, xi = _T16(np.eye(4) if T is None else T), _twist6(twist)
    check(load().sga_sweep_linearize(source.ctx.h, tree.h, source.h, _fp(t), C.byref(fp), _dp(t16), _dp(xi), float(ref_time), _dp(H), _dp(b), C.byref(e), C.byref(ninl),
                                     nearest.ctypes.data_as(C.POINTER(C.c_int64)) if return_nearest and source.size() > 0 else None))
    return H.reshape(12, 12), b, e.value, ninl.value, nearest


def sweep_error(target, source, times, target_tree=None, T=None, twist=None, ref_time=1.0, registration_type="GICP", max_correspondence_distance=1.0, setting=None):
    """sga_sweep_error: e at (T, twist) over the pairs of the last linearize_sweep of the same target_tree and source (pass the same
    PointCloud and KdTree objects: arrays would be uploaded again, and be another source)."""
    tree, source, t = _sweep_inputs(target, source, times, target_tree, registration_type)
    fp = setting.factor if setting is not None else make_setting(registration_type, max_correspondence_distance).factor
    e = C.c_double()
    t16, xi = _T16(np.eye(4) if T is None else T), _twist6(twist)
    check(load().sga_sweep_error(source.ctx.h, tree.h, source.h, _fp(t), C.byref(fp), _dp(t16), _dp(xi), float(ref_time), C.byref(e)))
    return e.value


def _sweep_params(ref_time=1.0, twist_prior=None, twist_information=None):
    p = _lib.SweepParams()
    load().sga_sweep_params_default(C.byref(p))
    p.ref_time = float(ref_time)
    if twist_prior is not None:
        for k, v in enumerate(np.asarray(twist_prior, dtype=np.float64).reshape(6)):
            p.twist_prior[k] = float(v)
    if twist_information is not None:
        for k, v in enumerate(np.asarray(twist_information, dtype=np.float64).reshape(36)):
            p.twist_information[k] = float(v)
    return p


def align_sweep(target, source, times, target_tree=None, init_T=None, init_twist=None, ref_time=1.0, registration_type="GICP", max_correspondence_distance=1.0, twist_prior=None, twist_information=None, setting=None):
    """The pose (target <- sensor at ref_time) and the twist (the sensor's motion per unit of time, [rx ry rz tx ty tz]) of the raw sweep
    `source` — point i measured at times[i] in the sensor frame of that instant — against `target`, estimated together
    (sga_align_sweep): a SweepResult.  twist_prior / twist_information (6,) / (6,6): a Gaussian prior on the twist; None: none.
    target / source: PointClouds (with target_tree, or a tree is built) or arrays, which are uploaded as they are."""
    tree, source, t = _sweep_inputs(target, source, times, target_tree, registration_type)
    st = setting if setting is not None else make_setting(registration_type, max_correspondence_distance)
    p = _sweep_params(ref_time, twist_prior, twist_information)
    rc = _lib.SweepResultC()
    t16 = None if init_T is None else _T16(init_T)
    xi = None if init_twist is None else _twist6(init_twist)
    check(load().sga_align_sweep(source.ctx.h, tree.h, source.h, _fp(t), _dp(t16), _dp(xi), C.byref(st), C.byref(p), C.byref(rc)))
    return SweepResult(rc)


def sweep_launches():
    """Diagnostics (sga_debug_sweep_launches): launches enqueued so far by the sweep calls, two per pass."""
    return _launches("sga_debug_sweep_launches")

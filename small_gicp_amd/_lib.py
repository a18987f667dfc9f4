"""ctypes binding of libsmall_gicp_amd.so (the C-ABI declared in include/small_gicp_amd.h).

The product path has NO CPU fallback: if the library is missing or there is no gfx950 device, calls raise.
"""
import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SGA_LIB_PATH") or os.path.join(_HERE, "lib", "libsmall_gicp_amd.so")

SGA_OK = 0
ICP, PLANE_ICP, GICP = 0, 1, 2
FLAT_NORMALS, FLAT_COVS = 1, 2  # contents of a flat voxel map (sga_flatmap_create_contents)
ROBUST_NONE, ROBUST_HUBER, ROBUST_CAUCHY = 0, 1, 2
LEVENBERG_MARQUARDT, GAUSS_NEWTON = 0, 1
MATH_FP32, MATH_FP64 = 0, 1
ACCUM_DOUBLES = 30


class SgaError(RuntimeError):
    pass


class FactorParams(C.Structure):
    _fields_ = [("factor_kind", C.c_int), ("robust_kind", C.c_int), ("robust_c", C.c_double), ("max_dist_sq", C.c_double), ("math_mode", C.c_int)]


class RegistrationSettingC(C.Structure):
    _fields_ = [
        ("factor", FactorParams),
        ("optimizer", C.c_int),
        ("max_iterations", C.c_int),
        ("max_inner_iterations", C.c_int),
        ("init_lambda", C.c_double),
        ("lambda_factor", C.c_double),
        ("gn_lambda", C.c_double),
        ("translation_eps", C.c_double),
        ("rotation_eps", C.c_double),
        ("verbose", C.c_int),
        ("restrict_dof_lambda", C.c_double),
        ("restrict_dof_mask", C.c_double * 6),
    ]


class ResultC(C.Structure):
    _fields_ = [
        ("T_target_source", C.c_double * 16),
        ("converged", C.c_int),
        ("iterations", C.c_uint64),
        ("num_inliers", C.c_uint64),
        ("H", C.c_double * 36),
        ("b", C.c_double * 6),
        ("error", C.c_double),
    ]


class SweepParams(C.Structure):
    """sga_sweep_params: ref_time, the prior on the twist and its information (row-major 6 x 6; all zero: no prior)."""

    _fields_ = [("ref_time", C.c_double), ("twist_prior", C.c_double * 6), ("twist_information", C.c_double * 36)]


class SweepResultC(C.Structure):
    """sga_sweep_result"""

    _fields_ = [
        ("T_target_source", C.c_double * 16),
        ("twist", C.c_double * 6),
        ("converged", C.c_int),
        ("iterations", C.c_uint64),
        ("num_inliers", C.c_uint64),
        ("H", C.c_double * 144),
        ("b", C.c_double * 12),
        ("error", C.c_double),
    ]


REJECTOR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER(C.c_ubyte))
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_size_t)  # sga_allreduce_fn
LINEARIZE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64))
ERROR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))

# sga_batch_linearize_fn / sga_batch_error_fn: (user, count, active, T, H, b, e, num_inliers) / (user, count, active, T, e)
BATCH_LINEARIZE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64))
BATCH_ERROR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_ubyte), C.POINTER(C.c_double), C.POINTER(C.c_double))

class DeviceArray(C.Structure):
    """sga_device_array: strided rows in device memory (data, dtype F32 | F64, cols, stride in elements)."""

    _fields_ = [("data", C.c_void_p), ("dtype", C.c_int), ("cols", C.c_int), ("stride", C.c_int)]


class Crop(C.Structure):
    """sga_crop: the predicate of sga_cloud_crop (center, min_range, max_range, box_lo, box_hi, box_mode 0 none | 1 inside | 2 outside)."""

    _fields_ = [("center", C.c_double * 3), ("min_range", C.c_double), ("max_range", C.c_double), ("box_lo", C.c_double * 3), ("box_hi", C.c_double * 3), ("box_mode", C.c_int), ("pad", C.c_int)]


class OutlierFilter(C.Structure):
    """sga_outlier_filter: mode 0 statistical (k, std_mul) | 1 radius (k neighbours within radius)."""

    _fields_ = [("mode", C.c_int), ("k", C.c_int), ("std_mul", C.c_double), ("radius", C.c_double)]


class OutlierStats(C.Structure):
    """sga_outlier_stats: mean, stddev and threshold of the per-point statistic, and the number of points kept."""

    _fields_ = [("mean", C.c_double), ("stddev", C.c_double), ("threshold", C.c_double), ("kept", C.c_size_t)]


class OverlapParams(C.Structure):
    """sga_overlap: max_distance, keep 0 none | 1 the matched | 2 the unmatched."""

    _fields_ = [("max_distance", C.c_double), ("keep", C.c_int), ("reserved", C.c_int)]


class OverlapStats(C.Structure):
    """sga_overlap_stats: points, matched, fitness = matched / points, rmse and mean_distance over the matched."""

    _fields_ = [("points", C.c_size_t), ("matched", C.c_size_t), ("fitness", C.c_double), ("rmse", C.c_double), ("mean_distance", C.c_double)]


class VisibilityParams(C.Structure):
    """sga_visibility: the range image (width x height over [fov_down, fov_up], radians), the ranges, the margin, the window, keep 0 none |
    1 the seen-through | 2 all the others."""

    _fields_ = [("width", C.c_int), ("height", C.c_int), ("fov_up", C.c_double), ("fov_down", C.c_double), ("min_range", C.c_double), ("max_range", C.c_double), ("margin", C.c_double),
                ("margin_ratio", C.c_double), ("window_h", C.c_int), ("window_v", C.c_int), ("keep", C.c_int), ("reserved", C.c_int)]


class VisibilityStats(C.Structure):
    """sga_visibility_stats: points and the number in each state."""

    _fields_ = [("points", C.c_size_t), ("unobserved", C.c_size_t), ("consistent", C.c_size_t), ("occluded", C.c_size_t), ("seen_through", C.c_size_t)]


class Ransac(C.Structure):
    """sga_ransac: max_distance, iterations (1 .. 2^32 - 1), seed, edge_similarity (0: off), min_edge."""

    _fields_ = [("max_distance", C.c_double), ("iterations", C.c_uint64), ("seed", C.c_uint64), ("edge_similarity", C.c_double), ("min_edge", C.c_double)]


class RansacResult(C.Structure):
    """sga_ransac_result: inliers and inlier_rmse of the best hypothesis, its number, the hypotheses that passed the tests, refit 0 | 1."""

    _fields_ = [("inliers", C.c_uint64), ("inlier_rmse", C.c_double), ("best_hypothesis", C.c_uint64), ("scored", C.c_uint64), ("refit", C.c_int), ("reserved", C.c_int)]


class PlaceParams(C.Structure):
    """sga_place_params: rings, sectors, max_range, height of a Scan Context descriptor."""

    _fields_ = [("rings", C.c_int), ("sectors", C.c_int), ("max_range", C.c_double), ("height", C.c_double)]


class PlaceMatch(C.Structure):
    """sga_place_match: the index of a database entry, its best column shift and its distance."""

    _fields_ = [("index", C.c_int64), ("shift", C.c_int32), ("reserved", C.c_int32), ("distance", C.c_double)]


class RadiusResult(C.Structure):
    """sga_radius_result: the sum of the counts, the list entries written, overflow 0 | 1 (lists asked for and total > capacity)."""

    _fields_ = [("total", C.c_uint64), ("written", C.c_uint64), ("overflow", C.c_int), ("reserved", C.c_int)]


class ClusterParams(C.Structure):
    """sga_cluster_params: radius (eps), min_points, keep 0 none | 1 the clustered | 2 the rest, min_size, max_size (0: no limit)."""

    _fields_ = [("radius", C.c_double), ("min_points", C.c_int), ("keep", C.c_int), ("min_size", C.c_int64), ("max_size", C.c_int64)]


class ClusterResult(C.Structure):
    """sga_cluster_result: clusters kept, noise points, points of dropped clusters, table rows written."""

    _fields_ = [("clusters", C.c_uint64), ("noise", C.c_uint64), ("dropped", C.c_uint64), ("rows", C.c_uint64)]


class ClusterRow(C.Structure):
    """sga_cluster_row: a cluster's seed (its lowest core index), size and box."""

    _fields_ = [("seed", C.c_int64), ("size", C.c_int64), ("lo", C.c_double * 3), ("hi", C.c_double * 3)]


class PlaneParams(C.Structure):
    """sga_plane_params: distance_threshold, iterations (1 .. 2^20), seed, axis (zeros: none), max_angle, min_inliers, refit 0 | 1,
    keep 0 none | 1 the plane's points | 2 the rest."""

    _fields_ = [("distance_threshold", C.c_double), ("iterations", C.c_uint64), ("seed", C.c_uint64), ("axis", C.c_double * 3), ("max_angle", C.c_double), ("min_inliers", C.c_uint64),
                ("refit", C.c_int), ("keep", C.c_int)]


class PlaneResult(C.Structure):
    """sga_plane_result: the final plane's inliers and their rmse, the best hypothesis' score and number, the hypotheses scored, refit 0 | 1."""

    _fields_ = [("inliers", C.c_uint64), ("rmse", C.c_double), ("hypothesis_inliers", C.c_uint64), ("best_hypothesis", C.c_uint64), ("scored", C.c_uint64), ("refit", C.c_int), ("reserved", C.c_int)]


class IssParams(C.Structure):
    """sga_iss_params: salient_radius, non_max_radius (no defaults), gamma_21, gamma_32 in (0, 1], min_neighbors >= 1, keep 0 none | 1 the keypoints."""

    _fields_ = [("salient_radius", C.c_double), ("non_max_radius", C.c_double), ("gamma_21", C.c_double), ("gamma_32", C.c_double), ("min_neighbors", C.c_int32), ("keep", C.c_int32)]


class OccupancyParams(C.Structure):
    """sga_occupancy_params: the box's minimum corner, the leaf, the dims (x, y, z), the fp32 log-odds of a hit and a miss and their clamps."""

    _fields_ = [("origin", C.c_double * 3), ("leaf", C.c_double), ("dims", C.c_int * 3), ("reserved", C.c_int), ("l_hit", C.c_float), ("l_miss", C.c_float), ("l_min", C.c_float), ("l_max", C.c_float)]


class OccupancyScanStats(C.Structure):
    """sga_occupancy_scan_stats: the returns of a scan by kind, and the cells it hit and freed."""

    _fields_ = [("beams", C.c_size_t), ("ignored", C.c_size_t), ("hits", C.c_size_t), ("truncated", C.c_size_t), ("cells_hit", C.c_size_t), ("cells_freed", C.c_size_t)]


class OccupancyCounts(C.Structure):
    """sga_occupancy_counts: points or cells per state, and the grid's epoch."""

    _fields_ = [("total", C.c_size_t), ("unknown", C.c_size_t), ("free", C.c_size_t), ("occupied", C.c_size_t), ("epoch", C.c_uint64)]


FPFH_DIM = 33
F32, F64 = 0, 1
REDUCE_MEAN, REDUCE_MIN, REDUCE_MAX, REDUCE_FIRST, REDUCE_NEAREST = 0, 1, 2, 3, 4  # SGA_REDUCE_*
IO_NO_ORDER, IO_RELATIVE = 1, 2
_da = C.POINTER(DeviceArray)

# every symbol include/small_gicp_amd.h and include/small_gicp_amd_debug.h declare: (name, restype, argtypes)
_vp, _dp, _fp = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_float)
_pvp = C.POINTER(C.c_void_p)
SYMBOLS = [
    ("sga_last_error", C.c_char_p, []),
    ("sga_version", C.c_char_p, []),
    ("sga_device_count", C.c_int, []),
    ("sga_allocator_stats", None, [C.POINTER(C.c_uint64)]),
    ("sga_context_create", C.c_int, [C.c_int, _pvp]),
    ("sga_context_create_on_stream", C.c_int, [C.c_int, _vp, _pvp]),
    ("sga_context_destroy", C.c_int, [_vp]),
    ("sga_context_synchronize", C.c_int, [_vp]),
    ("sga_context_stream", _vp, [_vp]),
    ("sga_cloud_create_f32", C.c_int, [_vp, _fp, _fp, _fp, C.c_size_t, _pvp]),
    ("sga_cloud_create_f64", C.c_int, [_vp, _dp, _dp, _dp, C.c_size_t, _pvp]),
    ("sga_cloud_create_f32_origin", C.c_int, [_vp, _fp, _fp, _fp, C.c_size_t, _dp, _pvp]),
    ("sga_cloud_create_f64_origin", C.c_int, [_vp, _dp, _dp, _dp, C.c_size_t, _dp, _pvp]),
    ("sga_cloud_origin", C.c_int, [_vp, _dp]),
    ("sga_index_origin", C.c_int, [_vp, _dp]),
    ("sga_choose_origin", None, [_dp, _dp, _dp]),
    ("sga_cloud_slice", C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _pvp]),
    ("sga_cloud_merge", C.c_int, [_vp, _pvp, _dp, C.c_size_t, _dp, _pvp]),
    ("sga_cloud_transform", C.c_int, [_vp, _vp, _dp, _dp, _pvp]),
    ("sga_debug_cloud_merge_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_cloud_deskew_batch", C.c_int, [_vp, _pvp, _pvp, _dp, _dp, C.c_size_t, _pvp]),
    ("sga_cloud_deskew", C.c_int, [_vp, _vp, _fp, _dp, C.c_double, _pvp]),
    ("sga_cloud_deskew_device", C.c_int, [_vp, _vp, C.POINTER(DeviceArray), _dp, C.c_double, _vp, C.c_int, _pvp]),
    ("sga_debug_cloud_deskew_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_crop_default", None, [C.POINTER(Crop)]),
    ("sga_cloud_crop_batch", C.c_int, [_vp, _pvp, C.POINTER(Crop), _pvp, C.c_size_t, _pvp]),
    ("sga_cloud_crop", C.c_int, [_vp, _vp, C.POINTER(Crop), C.POINTER(C.c_int64), _pvp]),
    ("sga_cloud_crop_device", C.c_int, [_vp, _vp, C.POINTER(Crop), _vp, _vp, C.c_int, _pvp]),
    ("sga_cloud_select", C.c_int, [_vp, _vp, C.POINTER(C.c_int64), C.c_size_t, _pvp]),
    ("sga_debug_cloud_crop_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_outlier_filter_default", None, [C.POINTER(OutlierFilter)]),
    ("sga_cloud_remove_outliers", C.c_int, [_vp, _vp, _vp, C.POINTER(OutlierFilter), C.POINTER(C.c_int64), _dp, C.POINTER(OutlierStats), _pvp]),
    ("sga_debug_cloud_outliers_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_overlap_default", None, [C.POINTER(OverlapParams)]),
    ("sga_cloud_overlap", C.c_int, [_vp, _vp, _vp, _dp, C.POINTER(OverlapParams), _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(OverlapStats), _pvp]),
    ("sga_debug_cloud_overlap_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_visibility_default", None, [C.POINTER(VisibilityParams)]),
    ("sga_cloud_visibility", C.c_int, [_vp, _vp, _vp, _dp, C.POINTER(VisibilityParams), C.POINTER(C.c_uint8), _dp, _dp, C.POINTER(C.c_int64), C.POINTER(VisibilityStats), _pvp]),
    ("sga_debug_cloud_visibility_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_features_create", C.c_int, [_vp, _fp, C.c_size_t, C.c_int, _pvp]),
    ("sga_features_size", C.c_int, [_vp, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("sga_features_download", C.c_int, [_vp, _vp, _fp]),
    ("sga_features_destroy", C.c_int, [_vp]),
    ("sga_features_create_device", C.c_int, [_vp, C.POINTER(DeviceArray), C.c_size_t, _vp, C.c_int, _pvp]),
    ("sga_features_export_device", C.c_int, [_vp, _vp, C.POINTER(DeviceArray), _vp, C.c_int]),
    ("sga_cloud_fpfh", C.c_int, [_vp, _vp, _vp, C.c_int, _dp, _pvp]),
    ("sga_features_match", C.c_int, [_vp, _vp, _vp, C.c_int, C.POINTER(C.c_int64), _dp, C.POINTER(C.c_size_t)]),
    ("sga_ransac_default", None, [C.POINTER(Ransac)]),
    ("sga_ransac_correspondences", C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int64), C.c_size_t, C.POINTER(Ransac), _dp, C.POINTER(RansacResult)]),
    ("sga_place_params_default", None, [C.POINTER(PlaceParams)]),
    ("sga_places_create", C.c_int, [_vp, C.POINTER(PlaceParams), _pvp]),
    ("sga_places_destroy", C.c_int, [_vp]),
    ("sga_places_size", C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    ("sga_places_params", C.c_int, [_vp, C.POINTER(PlaceParams)]),
    ("sga_places_add", C.c_int, [_vp, _vp, _vp, _dp, C.POINTER(C.c_size_t)]),
    ("sga_places_add_descriptor", C.c_int, [_vp, _vp, _fp, C.POINTER(C.c_size_t)]),
    ("sga_places_download", C.c_int, [_vp, _vp, C.c_size_t, C.c_size_t, _fp]),
    ("sga_cloud_scan_context", C.c_int, [_vp, _vp, C.POINTER(PlaceParams), _dp, _fp]),
    ("sga_places_query", C.c_int, [_vp, _vp, _vp, _dp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(PlaceMatch), C.POINTER(C.c_size_t), _dp, C.POINTER(C.c_int32)]),
    ("sga_places_query_descriptor", C.c_int, [_vp, _vp, _fp, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(PlaceMatch), C.POINTER(C.c_size_t), _dp, C.POINTER(C.c_int32)]),
    ("sga_debug_places_add_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_places_query_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_places_waits", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_index_radius_search", C.c_int, [_vp, _vp, _vp, C.c_double, C.c_size_t, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), _dp, C.POINTER(RadiusResult)]),
    ("sga_cluster_params_default", None, [C.POINTER(ClusterParams)]),
    ("sga_cloud_cluster", C.c_int, [_vp, _vp, _vp, C.POINTER(ClusterParams), C.POINTER(C.c_int32), C.POINTER(ClusterRow), C.c_size_t, C.POINTER(C.c_int64), C.POINTER(ClusterResult), _pvp]),
    ("sga_debug_radius_search_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_cloud_cluster_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_radius_waits", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_plane_default", None, [C.POINTER(PlaneParams)]),
    ("sga_cloud_segment_plane", C.c_int, [_vp, _vp, C.POINTER(PlaneParams), _dp, C.POINTER(C.c_uint32), C.POINTER(C.c_int64), _pvp, C.POINTER(PlaneResult)]),
    ("sga_debug_segment_plane_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_segment_plane_waits", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_plane_from_sums", C.c_int, [C.c_uint64, _dp, _dp, _dp, _dp, _dp]),
    ("sga_iss_default", None, [C.POINTER(IssParams)]),
    ("sga_cloud_iss_keypoints", C.c_int, [_vp, _vp, _vp, C.POINTER(IssParams), _dp, C.POINTER(C.c_int64), C.POINTER(C.c_size_t), _pvp]),
    ("sga_features_select", C.c_int, [_vp, _vp, C.POINTER(C.c_int64), C.c_size_t, _pvp]),
    ("sga_debug_iss_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_iss_waits", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_occupancy_params_default", None, [C.POINTER(OccupancyParams)]),
    ("sga_occupancy_create", C.c_int, [_vp, C.POINTER(OccupancyParams), _pvp]),
    ("sga_occupancy_destroy", C.c_int, [_vp]),
    ("sga_occupancy_get", C.c_int, [_vp, C.POINTER(OccupancyParams), C.POINTER(C.c_uint64)]),
    ("sga_occupancy_clear", C.c_int, [_vp, _vp]),
    ("sga_occupancy_integrate", C.c_int, [_vp, _vp, _vp, _dp, C.c_double, C.c_double, C.c_int, C.POINTER(OccupancyScanStats)]),
    ("sga_occupancy_classify", C.c_int, [_vp, _vp, _vp, _dp, C.c_double, C.c_int, C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(OccupancyCounts), _pvp]),
    ("sga_occupancy_stats", C.c_int, [_vp, _vp, C.c_double, C.POINTER(OccupancyCounts)]),
    ("sga_occupancy_export", C.c_int, [_vp, _vp, C.c_double, C.c_int, C.c_size_t, C.POINTER(C.c_int64), _fp, C.POINTER(C.c_size_t), _pvp]),
    ("sga_occupancy_download", C.c_int, [_vp, _vp, C.POINTER(C.c_uint32), _fp]),
    ("sga_debug_occupancy_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_occupancy_waits", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_cloud_fpfh_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_features_match_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_ransac_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_ransac_draw", C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64)]),
    ("sga_debug_rigid_from_sums", C.c_int, [C.c_uint64, _dp, _dp, _dp, _dp]),
    ("sga_debug_cloud_box", C.c_int, [_vp, C.POINTER(C.c_int), _fp, _fp]),
    ("sga_cloud_destroy", C.c_int, [_vp]),
    ("sga_cloud_size", C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    ("sga_cloud_has", C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("sga_cloud_download", C.c_int, [_vp, _vp, _fp, _fp, _fp]),
    ("sga_cloud_download_f64", C.c_int, [_vp, _vp, _dp, _fp, _fp]),
    ("sga_cloud_create_device", C.c_int, [C.c_void_p, _da, _da, _da, C.c_size_t, C.POINTER(C.c_double), C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    ("sga_cloud_export_device", C.c_int, [C.c_void_p, C.c_void_p, _da, _da, _da, C.c_void_p, C.c_int]),
    ("sga_index_knn_device", C.c_int, [C.c_void_p, C.c_void_p, _da, C.c_size_t, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("sga_problem_get_factors_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    ("sga_voxelgrid_sampling", C.c_int, [_vp, _vp, C.c_double, _pvp]),
    ("sga_voxelgrid_sampling_fields", C.c_int, [_vp, _vp, _vp, C.POINTER(C.c_int), C.c_double, _pvp, _pvp, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    ("sga_voxelgrid_sampling_fields_device", C.c_int, [_vp, _vp, C.POINTER(DeviceArray), C.POINTER(C.c_int), C.c_double, _pvp, _pvp, _vp, _vp, _vp, C.c_int]),
    ("sga_estimate_normals_covariances", C.c_int, [_vp, _vp, _vp, C.c_int, C.c_int]),
    ("sga_index_build_kdtree", C.c_int, [_vp, _vp, _pvp]),
    ("sga_index_build_kdtree_batch", C.c_int, [_vp, _pvp, C.c_size_t, _pvp]),
    ("sga_estimate_normals_covariances_batch", C.c_int, [_vp, _pvp, _pvp, C.c_size_t, C.c_int, C.c_int]),
    ("sga_debug_forest_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_voxelgrid_sampling_batch", C.c_int, [_vp, _pvp, C.c_size_t, C.c_double, _pvp]),
    ("sga_debug_voxelgrid_batch_plan", C.c_int, [_pvp, C.c_size_t, C.c_double, C.POINTER(C.c_int)]),
    ("sga_debug_voxelgrid_batch_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_index_build_gaussian_voxelmap_batch", C.c_int, [_vp, _pvp, C.c_size_t, C.c_double, _pvp]),
    ("sga_debug_voxelmap_batch_plan", C.c_int, [_pvp, C.c_size_t, C.c_double, C.POINTER(C.c_int)]),
    ("sga_debug_voxelmap_batch_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_index_bbox", C.c_int, [_vp, _fp, _fp]),
    ("sga_index_build_gaussian_voxelmap", C.c_int, [_vp, _vp, C.c_double, _pvp]),
    ("sga_index_create_voxelmap_from_voxels", C.c_int, [_vp, C.c_double, C.c_void_p, _dp, _dp, C.c_size_t, _pvp]),
    ("sga_index_create_flatmap_from_voxels", C.c_int, [_vp, C.c_double, C.c_void_p, C.c_void_p, _dp, _dp, C.c_int, C.c_size_t, _pvp]),
    ("sga_index_refresh_attributes", C.c_int, [_vp, _vp, _vp]),
    ("sga_index_clone", C.c_int, [_vp, _vp, _pvp]),
    ("sga_index_destroy", C.c_int, [_vp]),
    ("sga_index_size", C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    ("sga_index_voxelmap_download", C.c_int, [_vp, _vp, C.POINTER(C.c_int32), _fp, _fp, C.POINTER(C.c_uint32)]),
    ("sga_voxelmap_create", C.c_int, [_vp, C.c_double, _pvp]),
    ("sga_voxelmap_insert", C.c_int, [_vp, _vp, _vp, _dp]),
    ("sga_voxelmap_insert_batch", C.c_int, [_vp, _pvp, _pvp, _dp, C.c_size_t]),
    ("sga_debug_voxelmap_insert_batch_plan", C.c_int, [_pvp, _pvp, C.c_size_t, C.POINTER(C.c_int)]),
    ("sga_debug_voxelmap_insert_batch_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_voxelmap_set_lru", C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    ("sga_flatmap_create", C.c_int, [_vp, C.c_double, _pvp]),
    ("sga_flatmap_set_setting", C.c_int, [_vp, C.c_double, C.c_uint32]),
    ("sga_voxelmap_set_search_offsets", C.c_int, [_vp, C.c_int]),
    ("sga_flatmap_download", C.c_int, [_vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _fp, _fp]),
    ("sga_flatmap_create_contents", C.c_int, [_vp, C.c_double, C.c_int, _pvp]),
    ("sga_flatmap_get_contents", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("sga_flatmap_download_contents", C.c_int, [_vp, _vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), _fp, _fp, _fp]),
    ("sga_index_create_flatmap_from_voxels_contents", C.c_int, [_vp, C.c_double, C.c_void_p, C.c_void_p, _dp, _dp, _dp, C.c_int, C.c_size_t, _pvp]),
    ("sga_index_knn", C.c_int, [_vp, _vp, _fp, C.c_size_t, C.c_int, C.c_double, C.POINTER(C.c_int64), _fp]),
    ("sga_index_knn_f64", C.c_int, [_vp, _vp, _dp, C.c_size_t, C.c_int, C.c_double, C.POINTER(C.c_int64), _dp]),
    ("sga_index_build_projective", C.c_int, [_vp, _vp, C.c_int, C.c_int, _pvp]),
    ("sga_projective_set_search_window", C.c_int, [_vp, C.c_int, C.c_int]),
    ("sga_projective_set_border_modes", C.c_int, [_vp, C.c_int, C.c_int]),
    ("sga_projective_get_params", C.c_int, [_vp, C.POINTER(C.c_int)]),
    ("sga_projective_download_map", C.c_int, [_vp, _vp, C.POINTER(C.c_uint32)]),
    ("sga_factor_params_default", None, [C.POINTER(FactorParams)]),
    ("sga_problem_create", C.c_int, [_vp, _vp, _vp, _dp, _pvp]),
    ("sga_problem_create_from_index", C.c_int, [_vp, _vp, _vp, _dp, _pvp]),
    ("sga_problem_create_batch", C.c_int, [_vp, _pvp, _pvp, _dp, C.c_size_t, _pvp]),
    ("sga_debug_problem_batch_plan", C.c_int, [_pvp, _pvp, C.c_size_t, C.POINTER(C.c_int)]),
    ("sga_debug_problem_batch_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_problem_destroy", C.c_int, [_vp]),
    ("sga_linearize", C.c_int, [_vp, _vp, C.POINTER(FactorParams), _dp, _dp, _dp, _dp, C.POINTER(C.c_uint64)]),
    ("sga_error", C.c_int, [_vp, _vp, C.POINTER(FactorParams), _dp, _dp]),
    ("sga_linearize_async", C.c_int, [_vp, _vp, C.POINTER(FactorParams), _dp, _vp]),
    ("sga_error_async", C.c_int, [_vp, _vp, C.POINTER(FactorParams), _dp, _vp]),
    ("sga_comm_unique_id", C.c_int, [C.POINTER(C.c_ubyte)]),
    ("sga_comm_init", C.c_int, [_vp, C.c_int, C.c_int, C.POINTER(C.c_ubyte)]),
    ("sga_comm_destroy", C.c_int, [_vp]),
    ("sga_comm_init_callback", C.c_int, [_vp, C.c_int, C.c_int, ALLREDUCE_FN, _vp]),
    ("sga_error_model_eval", C.c_int, [_dp, _dp, _dp, _dp]),
    ("sga_unpack_accumulator", None, [_dp, _dp, _dp, _dp, C.POINTER(C.c_uint64)]),
    ("sga_problem_set_rejector", C.c_int, [_vp, REJECTOR_FN, _vp]),
    ("sga_linearize_per_point", C.c_int, [_vp, _vp, C.POINTER(FactorParams), _dp, _dp, C.POINTER(C.c_ubyte)]),
    ("sga_problem_get_factors", C.c_int, [_vp, _vp, C.POINTER(C.c_int64), _fp]),
    ("sga_context_set_stream_ordered", C.c_int, [_vp, C.c_int]),
    ("sga_context_set_profiling", C.c_int, [_vp, C.c_int]),
    ("sga_context_get_kernel_ms", C.c_int, [_vp, _dp, C.POINTER(C.c_uint64), _dp, C.POINTER(C.c_uint64)]),
    ("sga_context_get_comm_ms", C.c_int, [_vp, _dp, C.POINTER(C.c_uint64)]),
    ("sga_context_get_search_ms", C.c_int, [_vp, _dp, C.POINTER(C.c_uint64)]),
    ("sga_context_get_pass_ms", C.c_int, [_vp, _dp, C.POINTER(C.c_uint64), _dp, C.POINTER(C.c_uint64), _dp]),
    ("sga_set_warm_limit", None, [C.c_double]),
    ("sga_set_error_model", None, [C.c_int]),
    ("sga_problem_set_search_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    ("sga_problem_get_search_stats", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("sga_problem_get_sorted_points", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("sga_problem_get_grid_stats", C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("sga_problem_get_last_plan", C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    ("sga_set_grid_mode", None, [C.c_int, C.c_longlong]),
    ("sga_host_alloc", C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    ("sga_host_free", C.c_int, [C.c_void_p]),
    ("sga_index_spacing", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("sga_set_knn_wave_max", None, [C.c_longlong]),
    ("sga_debug_kd_tree", C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_void_p, C.c_void_p]),
    ("sga_debug_voxelgrid_plan", C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_int)]),
    ("sga_debug_set_voxelgrid_epoch", C.c_int, [C.c_void_p, C.c_uint]),
    ("sga_debug_timer_start", C.c_int, [C.c_void_p]),
    ("sga_debug_timer_stop", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("sga_debug_shard_frame_pack", None, [C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("sga_debug_shard_frame_agree", C.c_int, [C.POINTER(C.c_double)]),
    ("sga_debug_reduce_rows", C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    ("sga_debug_reduce_stamps", C.c_int, [C.c_void_p]),
    ("sga_debug_kd_trips", C.c_int, [C.c_void_p]),
    ("sga_debug_kd_wave_times", C.c_int, [C.c_void_p, C.c_int]),
    ("sga_set_search_mode", None, [C.c_int, C.c_int, C.c_int]),
    ("sga_get_warm_limit", C.c_double, []),
    ("sga_problem_get_pass_stats", C.c_int, [_vp, _vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    ("sga_registration_setting_default", None, [C.POINTER(RegistrationSettingC)]),
    ("sga_align", C.c_int, [_vp, _vp, _vp, _dp, C.POINTER(RegistrationSettingC), C.POINTER(ResultC)]),
    ("sga_align_problem", C.c_int, [_vp, _vp, _dp, C.POINTER(RegistrationSettingC), C.POINTER(ResultC)]),
    ("sga_sweep_params_default", None, [C.POINTER(SweepParams)]),
    # ctx, target, source, times, factor params, T, twist, ref_time, H144, b12, e, num_inliers, nearest
    ("sga_sweep_linearize", C.c_int, [_vp, _vp, _vp, _fp, C.POINTER(FactorParams), _dp, _dp, C.c_double, _dp, _dp, _dp, C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]),
    ("sga_sweep_error", C.c_int, [_vp, _vp, _vp, _fp, C.POINTER(FactorParams), _dp, _dp, C.c_double, _dp]),
    # ctx, target, source, times, init_T, init_twist, setting, sweep params, result
    ("sga_align_sweep", C.c_int, [_vp, _vp, _vp, _fp, _dp, _dp, C.POINTER(RegistrationSettingC), C.POINTER(SweepParams), C.POINTER(SweepResultC)]),
    ("sga_debug_sweep_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_debug_voxelgrid_fields_launches", C.c_int, [C.POINTER(C.c_ulonglong)]),
    ("sga_multi_create", C.c_int, [C.POINTER(C.c_int), C.c_int, _pvp]),
    ("sga_multi_destroy", C.c_int, [_vp]),
    ("sga_multi_num_devices", C.c_int, [_vp]),
    ("sga_multi_set_target_f64", C.c_int, [_vp, _dp, _dp, _dp, C.c_size_t]),
    ("sga_multi_set_target_f32", C.c_int, [_vp, _fp, _fp, _fp, C.c_size_t]),
    ("sga_multi_set_source_f32", C.c_int, [_vp, _fp, _fp, _fp, C.c_size_t, _dp]),
    ("sga_multi_set_target_f32_origin", C.c_int, [_vp, _fp, _fp, _fp, C.c_size_t, _dp]),
    ("sga_multi_set_source_f32_origin", C.c_int, [_vp, _fp, _fp, _fp, C.c_size_t, _dp, _dp]),
    ("sga_multi_set_target_voxels", C.c_int, [_vp, C.c_double, C.c_void_p, _dp, _dp, C.c_size_t]),
    ("sga_multi_set_search_offsets", C.c_int, [_vp, C.c_int]),
    ("sga_multi_set_rejector", C.c_int, [_vp, C.c_void_p, _vp]),
    ("sga_multi_set_target_flat_voxels", C.c_int, [_vp, C.c_double, C.c_void_p, C.c_void_p, _dp, _dp, C.c_int, C.c_size_t]),
    ("sga_multi_set_source_f64", C.c_int, [_vp, _dp, _dp, _dp, C.c_size_t, _dp]),
    ("sga_multi_linearize", C.c_int, [_vp, C.POINTER(FactorParams), _dp, _dp, _dp, _dp, C.POINTER(C.c_uint64)]),
    ("sga_multi_error", C.c_int, [_vp, C.POINTER(FactorParams), _dp, _dp]),
    ("sga_multi_align", C.c_int, [_vp, _dp, C.POINTER(RegistrationSettingC), C.POINTER(ResultC)]),
    ("sga_multi_reset_search_state", C.c_int, [_vp]),
    ("sga_multi_get_factors", C.c_int, [_vp, C.c_void_p, C.c_void_p]),
    ("sga_batch_create", C.c_int, [_vp, _pvp, C.c_size_t, _pvp]),
    ("sga_batch_destroy", C.c_int, [_vp]),
    ("sga_batch_size", C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    ("sga_batch_linearize", C.c_int, [_vp, _vp, C.POINTER(FactorParams), _dp, C.POINTER(C.c_ubyte), _dp, _dp, _dp, C.POINTER(C.c_uint64)]),
    ("sga_align_batch", C.c_int, [_vp, _vp, _dp, C.POINTER(RegistrationSettingC), C.POINTER(ResultC)]),
    ("sga_optimize_batch", C.c_int, [C.POINTER(RegistrationSettingC), C.c_size_t, _dp, BATCH_LINEARIZE_FN, BATCH_ERROR_FN, _vp, C.POINTER(ResultC)]),
    ("sga_optimize", C.c_int, [C.POINTER(RegistrationSettingC), _dp, LINEARIZE_FN, ERROR_FN, _vp, C.POINTER(ResultC)]),
    ("sga_se3_exp", None, [_dp, _dp]),
    ("sga_se3_log", None, [_dp, _dp]),
]

_LIB = None


def load():
    """Load the shared library (raises if it has not been built: `python -c 'import __graft_entry__ as g; g.build()'` or `make lib`)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise SgaError(f"{LIB_PATH} is missing: build it with `make lib` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    # torch bundles its own libamdhip64.so with the same SONAME; if torch is (or will be) in this process it must be
    # loaded first so that exactly one HIP runtime is mapped.
    if "torch" in sys.modules or os.environ.get("SGA_WITH_TORCH", "0") == "1":
        import torch  # noqa: F401
    # contexts are streams, and streams that share a hardware queue serialise (csrc/context.hip: 4 queues per device unless asked otherwise;
    # read once, when the HIP runtime initialises — so before anything of it runs)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _LIB = lib
    return lib


def check(rc):
    if rc != SGA_OK:
        raise SgaError(f"small_gicp_amd error {rc}: {load().sga_last_error().decode()}")

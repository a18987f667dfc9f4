"""small_gicp_amd — MI355X-native drop-in for the per-iteration registration hot path of koide3/small_gicp.

The compute lives in lib/libsmall_gicp_amd.so (hand-written HIP for gfx950 behind the C-ABI of include/small_gicp_amd.h).
This package is the thin host layer: ctypes binding (_lib), a Python mirror of the reference's module (api) and the frozen
synthetic workloads of the benchmark configs (synthetic).
"""
from . import api, synthetic  # noqa: F401
from ._lib import GICP, ICP, LIB_PATH, PLANE_ICP, SgaError, load  # noqa: F401
from .api import (  # noqa: F401
    BatchProblem,
    Context,
    GaussianVoxelMap,
    IncrementalVoxelMap,
    IncrementalVoxelMapCov,
    IncrementalVoxelMapNormal,
    IncrementalVoxelMapNormalCov,
    KdTree,
    MultiProblem,
    PointCloud,
    Problem,
    ProjectiveSearch,
    RegistrationResult,
    align,
    align_batch,
    build_gaussian_voxelmaps,
    build_kdtrees,
    cloud_merge_launches,
    create_problems,
    default_context,
    estimate_covariances,
    estimate_covariances_batch,
    estimate_normals,
    estimate_normals_batch,
    estimate_normals_covariances,
    estimate_normals_covariances_batch,
    forest_launches,
    error_model_eval,
    get_warm_limit,
    insert_batch,
    set_error_model,
    set_grid_mode,
    set_search_mode,
    set_warm_limit,
    make_setting,
    merge_clouds,
    optimize,
    optimize_batch,
    pinned_copy,
    pinned_empty,
    preprocess_batch,
    preprocess_points,
    preprocess_points_batch,
    problem_batch_launches,
    unpack_accumulator,
    voxelgrid_sampling,
    voxelgrid_sampling_batch,
    voxelgrid_batch_launches,
    voxelmap_batch_launches,
    voxelmap_insert_batch_launches,
)

__version__ = "0.1.0"

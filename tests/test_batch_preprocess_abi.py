"""The batched preprocessing entry points (include/small_gicp_amd.h: sga_index_build_kdtree_batch,
sga_estimate_normals_covariances_batch) where no device is needed: the checks that come before any device work, and the argument
handling of the Python wrappers (small_gicp_amd/api.py)."""
import ctypes as C

import pytest

import small_gicp_amd as sga
from small_gicp_amd import api

INVALID = 1


def test_symbols_are_declared_and_exported():
    lib = sga.load()
    names = [s[0] for s in sga._lib.SYMBOLS]
    for name in ("sga_index_build_kdtree_batch", "sga_estimate_normals_covariances_batch", "sga_debug_forest_launches"):
        assert name in names and getattr(lib, name) is not None


def test_null_arguments_and_empty_batches():
    lib = sga.load()
    out = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    hs = (C.c_void_p * 2)()
    assert lib.sga_index_build_kdtree_batch(None, hs, 2, out) == INVALID and b"null" in lib.sga_last_error()
    assert not out[0] and not out[1]  # on any failure every out[k] is NULL
    out = (C.c_void_p * 2)(0xDEAD, 0xDEAD)
    assert lib.sga_index_build_kdtree_batch(None, None, 2, out) == INVALID and not out[0] and not out[1]
    assert lib.sga_index_build_kdtree_batch(None, None, 0, None) == 0  # count == 0 is SGA_OK and does nothing
    assert lib.sga_estimate_normals_covariances_batch(None, hs, hs, 2, 20, 3) == INVALID and b"null" in lib.sga_last_error()
    assert lib.sga_estimate_normals_covariances_batch(None, None, None, 0, 20, 3) == 0
    assert lib.sga_debug_forest_launches(None) == INVALID
    v = C.c_ulonglong(0)
    assert lib.sga_debug_forest_launches(C.byref(v)) == 0  # (a count: whatever this process enqueued so far)


@pytest.mark.parametrize("k", [0, -3, 113, 1000])
def test_num_neighbors_outside_the_lone_range(k):
    lib = sga.load()
    hs = (C.c_void_p * 1)()
    assert lib.sga_estimate_normals_covariances_batch(None, hs, hs, 1, k, 3) == INVALID
    assert b"num_neighbors must be in [1,112]" in lib.sga_last_error()


def test_python_wrappers_check_their_arguments():
    with pytest.raises(TypeError):
        api.build_kdtrees([object()])
    with pytest.raises(ValueError, match="as many trees as clouds"):
        api._estimate_batch([], [object()], 20, 3)
    with pytest.raises(TypeError):
        api.preprocess_batch([[0.0, 0.0, 0.0]])
    # keyword of the batched odometry driver exists and defaults to the unbatched preprocessing
    import inspect

    from small_gicp_amd import odometry

    assert inspect.signature(odometry.run_synthetic_batched).parameters["batched_preprocessing"].default is False
    for name in ("build_kdtrees", "estimate_covariances_batch", "estimate_normals_batch", "estimate_normals_covariances_batch", "preprocess_batch"):
        assert callable(getattr(sga, name))

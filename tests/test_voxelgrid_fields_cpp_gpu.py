"""include/small_gicp_amd.hpp: enum class Reduce, GridFields and voxelgrid_sampling(cloud, fields, ops, leaf, ...) against a host loop
(tests/cpp/test_cpp_voxelgrid_fields.cpp, compiled with g++ as tests/test_cloud_crop_gpu.py compiles its program), and the odometry
driver's sweep_source="voxelgrid" (DESIGN.md section 3.31)."""
import os
import subprocess

import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import odometry

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_program(tmp_path):
    exe = tmp_path / "test_cpp_voxelgrid_fields"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_voxelgrid_fields.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    return exe


def test_cpp_program_compiles(tmp_path):
    """(no device) the header's new declarations compile and link"""
    assert os.path.exists(compile_program(tmp_path))


@gpu
def test_cpp_voxelgrid_fields(tmp_path):
    exe = compile_program(tmp_path)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    grid = [r for r in rows if r[0] == "GRID"]
    assert len(grid) == 1 and int(grid[0][2]) >= 8 and grid[0][4] == "1" and grid[0][6] == "1" and grid[0][8] == "1", grid
    cols = [r for r in rows if r[0] == "COLUMN"]
    assert [r[2] for r in cols] == ["mean", "min", "max", "first", "nearest"] and all(r[4] == "1" for r in cols), cols
    for label in ("MEMBERSHIP", "DEFAULT", "REFUSE"):
        row = [r for r in rows if r[0] == label]
        assert len(row) == 1 and row[0][2] == "1", (label, row)


@gpu
def test_driver_sweep_source_voxelgrid():
    """The slalom with a reduced sensor: registering the voxel grid of the raw sweep, its times reduced by NEAREST, gives a finite
    trajectory whose largest position error is below that of the same frames deskewed with the previous motion (estimate_twist=False) —
    the relation DESIGN.md section 3.30 reports for the sample route.  Nothing tighter is asserted."""
    kw = dict(sweeps=True, trajectory="slalom", n_rings=16, n_az=400)
    base = odometry.run_synthetic(5, estimate_twist=False, **kw)
    res = {src: odometry.run_synthetic(5, estimate_twist=True, sweep_source=src, **kw) for src in ("sample", "voxelgrid")}
    for src, r in res.items():
        print("sweep_source=%-9s ate_trans_m_max %.4f (estimate_twist=False: %.4f), %.2f ms per scan" % (src, r["ate_trans_m_max"], base["ate_trans_m_max"], r["total_ms_per_scan"]))
        assert len(r["estimated"]) == 5 and all(np.isfinite(T).all() for T in r["estimated"]) and len(r["twists"]) == 4
    assert res["voxelgrid"]["ate_trans_m_max"] < base["ate_trans_m_max"]
    with pytest.raises(ValueError, match="sweep_source"):
        odometry.OnlineOdometry(sweep_source="grid")

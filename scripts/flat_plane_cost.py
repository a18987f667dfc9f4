"""GPU time of the scan-to-model factor kernels over a flat voxel map that keeps normals: a 1M-point source linearized against an
IncrementalVoxelMapNormal (1 m voxels, 7 offsets) built from a 1M-point target, REPS passes of ICP and REPS of PLANE_ICP at one pose
(linearize_kernel<..., ICP, 2> beside linearize_kernel<..., PLANE_ICP, 2>).  Run under `rocprofv3 --kernel-trace --stats -- python ...`
for the per-kernel means (profiles/flat_plane_kernel_stats.txt)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import synthetic  # noqa: E402

REPS = int(os.environ.get("REPS", "50"))
N = int(os.environ.get("POINTS", "1000000"))

tgt_raw, src_raw, T_gt = synthetic.registration_pair(N)
tgt = sga.PointCloud(tgt_raw)
sga.estimate_normals(tgt, None, 20)
src = sga.PointCloud(src_raw)
vm = sga.IncrementalVoxelMapNormal(1.0)
vm.set_search_offsets(7)
vm.insert(tgt)
pb = sga.Problem(vm, src, T_gt)
for mode in ("fp32", "fp64"):
    for factor in ("ICP", "PLANE_ICP"):
        st = sga.make_setting(factor, math_mode=mode)
        for _ in range(REPS):
            H, b, e, n = pb.linearize(st.factor, T_gt)
        print("%s %s: voxels %d, source %d, inliers %d, e %.6g" % (mode, factor, len(vm), len(src_raw), n, e))

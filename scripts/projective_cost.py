"""GPU time of a registration pass against a ProjectiveSearch target beside the same pass against a KdTree of the same cloud: a C5-sized
scan pair (synthetic.kitti_like_scan frames 0 and 1 turned into the camera convention, y down / z forward, 2048 x 512 image) and a
1M-point synthetic.scene target with a 1M-point source (1024 x 256 image), REPS GICP passes of each in fp32 and in fp64.  The passes
alternate between two poses 0.5 m apart so that every kd-tree pass is a cold one (a full search; the projective pass has no other kind).
Run under `rocprofv3 --kernel-trace --stats -- python ...` for the per-kernel means (profiles/projective_kernel_stats.txt)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import small_gicp_amd as sga  # noqa: E402
from small_gicp_amd import synthetic  # noqa: E402

REPS = int(os.environ.get("REPS", "50"))
CAM = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])


def cam_scan(frame):
    pts, Tws = synthetic.kitti_like_scan(frame)
    return (pts.astype(np.float64) @ CAM.T).astype(np.float32), Tws


def run(label, tgt_raw, src_raw, T, W, H):
    tgt, src = sga.PointCloud(tgt_raw), sga.PointCloud(src_raw)
    sga.estimate_covariances(tgt)
    sga.estimate_covariances(src)
    T2 = T.copy()
    T2[:3, 3] += [0.5, 0.0, 0.0]
    for name, index in (("projective", sga.ProjectiveSearch(tgt, W, H)), ("kdtree", sga.KdTree(tgt))):
        if name == "kdtree":
            index.refresh_attributes()
        pb = sga.Problem(index, src, T)
        for mode in ("fp32", "fp64"):
            st = sga.make_setting("GICP", 1.0, math_mode=mode)
            for r in range(REPS):
                H6, b, e, n = pb.linearize(st.factor, T if r % 2 == 0 else T2)
            print("%s %s %s: target %d, source %d, inliers at the last pose %d" % (label, name, mode, len(tgt_raw), len(src_raw), n))


(p0, T0), (p1, T1) = cam_scan(0), cam_scan(1)
C4 = np.eye(4)
C4[:3, :3] = CAM
run("C5", p0, p1, C4 @ np.linalg.inv(T0) @ T1 @ np.linalg.inv(C4), 2048, 512)
t1m, s1m, Tgt = synthetic.registration_pair(1_000_000)
run("1M", t1m, s1m, Tgt, 1024, 256)

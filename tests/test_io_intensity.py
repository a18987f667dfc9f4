"""io.read_points hands back the fourth column of a KITTI .bin on request; the default is what it was.  No device."""
import numpy as np

from small_gicp_amd import io


def test_read_points_returns_the_intensity_on_request(tmp_path):
    rng = np.random.default_rng(5)
    scan = rng.random((37, 4)).astype(np.float32)
    name = str(tmp_path / "scan.bin")
    scan.astype("<f4").tofile(name)
    plain = io.read_points(name)
    assert isinstance(plain, np.ndarray) and plain.shape == (37, 4) and np.array_equal(plain[:, :3], scan[:, :3]) and (plain[:, 3] == 1.0).all()
    pts, intensity = io.read_points(name, return_intensity=True)
    assert np.array_equal(pts, plain) and intensity.dtype == np.float32 and np.array_equal(intensity, scan[:, 3])
    pts, intensity = io.read_points(str(tmp_path / "missing.bin"), return_intensity=True)
    assert pts.shape == (0, 4) and intensity.shape == (0,)
    assert io.read_points(str(tmp_path / "missing.bin")).shape == (0, 4)

"""A range of a cloud as a cloud of its own (csrc/cloud_crop.hip: sga_cloud_slice), against sga_cloud_select over the same indices: the two
entry points share one gather kernel and one host body, and differ in what this file pins — an empty slice keeps its cloud's attribute
flags where an empty selection has none, and the range check has a message of its own.

The inputs' records are known exactly (tests/test_cloud_merge_gpu.py: Member uploads RELATIVE to a named origin), so the comparison is on
bits: downloads, origin, index words, box."""
import numpy as np
import pytest

import small_gicp_amd as sga
from small_gicp_amd import api
from test_cloud_merge_gpu import Member, attributes, upload_relative

pytestmark = pytest.mark.gpu

F32 = np.float32
FAR = np.array([500e3, 4000e3, 0.0])
RANGES = [(0, 0), (3, 0), (3, 1), (3, 255), (3, 256), (3, 257), (0, 600), (599, 1)]  # empty, one, around a workgroup of 256, whole, last


@pytest.fixture(scope="module")
def full():
    """600 points with normals and covariances, far from the origin (read only)"""
    return Member(600, 901, origin=FAR)


@pytest.fixture(scope="module")
def bare():
    """600 points with neither attribute (read only)"""
    return Member(600, 902, normals=False, covs=False)


def downloads(cloud):
    """what sga_cloud_download gives for the points, and for the attributes the cloud has"""
    nr, c6 = attributes(cloud)
    return cloud.xyz().tobytes(), None if nr is None else nr.tobytes(), None if c6 is None else c6.tobytes()


def check_slice(m, first, count):
    out = m.cloud.slice(first, count)
    twin = m.cloud.selected(np.arange(first, first + count))
    has = (m.nrm is not None, m.cov6 is not None)
    assert out.size() == count == twin.size()
    assert np.array_equal(out.origin(), m.origin) and np.array_equal(twin.origin(), m.origin)  # the origin is the input's
    assert out._box() is None  # a slice carries no box
    assert out._has() == has  # ... and its cloud's attributes, an empty one too
    if count == 0:
        assert twin._has() == (False, False)  # an empty selection: an empty cloud without attributes
        assert out.xyz().shape == (0, 3)
        return
    assert twin._has() == has
    assert downloads(out) == downloads(twin)  # points, normals, covariances: bit for bit
    nr, c6 = attributes(out)
    if m.nrm is not None:
        assert nr.tobytes() == np.ascontiguousarray(m.nrm[first : first + count]).tobytes()
    if m.cov6 is not None:
        assert c6.tobytes() == np.ascontiguousarray(m.cov6[first : first + count]).tobytes()
    # the index words run 0 .. count - 1 in storage order: the kd-tree's view returns the points with their index words
    _, _, _, pts, order = sga.KdTree(out)._tree()
    assert np.array_equal(np.sort(order), np.arange(count))
    back = np.empty((count, 3), F32)
    back[order] = pts
    assert back.tobytes() == np.ascontiguousarray(m.rel[first : first + count]).tobytes()  # index word j sits on record first + j


@pytest.mark.parametrize("first,count", RANGES)
def test_slice_equals_the_selection_of_its_range(full, bare, first, count):
    check_slice(full, first, count)
    check_slice(bare, first, count)


def test_an_empty_slice_keeps_the_flags_and_an_empty_selection_has_none(full, bare):
    assert full.cloud.slice(3, 0)._has() == full.cloud._has() == (True, True)
    assert bare.cloud.slice(3, 0)._has() == bare.cloud._has() == (False, False)
    assert full.cloud.selected([])._has() == (False, False)


@pytest.mark.parametrize("first,count", [(0, 601), (600, 1), (601, 0)])
def test_a_range_outside_the_cloud_is_refused(full, first, count):
    with pytest.raises(sga.SgaError, match=r"slice \[%d, %d\) outside a cloud of 600 points" % (first, first + count)):
        full.cloud.slice(first, count)


def test_slice_made_on_a_stream_ordered_context_is_read_through_another():
    """Uploaded and sliced on a stream-ordered context, downloaded through a second context on the same device: the slice is marked ready
    behind its kernel and the download waits for it.  This pins that the path works and gives the right rows; a passing run cannot prove
    the absence of a race."""
    rng = np.random.default_rng(903)
    xyz = rng.uniform(-30.0, 30.0, (2049, 3)).astype(F32)
    made = sga.Context(0)
    made.set_stream_ordered(True)
    cloud = upload_relative(xyz, None, None, np.zeros(3), made)
    part = cloud.slice(1, 2048)
    other = sga.Context(0)
    got = np.zeros((2048, 3), F32)
    api.check(sga.load().sga_cloud_download(other.h, part.h, api._fp(got), None, None))
    assert not cloud.origin().any()  # origin zero: the download is the records as they are
    assert got.tobytes() == np.ascontiguousarray(xyz[1:]).tobytes()
    made.set_stream_ordered(False)

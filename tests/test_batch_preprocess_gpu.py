"""Batched preprocessing on the device (csrc/batch_preprocess.hip; index_build.hip: kd_forest_*_kernel; preprocess.hip:
knn_wave_forest_kernel / features_from_list_forest_kernel): the kd-trees and the covariances of B clouds in one chain of launches.

  1. every tree of a forest is the lone build's tree, bit for bit (download, box, origin, and — for what the download does not show —
     equal linearizations and kNN rows);
  2. every tree meets its definition (kd_ref.check_tree), which does not lean on the lone build;
  3. normals / covariances equal the lone routine's bit for bit, and three members are checked against the float64 restatement of
     tests/search_ref.py with tests/test_search_matrix.py's bounds;
  4. mixed regimes (a large cloud, an empty one, members above the one-wave-per-query limit) inside one call;
  5. a member does not depend on its company;
  6. align_batch and the batched odometry driver give the same bits over batched and lone preprocessing;
  7. failure paths on a live device; 8. the launch count of a forest does not grow with its size.
"""
import ctypes as C

import numpy as np
import pytest

import search_ref as sr
import small_gicp_amd as sga
import test_batch_gpu as tb
import test_search_matrix as sm
from kd_ref import check_tree
from test_gpu_parity import _checked_tree, _same_tree

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = 1, 4
# every leaf / finish / instantiation boundary (8, 64, 256, 512, 1024, 2048, 4096, 8192, 16384), C5-shaped sizes, the largest forest member
SIZES = [1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1025, 2049, 4097, 8193, 11_119, 12_444, 16_385, 32_768]
_FRAMES = {}


def scan(frame):
    if frame not in _FRAMES:
        _FRAMES[frame] = np.ascontiguousarray(sga.synthetic.kitti_like_scan(frame)[0][:, :3], dtype=np.float32)
    return _FRAMES[frame]


def cut(n, k):
    """n points of a KITTI-shaped scan, spread over the scan (not its first rings only)"""
    pts = scan(k % 3)
    return np.ascontiguousarray(pts[np.random.default_rng(100 + k).choice(len(pts), n, replace=False)])


def members():
    """(points, is double) per size: one member geo-referenced, one with all points equal, one with a fiftieth duplicated"""
    out = []
    for k, n in enumerate(SIZES):
        p = cut(n, k)
        if n == 2049:
            p = np.tile(p[:1], (n, 1))
        if n == 8193:
            p[: n // 50] = p[n // 50 : 2 * (n // 50)]
        out.append(p.astype(np.float64) + tb.SHIFT if n == 4097 else p)
    return out


def same_index(forest, lone, label, probe=True):
    assert _same_tree(forest._tree(), lone._tree()), label
    lib = sga.load()
    of, ol = np.zeros(3), np.zeros(3)
    sga._lib.check(lib.sga_index_origin(forest.h, of.ctypes.data_as(C.POINTER(C.c_double))))
    sga._lib.check(lib.sga_index_origin(lone.h, ol.ctypes.data_as(C.POINTER(C.c_double))))
    assert np.array_equal(of, ol), label
    assert forest.size() == lone.size(), label
    # the box: in the forest it comes through the call's pinned block (for <= 256 points from kd_forest_root_kernel), not through a note
    (flo, fhi), (llo, lhi) = forest._bbox(), lone._bbox()
    assert flo.tobytes() == llo.tobytes() and fhi.tobytes() == lhi.tobytes(), (label, flo, fhi, llo, lhi)
    if lone.size() > 0:  # and it is the box of the stored records
        rec = lone._tree()[3]
        assert np.array_equal(flo, rec.min(0)) and np.array_equal(fhi, rec.max(0)), label
    if not probe or lone.size() == 0:
        return
    # boxes, group headers, leaf blocks, pair records: pinned by behaviour (test_kd_build_is_valid_and_repeatable)
    src = lone.cloud.xyz64()[:: max(1, lone.size() // 300)] + 0.05
    q = np.concatenate([src, lone.cloud.xyz64()[:5] + 30.0])
    k = min(10, lone.size())
    a, b = forest.batch_knn_search(q, k), lone.batch_knn_search(q, k)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), label
    st = sga.make_setting("ICP")
    sc = sga.PointCloud(src)
    la, lb = sga.Problem(forest, sc).linearize(st.factor, np.eye(4)), sga.Problem(lone, sc).linearize(st.factor, np.eye(4))
    assert all(np.array_equal(x, y) for x, y in zip(la, lb)), label
    assert forest.spacing() == lone.spacing(), label


def test_forest_trees_equal_lone_builds_and_their_definition():
    """Checks 1 and 2: the sizes in one call, the same reversed, and a call of one."""
    pts = members()
    clouds = [sga.PointCloud(p) for p in pts]
    lone = [sga.KdTree(c) for c in clouds]
    for order in (list(range(len(pts))), list(reversed(range(len(pts)))), [14]):
        forest = sga.build_kdtrees([clouds[i] for i in order])
        assert len(forest) == len(order)
        for tree, i in zip(forest, order):
            label = "n=%d order=%s" % (SIZES[i], "one" if len(order) == 1 else order[0])
            same_index(tree, lone[i], label)
            # the definition, independent of the lone build: node by node, and the stored records
            depth, thr, axis, pk, o = tree._tree()
            check_tree(pk, o, depth, thr, axis, SIZES[i])
            org = clouds[i].origin()
            p64 = np.asarray(pts[i], dtype=np.float64)
            stored = (p64 - org).astype(np.float32) if org.any() else np.asarray(pts[i], dtype=np.float32)
            assert np.array_equal(pk.view(np.uint32), stored[o].view(np.uint32)), label
        del forest
    # _checked_tree itself on a forest member's cloud: the lone tree it builds is the forest's
    tree, t = _checked_tree(pts[10], clouds[10])
    assert _same_tree(t, sga.build_kdtrees([clouds[10], clouds[3]])[0]._tree())


def _attributes(cloud, flags):
    """the cloud's own arrays"""
    out = []
    if flags & 1:
        out.append(cloud.normals().tobytes())
    if flags & 2:
        out.append(cloud.covs().tobytes())
    return out


def _same_index_attributes(ta, tb_, pts, flags, label):
    """the indexes' kd-ordered copies, seen through Problems built from the indexes: GICP reads the covariances of target and source
    index, PLANE_ICP the target index's normals"""
    T = np.eye(4)
    T[:3, 3] = [0.02, -0.01, 0.015]
    if flags & 1:
        f = sga.make_setting("PLANE_ICP").factor
        la, lb = sga.Problem(ta, sga.PointCloud(pts)).linearize(f, T), sga.Problem(tb_, sga.PointCloud(pts)).linearize(f, T)
        assert all(np.array_equal(x, y) for x, y in zip(la, lb)), (label, "normals")
    if flags & 2:
        f = sga.make_setting("GICP").factor
        la, lb = sga.Problem(ta, ta).linearize(f, T), sga.Problem(tb_, tb_).linearize(f, T)
        assert all(np.array_equal(x, y) for x, y in zip(la, lb)), (label, "covariances")


@pytest.mark.parametrize("k", [5, 10, 20, 64])
@pytest.mark.parametrize("flags", [1, 2, 3])
def test_forest_features_equal_the_lone_routine(k, flags):
    """Check 3, first half: per member the bits of sga_estimate_normals_covariances(cloud, tree, k, flags) — the cloud's arrays, and
    the index's kd-ordered copies through a linearization of a Problem built from the index (GICP reads the covariances, PLANE_ICP the normals)."""
    sizes = [1, 4, 5, 64, 65, 513, 4097, 11_119, 32_768]
    pts = [cut(n, 40 + j) for j, n in enumerate(sizes)]
    pts[3] = pts[3].astype(np.float64) + tb.SHIFT
    a = [sga.PointCloud(p) for p in pts]
    b = [sga.PointCloud(p) for p in pts]
    ta = sga.build_kdtrees(a)
    tb_ = [sga.KdTree(c) for c in b]
    sga.api._estimate_batch(a, ta, k, flags)
    for c, t in zip(b, tb_):
        sga.api._estimate(c, t, k, flags)
    for j, n in enumerate(sizes):
        assert _attributes(a[j], flags) == _attributes(b[j], flags), (n, k, flags)
        assert a[j]._has() == b[j]._has()
        _same_index_attributes(ta[j], tb_[j], pts[j], flags, (n, k, flags))


@pytest.mark.parametrize("k", [5, 20, 64])
def test_forest_features_against_float64_restatement(k):
    """Check 3, second half, independent of the lone kernels: three members of a forest against tests/search_ref.py — the neighbour
    sets (kNN rows of the forest's tree: test_search_matrix.check_rows) and the normals / covariances (check_features, its bounds)."""
    pts = [sm.random_scene(n, 7 * n + k, scale=12.0) for n in (65, 4097, 9000)] + [cut(11_119, 3)]
    clouds = [sga.PointCloud(p) for p in pts]
    trees = sga.build_kdtrees(clouds)
    sga.estimate_normals_covariances_batch(clouds, trees, k)
    for p32, c, t in zip(pts[:3], clouds[:3], trees[:3]):
        label = "forest n=%d k=%d" % (len(p32), k)
        sm.check_features(label, c, sr.features_ref(p32, k))
        q = sm.make_queries(p32, k + len(p32), m=96)
        ri, rd, band, e = sr.knn_ref(p32, q, k, -1.0, origin=np.zeros(3))
        idx, d2 = t.batch_knn_search(q, k)
        sm.check_rows(label, idx, d2, ri, rd, band, e, len(p32), k, True, True)


def test_mixed_regimes_in_one_call():
    """Check 4: a 200 000-point cloud, an empty cloud and three small ones; covariances with a member above the one-wave-per-query limit."""
    big, _, _ = sga.synthetic.registration_pair(200_000)
    pts = [cut(5000, 1), big, np.zeros((0, 3), np.float32), cut(300, 2), cut(12_000, 3)]
    a = [sga.PointCloud(p) for p in pts]
    b = [sga.PointCloud(p) for p in pts]
    ta = sga.build_kdtrees(a)
    tl = [sga.KdTree(c) for c in b]
    for j in range(len(pts)):
        same_index(ta[j], tl[j], "mixed %d" % j, probe=len(pts[j]) > 0)
    lib = sga.load()
    lib.sga_set_knn_wave_max(6000)  # members 1 and 4 take the lone routine inside the call
    try:
        sga.estimate_normals_covariances_batch(a, ta, 20)
        for c, t in zip(b, tl):
            sga.estimate_normals_covariances(c, t, 20)
    finally:
        lib.sga_set_knn_wave_max(sm.WAVE_DEFAULT)
    for j in range(len(pts)):
        assert _attributes(a[j], 3) == _attributes(b[j], 3), j
        assert a[j]._has() == b[j]._has() == (True, True), j
        if len(pts[j]) > 0:  # the kd-ordered copies of forest members and of the members that fell back
            _same_index_attributes(ta[j], tl[j], pts[j], 3, "mixed %d" % j)
    # k > 64: every member through the lone routine, the same bits
    sga.estimate_covariances_batch(a[:1] + a[3:], ta[:1] + ta[3:], 100)
    for c, t in zip(b[:1] + b[3:], tl[:1] + tl[3:]):
        sga.estimate_covariances(c, t, 100)
    for j in (0, 3, 4):
        assert a[j].covs().tobytes() == b[j].covs().tobytes(), j
        _same_index_attributes(ta[j], tl[j], pts[j], 2, "k=100 member %d" % j)


def test_a_member_does_not_depend_on_its_company():
    """Check 5: tree and covariances of one cloud alone, first and last of 16, bit for bit."""
    mine = cut(11_119, 5)
    others = [cut(n, 60 + j) for j, n in enumerate([12_444, 700, 11_800, 32_768, 9, 10_950, 4096, 11_500, 257, 12_000, 11_119, 2048, 13_000, 64, 11_700])]

    def run(pos):
        ps = list(others) if pos is not None else []
        at = 0 if pos is None else pos
        ps.insert(at, mine)
        clouds = [sga.PointCloud(p) for p in ps]
        pairs = sga.preprocess_batch(clouds, 20)
        c, t = pairs[at]
        return t._tree(), c.covs().tobytes(), t.spacing()

    alone, first, last = run(None), run(0), run(15)
    for other in (first, last):
        assert _same_tree(alone[0], other[0]) and alone[1] == other[1] and alone[2] == other[2]


def test_down_the_chain_align_batch_and_odometry():
    """Check 6."""
    from small_gicp_amd import odometry

    downs = [sga.voxelgrid_sampling(sga.PointCloud(scan(f)), 0.25) for f in range(3)]
    twins = [sga.voxelgrid_sampling(sga.PointCloud(scan(f)), 0.25) for f in range(3)]
    batched = sga.preprocess_batch(downs, 20)
    lone = []
    for c in twins:
        t = sga.KdTree(c)
        sga.estimate_covariances(c, t, 20)
        lone.append((c, t))
    ra = sga.align_batch([batched[0][1], batched[1][1]], [batched[1][1], batched[2][1]])
    rb = sga.align_batch([lone[0][1], lone[1][1]], [lone[1][1], lone[2][1]])
    assert len(ra) == 2 and all(tb._same(x, y) for x, y in zip(ra, rb)) and all(r.converged for r in ra)
    a = odometry.run_synthetic_batched(7, batch=4, batched_preprocessing=True)
    b = odometry.run_synthetic_batched(7, batch=4, batched_preprocessing=False)
    assert a["iterations"] == b["iterations"] and len(a["relative_poses"]) == 6
    assert all(np.array_equal(x, y) for x, y in zip(a["relative_poses"], b["relative_poses"]))


def _raw_build(ctx, clouds):
    hs = (C.c_void_p * len(clouds))(*[c.h.value if c is not None else None for c in clouds])
    out = (C.c_void_p * len(clouds))(*[0xDEAD] * len(clouds))
    return sga.load().sga_index_build_kdtree_batch(ctx.h, hs, len(clouds), out), out


def test_failure_paths_on_a_live_device():
    """Check 7: a NaN member, stream-ordered mode, every validation error once.  Nothing here provokes a fault."""
    lib = sga.load()
    ctx = sga.default_context()
    good = [sga.PointCloud(cut(n, 70 + j)) for j, n in enumerate([3000, 11_119, 200])]
    bad = cut(5000, 9)
    bad[1234, 1] = np.nan
    rc, out = _raw_build(ctx, [good[0], sga.PointCloud(bad), good[1]])
    assert rc == INVALID and not any(out[k] for k in range(3)) and b"cloud 1 " in lib.sga_last_error()
    trees = sga.build_kdtrees(good)  # a following good call works
    lone = [sga.KdTree(c) for c in good]
    for t, l in zip(trees, lone):
        same_index(t, l, "after a failed call")
    # stream-ordered mode: the same bits
    sctx = sga.Context(0)
    sctx.set_stream_ordered(True)
    sc = [sga.PointCloud(cut(n, 70 + j), ctx=sctx) for j, n in enumerate([3000, 11_119, 200])]
    pairs = sga.preprocess_batch(sc, 20)
    sga.estimate_covariances_batch(good, trees, 20)
    for (c, t), g, gt in zip(pairs, good, trees):
        assert _same_tree(t._tree(), gt._tree()) and c.covs().tobytes() == g.covs().tobytes()
    sctx.synchronize()
    # a member made by ANOTHER context of the same device is accepted (waited for, as in the lone calls) and gives the same bits
    foreign = sga.PointCloud(cut(3000, 70), ctx=sctx)
    out1 = (C.c_void_p * 1)()
    assert lib.sga_index_build_kdtree_batch(ctx.h, (C.c_void_p * 1)(foreign.h.value), 1, out1) == 0
    ftree = sga.KdTree(foreign, _handle=C.c_void_p(out1[0]))
    assert lib.sga_estimate_normals_covariances_batch(ctx.h, (C.c_void_p * 1)(foreign.h.value), (C.c_void_p * 1)(ftree.h.value), 1, 20, 2) == 0
    sctx.synchronize()
    same_index(ftree, lone[0], "a cloud of another context", probe=False)
    assert foreign.covs().tobytes() == good[0].covs().tobytes()
    # validation, each once
    rc, out = _raw_build(ctx, [good[0], None])
    assert rc == INVALID and not out[0] and not out[1]
    assert lib.sga_index_build_kdtree_batch(ctx.h, None, 2, out) == INVALID
    cs = (C.c_void_p * 2)(good[0].h.value, good[1].h.value)
    ts = (C.c_void_p * 2)(trees[0].h.value, trees[1].h.value)
    est = lib.sga_estimate_normals_covariances_batch
    assert est(ctx.h, cs, ts, 2, 20, 3) == 0
    assert est(ctx.h, cs, ts, 2, 0, 3) == INVALID and est(ctx.h, cs, ts, 2, 113, 3) == INVALID
    assert est(ctx.h, cs, None, 2, 20, 3) == INVALID
    assert est(ctx.h, cs, (C.c_void_p * 2)(trees[0].h.value, None), 2, 20, 3) == INVALID
    assert est(ctx.h, (C.c_void_p * 2)(good[0].h.value, good[0].h.value), (C.c_void_p * 2)(trees[0].h.value, lone[0].h.value), 2, 20, 3) == INVALID  # the same cloud twice
    assert est(ctx.h, cs, (C.c_void_p * 2)(trees[0].h.value, trees[0].h.value), 2, 20, 3) == INVALID  # the same index twice (and the wrong size)
    assert est(ctx.h, cs, (C.c_void_p * 2)(trees[1].h.value, trees[0].h.value), 2, 20, 3) == INVALID  # not built over their clouds (sizes)
    shifted = sga.PointCloud(good[2].xyz64() + tb.SHIFT)
    assert est(ctx.h, (C.c_void_p * 1)(shifted.h.value), (C.c_void_p * 1)(trees[2].h.value), 1, 20, 3) == INVALID  # same size, another frame
    ring = sga.PointCloud(cut(200, 72))
    proj = sga.ProjectiveSearch(ring, 64, 32)
    assert est(ctx.h, (C.c_void_p * 1)(ring.h.value), (C.c_void_p * 1)(proj.h.value), 1, 20, 3) == UNSUPPORTED
    covd = sga.PointCloud(cut(200, 72))
    sga.estimate_covariances(covd, None, 10)
    vm = sga.GaussianVoxelMap(1.0)
    vm.insert(covd)
    assert est(ctx.h, (C.c_void_p * 1)(covd.h.value), (C.c_void_p * 1)(vm.h.value), 1, 20, 3) == INVALID
    assert b"kd-tree" in lib.sga_last_error()
    # count == 0, and the trees of the failed calls above were left usable
    assert est(ctx.h, None, None, 0, 20, 3) == 0 and lib.sga_index_build_kdtree_batch(ctx.h, None, 0, None) == 0
    assert sga.build_kdtrees([]) == [] and sga.preprocess_batch([]) == []
    same_index(trees[1], lone[1], "after the validation errors")


def test_launch_count_does_not_grow_with_the_forest():
    """Check 8: 16 clouds of equal depth enqueue as many kernels as one such cloud (tree build and covariances)."""
    clouds = [sga.PointCloud(cut(11_000 + 37 * j, 80 + j)) for j in range(16)]  # all of depth 11, one split instantiation per level

    def launches(cs):
        before = sga.forest_launches()
        pairs = sga.preprocess_batch(cs, 20)
        del pairs
        return sga.forest_launches() - before

    one, sixteen = launches(clouds[:1]), launches(clouds)
    print("forest launches: 1 cloud %d, 16 clouds %d" % (one, sixteen))
    assert one == sixteen and one > 0

"""Fixed-radius neighbourhoods on the device (csrc/kd_radius.hpp, cloud_radius.hip, cloud_cluster.hip) against
the fp64 restatement of tests/cluster_ref.py, which never goes through the library.

The condition of every case: the restatement finds ZERO band pairs, band points and band ties in its input (cluster_ref: decisions that
hang on less than 1e-12 relative).  That is asserted first; it is a condition on the input, not a tolerance (if it ever fails: another
seed).  Then labels, seeds, sizes, the three counts and the boxes are compared for equality, the radius search's counts exactly and its
lists as sets sorted by index.

The bound on a list's squared distance.  Device and restatement form the same dx, dy, dz (the same double subtraction of the same
operands) and then three squares and two sums of non-negative terms; each of the five operations is rounded once (relative 2^-53 = u),
a fused multiply-add saves one, so each side lies within (1 + u)^3 - 1 < 3.01 u of the exact sum: the two differ by at most 6.02 u.
D2_RTOL = 8 u."""
import ctypes as C
import functools

import numpy as np
import pytest

import cluster_ref as ref
import small_gicp_amd as sga
from small_gicp_amd import api, odometry, synthetic
from test_cloud_merge_gpu import attributes, records, upload_relative

pytestmark = pytest.mark.gpu

F32 = np.float32
ZERO = np.zeros(3)
D2_RTOL = 8 * 2.0**-53
NO_BAND = {"pairs": 0, "points": 0, "ties": 0}


# ---- inputs (fp32 records, fixed seeds) and references, computed once -------------------------------------------------------------------
def frozen(p):
    p = np.ascontiguousarray(p, dtype=F32).reshape(-1, 3)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def scatter(n, seed=None):
    """n points uniform in a cube whose side gives a handful of neighbours within 0.5 m: clusters, pairs and singletons together"""
    side = max(1.0, (n / 1.5) ** (1.0 / 3.0))
    return frozen(np.random.default_rng(1000 + n if seed is None else seed).uniform(0.0, side, (n, 3)))


@functools.lru_cache(maxsize=None)
def singletons():
    g = np.stack(np.meshgrid(np.arange(5), np.arange(5), np.arange(4), indexing="ij"), -1).reshape(-1, 3) * 2.0
    return frozen(np.random.default_rng(7).permutation(g))


@functools.lru_cache(maxsize=None)
def blob():
    return frozen(np.random.default_rng(8).uniform(0.0, 0.25, (2000, 3)))  # the cube's diagonal is 0.433 < 0.5: every pair is an edge


@functools.lru_cache(maxsize=None)
def chains(count):
    """`count` chains of 4096 points spaced 0.9 eps (eps = 0.5) along x, 2 eps apart in y, the cloud indices shuffled over all of them"""
    x = np.arange(4096) * 0.45
    p = np.concatenate([np.stack([x, np.full(4096, 1.0 * c), np.zeros(4096)], 1) for c in range(count)])
    return frozen(np.random.default_rng(9 + count).permutation(p))


@functools.lru_cache(maxsize=None)
def lattice():
    g = np.stack(np.meshgrid(np.arange(16), np.arange(16), np.arange(16), indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    return frozen(np.random.default_rng(10).permutation(g))


@functools.lru_cache(maxsize=None)
def duplicated():
    p = scatter(300, seed=11)
    return frozen(np.random.default_rng(12).permutation(np.concatenate([p, p, p])))


@functools.lru_cache(maxsize=None)
def street():
    """synthetic.kitti_like_scan(0) with 3 % isolated returns, within 30 m, above the ground, as 0.25 m voxel means (plain numpy): walls,
    their edges, stray returns"""
    pts, _ = synthetic.kitti_like_scan(0)
    p = synthetic.with_isolated_returns(pts, 0.03, seed=21)[0].astype(np.float64)
    p = p[(np.linalg.norm(p, axis=1) < 30.0) & (p[:, 2] > -1.5)]
    cell = np.floor(p / 0.25).astype(np.int64)
    _, inv = np.unique(cell, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    count = np.bincount(inv)
    return frozen(np.stack([np.bincount(inv, p[:, a]) / count for a in range(3)], 1))


@functools.lru_cache(maxsize=None)
def want(maker, radius, min_points=1, min_size=1, max_size=None, origin=(0.0, 0.0, 0.0), args=()):
    return ref.cluster(maker(*args), radius, min_points, min_size, max_size, origin)


def compare(got, w, what=""):
    print("%s: n %d  clusters %d (%d)  noise %d (%d)  dropped %d (%d)  core %d  band %s" % (what, len(w["labels"]), got["num_clusters"], w["num_clusters"], got["noise"], w["noise"], got["dropped"], w["dropped"],
                                                                                     int(w["core"].sum()), w["band"]))
    assert w["band"] == NO_BAND, (what, w["band"])
    assert got["labels"].dtype == np.int32 and np.array_equal(got["labels"], w["labels"]), what
    assert (got["num_clusters"], got["noise"], got["dropped"]) == (w["num_clusters"], w["noise"], w["dropped"]), what
    assert np.array_equal(got["seeds"], w["seeds"]) and np.array_equal(got["sizes"], w["sizes"]), what
    assert got["boxes"].shape == w["boxes"].shape and got["boxes"].dtype == np.float64 and np.array_equal(got["boxes"], w["boxes"]), what


def run(maker, radius, min_points=1, min_size=1, max_size=None, origin=ZERO, args=(), tree=False, what=""):
    rel = maker(*args)
    cloud = upload_relative(rel, None, None, origin) if len(rel) else sga.PointCloud(np.zeros((0, 3), F32))
    w = want(maker, radius, min_points, min_size, max_size, tuple(float(v) for v in origin), args)
    got = cloud.clusters(radius, min_points, min_size, max_size, tree=sga.KdTree(cloud) if tree else None)
    compare(got, w, what or "%s%s eps %g min_points %d" % (maker.__name__, args, radius, min_points))
    return cloud, got, w


# ---- clustering ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 5000])
@pytest.mark.parametrize("min_points", [1, 3])
def test_sizes_around_a_wave_a_workgroup_and_the_prefix(n, min_points):
    run(scatter, 0.5, min_points, args=(n,), tree=n % 2 == 1)


def test_all_singletons():
    _, got, _ = run(singletons, 0.5)
    assert got["num_clusters"] == 100 and np.array_equal(got["labels"], np.arange(100)) and (got["sizes"] == 1).all()
    _, got, _ = run(singletons, 0.5, min_points=2)
    assert got["num_clusters"] == 0 and got["noise"] == 100


def test_one_blob_every_pair_an_edge():
    _, got, _ = run(blob, 0.5)
    assert got["num_clusters"] == 1 and got["sizes"].tolist() == [2000] and got["seeds"].tolist() == [0]
    run(blob, 0.5, min_points=2000)
    _, got, _ = run(blob, 0.5, min_points=2001)
    assert got["noise"] == 2000


def test_a_shuffled_chain_is_one_component():
    _, got, _ = run(chains, 0.5, args=(1,))
    assert got["num_clusters"] == 1 and got["sizes"].tolist() == [4096]
    run(chains, 0.5, min_points=3, args=(1,))  # the two ends become border points


def test_two_interleaved_chains_are_never_merged():
    _, got, _ = run(chains, 0.5, args=(2,))
    assert got["num_clusters"] == 2 and got["sizes"].tolist() == [4096, 4096]


@pytest.mark.parametrize("radius, min_points", [(1.2, 1), (1.5, 1), (1.2, 7), (1.5, 19)])
def test_a_lattice_has_distance_ties_and_no_band(radius, min_points):
    _, got, w = run(lattice, radius, min_points)
    if min_points == 1:
        assert got["num_clusters"] == 1 and got["sizes"].tolist() == [4096]
    else:
        assert int(w["core"].sum()) == 14**3 and got["num_clusters"] == 1  # the interior is core, faces are border, the rest is noise


def test_duplicated_points():
    run(duplicated, 0.5)
    run(duplicated, 0.5, min_points=4)
    run(duplicated, 1e-6, min_points=3)  # every triple is a cluster of its own


def exact_pair():
    return frozen([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])


def test_the_double_predicate_decides_inside_fp32_resolution():
    """distance exactly 1, eps = 1 +- 1e-9: outside the 1e-12 band and far inside what fp32 resolves (6e-8)"""
    _, got, _ = run(exact_pair, 1.0 + 1e-9)
    assert got["labels"].tolist() == [0, 0]
    _, got, _ = run(exact_pair, 1.0 - 1e-9)
    assert got["labels"].tolist() == [0, 1]
    tree = sga.KdTree(upload_relative(exact_pair(), None, None, ZERO))
    assert tree.radius_search(tree.cloud, 1.0 + 1e-9, return_lists=False).tolist() == [2, 2]
    assert tree.radius_search(tree.cloud, 1.0 - 1e-9, return_lists=False).tolist() == [1, 1]


def test_an_origin_256_km_away():
    origin = np.array([256000.0, -256000.0, 128.0])
    cloud, got, w = run(scatter, 0.5, 3, origin=origin, args=(2049,))
    assert np.array_equal(cloud.origin(), origin) and (got["boxes"][:, 0, 0] > 255999.0).all()
    assert np.array_equal(got["labels"], want(scatter, 0.5, 3, args=(2049,))["labels"])  # the labels do not depend on the frame


@pytest.mark.parametrize("min_points", [1, 4, 10])
def test_a_street_scene_has_clusters_border_points_and_noise(min_points):
    _, got, w = run(street, 0.5, min_points)
    assert got["num_clusters"] > 1
    if min_points > 1:
        assert got["noise"] > 0 and int((~w["core"] & (w["labels"] >= 0)).sum()) > 0  # noise and border points are both there


@pytest.mark.parametrize("min_size, max_size", [(10, None), (1, 50), (5, 200)])
def test_the_size_filter_renumbers(min_size, max_size):
    _, got, w = run(street, 0.5, 1, min_size, max_size)  # (min_points 1: the stray returns are clusters of one)
    assert got["dropped"] > 0 and got["noise"] == 0 and 0 < got["num_clusters"] < want(street, 0.5, 1)["num_clusters"]


def test_keep_returns_the_clustered_points_or_the_rest():
    rel = street()
    rng = np.random.default_rng(3)
    nrm = rng.normal(size=rel.shape).astype(F32)
    cov6 = rng.uniform(0.1, 1.0, (len(rel), 6)).astype(F32)
    cloud = upload_relative(rel, nrm, cov6, ZERO)
    w = want(street, 0.5, 4, 10)
    for keep, mask in (("clustered", w["labels"] >= 0), ("rest", w["labels"] < 0)):
        got = cloud.clusters(0.5, 4, 10, keep=keep)
        compare(got, w, keep)
        idx = np.nonzero(mask)[0]
        assert np.array_equal(got["kept"], idx) and got["cloud"].size() == len(idx) and 0 < len(idx) < len(rel)
        sel = cloud.selected(idx)
        assert np.array_equal(records(got["cloud"])[0], records(sel)[0]) and np.array_equal(records(got["cloud"])[0], rel[idx])
        for a, b in zip(attributes(got["cloud"]), attributes(sel)):
            assert np.array_equal(a, b)
        assert np.array_equal(got["cloud"].origin(), cloud.origin())


def test_the_cloud_s_own_tree_a_temporary_one_and_two_calls_give_the_same_bytes():
    cloud = upload_relative(street(), None, None, ZERO)
    tree = sga.KdTree(cloud)
    a, b, c = cloud.clusters(0.5, 4, tree=tree), cloud.clusters(0.5, 4), cloud.clusters(0.5, 4, tree=tree)
    for x in (b, c):
        for name in ("labels", "seeds", "sizes", "boxes"):
            assert a[name].tobytes() == x[name].tobytes(), name
        assert (a["num_clusters"], a["noise"], a["dropped"]) == (x["num_clusters"], x["noise"], x["dropped"])
    compare(a, want(street, 0.5, 4), "own tree")


def test_a_table_capacity_limits_the_rows_not_the_count():
    cloud = upload_relative(street(), None, None, ZERO)
    w = want(street, 0.5, 4)
    got = cloud.clusters(0.5, 4, table_capacity=3)
    assert got["num_clusters"] == w["num_clusters"] > 3 and np.array_equal(got["seeds"], w["seeds"][:3]) and np.array_equal(got["boxes"], w["boxes"][:3]) and np.array_equal(got["labels"], w["labels"])
    got = cloud.clusters(0.5, 4, return_table=False)
    assert "seeds" not in got and np.array_equal(got["labels"], w["labels"])


def test_launches_and_waits():
    cloud = upload_relative(scatter(2049), None, None, ZERO)
    tree = sga.KdTree(cloud)

    def counted(fn):
        before = (sga.cloud_cluster_launches(), sga.radius_search_launches(), sga.radius_waits())
        fn()
        return tuple(a - b for a, b in zip((sga.cloud_cluster_launches(), sga.radius_search_launches(), sga.radius_waits()), before))

    cap = 2048  # (room for every row: PointCloud.clusters calls a second time when its default table is too small)
    assert counted(lambda: cloud.clusters(0.5, tree=tree, table_capacity=cap)) == (6, 0, 1)
    assert counted(lambda: cloud.clusters(0.5, table_capacity=cap)) == (6, 0, 1)  # (the temporary tree's build is not counted here)
    assert counted(lambda: cloud.clusters(0.5, 3, tree=tree, table_capacity=cap)) == (8, 0, 1)
    assert counted(lambda: cloud.clusters(0.5, 3, tree=tree, keep="rest", table_capacity=cap)) == (10, 0, 1)
    assert counted(lambda: cloud.clusters(0.5, tree=tree, keep="clustered", return_table=False)) == (8, 0, 1)
    assert counted(lambda: cloud.clusters(0.5, tree=tree)) == (12, 0, 2)  # 1349 clusters, 1024 rows: called again with room for all
    assert counted(lambda: sga.PointCloud(np.zeros((0, 3), F32)).clusters(0.5)) == (0, 0, 0)
    assert counted(lambda: tree.radius_search(cloud, 0.5, return_lists=False)) == (0, 2, 1)
    assert counted(lambda: tree.radius_search(cloud, 0.5, capacity=1 << 20)) == (0, 5, 2)
    assert counted(lambda: tree.radius_search(cloud, 0.5, capacity=1)) == (0, 2 + 5, 1 + 2)  # the lists did not fit: counted, then called again
    assert counted(lambda: tree.radius_search(sga.PointCloud(np.zeros((0, 3), F32)), 0.5)) == (0, 0, 0)


def test_refusals_on_real_handles():
    rel = scatter(2049)
    cloud = upload_relative(rel, None, None, ZERO)
    tree = sga.KdTree(cloud)
    before = (sga.cloud_cluster_launches(), sga.radius_search_launches(), sga.radius_waits())
    bad = rel.copy()
    bad[17, 1] = np.nan
    with pytest.raises(sga.SgaError, match="contains non-finite coordinates"):
        upload_relative(bad, None, None, ZERO).clusters(0.5)
    with pytest.raises(sga.SgaError, match="index was built over a cloud of 2048 points, got 2049"):
        cloud.clusters(0.5, tree=sga.KdTree(upload_relative(rel[:2048], None, None, ZERO)))
    with pytest.raises(sga.SgaError, match="device frames differ"):
        cloud.clusters(0.5, tree=sga.KdTree(upload_relative(rel, None, None, np.array([128.0, 0.0, 0.0]))))
    with pytest.raises(sga.SgaError, match="projective"):
        cloud.clusters(0.5, tree=sga.ProjectiveSearch(rel, 64, 32))
    for kw, word in (({"radius": 0.0}, "radius must be finite"), ({"radius": -1.0}, "radius must be finite"), ({"radius": np.inf}, "radius must be finite"), ({"radius": np.nan}, "radius must be finite"),
                     ({"radius": 0.5, "min_points": 0}, "min_points 0 is below 1"), ({"radius": 0.5, "min_size": 5, "max_size": 4}, "min_size 5 is above max_size 4")):
        with pytest.raises(sga.SgaError, match=word):
            cloud.clusters(tree=tree, **kw)
    for radius in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(sga.SgaError, match="radius must be finite"):
            tree.radius_search(cloud, radius)
    with pytest.raises(sga.SgaError, match="projective"):
        sga.KdTree.radius_search(sga.ProjectiveSearch(rel, 64, 32), cloud, 0.5)
    if sga.load().sga_device_count() >= 2:
        far = upload_relative(rel, None, None, ZERO, sga.Context(1))
        with pytest.raises(sga.SgaError, match="cloud lives on another device"):
            api.check(sga.load().sga_cloud_cluster(cloud.ctx.h, far.h, None, C.byref(api._cluster_params(0.5)), None, None, 0, None, None, None))
        with pytest.raises(sga.SgaError, match="another device"):
            tree.radius_search(far, 0.5)
    else:
        print("ONE DEVICE ONLY: the refusal of a cloud that lives on another device was NOT exercised")
    assert (sga.cloud_cluster_launches(), sga.radius_search_launches(), sga.radius_waits()) == before  # nothing was enqueued


# ---- radius search ------------------------------------------------------------------------------------------------------------------------
def check_search(rel_t, o_t, rel_q, o_q, radius, what="", same=False):
    target = upload_relative(rel_t, None, None, o_t)
    tree = sga.KdTree(target)
    queries = target if same else upload_relative(rel_q, None, None, o_q)
    q64 = np.asarray(rel_q, F32).astype(np.float64) + (np.asarray(o_q, np.float64) - np.asarray(o_t, np.float64))
    lists, band = ref.neighbours(rel_t, q64, radius)
    assert band == 0, (what, band)
    counts, offsets, indices, sq = tree.radius_search(queries, radius)
    want_counts = np.array([len(i) for i, _ in lists], np.int64)
    print("%s: m %d  n %d  total %d (%d)  max count %d" % (what, len(rel_q), len(rel_t), len(indices), want_counts.sum(), want_counts.max() if len(want_counts) else 0))
    assert np.array_equal(counts, want_counts) and np.array_equal(tree.radius_search(queries, radius, return_lists=False), want_counts), what
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(want_counts)])) and len(indices) == len(sq) == want_counts.sum() and sq.dtype == np.float64, what
    worst = 0.0
    for i, (idx, d2) in enumerate(lists):
        seg = slice(offsets[i], offsets[i + 1])
        order = np.argsort(indices[seg], kind="stable")
        assert np.array_equal(indices[seg][order], idx), (what, i)
        err = np.abs(sq[seg][order] - d2)
        assert (err <= D2_RTOL * d2).all(), (what, i)
        worst = max(worst, float((err / np.maximum(d2, 1e-300)).max()) if len(d2) else 0.0)
    print("%s: worst relative difference of a squared distance %.2e (bound %.2e)" % (what, worst, D2_RTOL))
    return tree, queries, want_counts


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_radius_search_of_a_cloud_in_its_own_tree(n):
    check_search(scatter(n), ZERO, scatter(n), ZERO, 0.5, "scatter %d" % n, same=True)


@pytest.mark.parametrize("maker, radius", [(singletons, 0.5), (blob, 0.5), (lattice, 1.2), (lattice, 1.5), (duplicated, 0.5), (street, 0.5)])
def test_radius_search_on_the_special_shapes(maker, radius):
    check_search(maker(), ZERO, maker(), ZERO, radius, "%s eps %g" % (maker.__name__, radius), same=True)


def test_radius_search_of_a_shuffled_chain():
    check_search(chains(1), ZERO, chains(1), ZERO, 0.5, "chain", same=True)


def test_radius_search_with_queries_of_another_cloud_and_another_frame():
    check_search(scatter(2049), ZERO, scatter(777, seed=5), ZERO, 0.5, "other cloud")
    o_t, o_q = np.array([256000.0, -256000.0, 128.0]), np.array([256000.0 + 128.0, -256000.0, 0.0])
    rel_q = frozen(scatter(777, seed=5).astype(np.float64) - (o_q - o_t))  # the same region seen from another origin: the records differ, and q != float(q)
    check_search(scatter(2049), o_t, rel_q, o_q, 0.5, "other frame")


def test_radius_search_when_the_lists_do_not_fit_and_without_queries():
    tree, cloud, want_counts = check_search(scatter(2049), ZERO, scatter(2049), ZERO, 0.5, "capacity", same=True)
    m, total = len(want_counts), int(want_counts.sum())
    I64 = C.POINTER(C.c_int64)
    counts, offsets = np.full(m, -1, np.int64), np.full(m + 1, -1, np.int64)
    indices, sq = np.full(total, -7, np.int64), np.full(total, -7.0)
    res = api._lib.RadiusResult()
    call = lambda cap: sga.load().sga_index_radius_search(cloud.ctx.h, tree.h, cloud.h, 0.5, cap, counts.ctypes.data_as(I64), offsets.ctypes.data_as(I64), indices.ctypes.data_as(I64), api._dp(sq), C.byref(res))
    assert call(total - 1) == 0 and (res.total, res.written, res.overflow) == (total, 0, 1)
    assert np.array_equal(counts, want_counts) and offsets[-1] == total and (indices == -7).all() and (sq == -7.0).all()  # counted, not written
    assert call(total) == 0 and (res.total, res.written, res.overflow) == (total, total, 0) and (indices >= 0).all()
    empty = sga.PointCloud(np.zeros((0, 3), F32))
    c, o, i, d = tree.radius_search(empty, 0.5)
    assert len(c) == 0 and o.tolist() == [0] and len(i) == 0 and len(d) == 0
    c = sga.KdTree(empty).radius_search(cloud, 0.5, return_lists=False)
    assert c.tolist() == [0] * m


# ---- end to end: the mover's track ---------------------------------------------------------------------------------------------------------
def test_the_seen_through_points_of_a_mover_are_one_cluster_around_it():
    """Asserted on the restatement first — tests/visibility_ref.py + tests/cluster_ref.py over the library's own keyframe records: for
    each of frames 1 .. 7 the seen-through points hold exactly one cluster of at least 10 points, every member within 1.1 m of the
    sphere's centre — then the device's labels equal the restatement's on those points."""
    import visibility_ref

    frames = odometry.run_synthetic_movers(num_frames=8, radius=0.5, min_size=10)
    assert [r["frame"] for r in frames] == list(range(1, 8))
    for r in frames:
        key_rel, scan_rel = records(r["keyframe"])[0], records(r["scan"])[0]
        vis = visibility_ref.restate(key_rel, scan_rel, r["keyframe"].origin(), r["T"], r["scan"].origin())
        idx = visibility_ref.kept(vis, "seen_through")
        assert set(np.setxor1d(r["kept"], idx).tolist()) <= set(vis["band"].tolist()), r["frame"]  # (the device may state a band point of the visibility otherwise)
        seen_rel = records(r["seen"])[0]
        assert np.array_equal(seen_rel, key_rel[r["kept"]])
        if not np.array_equal(r["kept"], idx):  # the property is the restatement's: on its own seen-through points
            own = ref.cluster(key_rel[idx], 0.5, 1, 10, None, r["keyframe"].origin())
            near = np.linalg.norm(key_rel[idx][own["labels"] == 0].astype(np.float64) + r["keyframe"].origin() - r["centre"], axis=1)
            assert own["band"] == NO_BAND and own["num_clusters"] == 1 and own["sizes"][0] >= 10 and near.max() <= 1.1, r["frame"]
        w = ref.cluster(seen_rel, 0.5, 1, 10, None, r["seen"].origin())
        assert w["band"] == NO_BAND, (r["frame"], w["band"])
        members = seen_rel[w["labels"] == 0].astype(np.float64) + r["seen"].origin()
        far = np.linalg.norm(members - r["centre"], axis=1).max() if len(members) else np.inf
        print("frame %d: %d seen-through points, %d clusters of >= 10 (sizes %s), farthest member %.3f m from the sphere's centre, centroid %.3f m"
              % (r["frame"], len(idx), w["num_clusters"], w["sizes"].tolist(), far, np.linalg.norm(members.mean(axis=0) - r["centre"]) if len(members) else np.nan))
        assert w["num_clusters"] == 1 and w["sizes"][0] >= 10 and far <= 1.1, r["frame"]
        assert np.array_equal(r["labels"], w["labels"]), r["frame"]
        assert [d["seed"] for d in r["detections"]] == w["seeds"].tolist() and [d["size"] for d in r["detections"]] == w["sizes"].tolist()
        assert np.array_equal(np.stack([d["box"] for d in r["detections"]]), w["boxes"])


# ---- the C++ header -----------------------------------------------------------------------------------------------------------------------
def test_cpp_clusters_and_radius_search(tmp_path):
    """include/small_gicp_amd.hpp: ClusterParams, PointCloud::clusters and KdTree::radius_search against a host loop
    (tests/cpp/test_cpp_cloud_cluster.cpp, compiled with g++ as test_cloud_outliers_gpu.py compiles its program)."""
    import os
    import subprocess

    from conftest import ROOT

    exe = tmp_path / "test_cpp_cloud_cluster"
    libdir = os.path.dirname(sga.LIB_PATH)
    cmd = ["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_cpp_cloud_cluster.cpp"), "-o", str(exe), "-L" + libdir, "-lsmall_gicp_amd",
           "-Wl,-rpath," + libdir, "-Wl,-rpath-link,/opt/rocm/lib"]
    subprocess.check_call(cmd)
    pts, _ = synthetic.kitti_like_scan(0)
    pts = np.ascontiguousarray(synthetic.with_isolated_returns(pts[::6], 0.01)[0], dtype=F32)  # every sixth point, with scatter
    (tmp_path / "p.f32").write_bytes(pts.tobytes())
    p = subprocess.run([str(exe), str(tmp_path / "p.f32")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    print(p.stdout)
    rows = [ln.split() for ln in p.stdout.splitlines()]
    out = [r for r in rows if r[0] == "CLUSTER"]
    assert len(out) == 2 and [r[1] for r in out] == ["1", "4"]
    for r in out:  # CLUSTER min_points clusters c noise x dropped y equal e table t tree s keep k
        assert int(r[3]) > 1 and int(r[5]) + int(r[7]) > 0 and r[9] == "1" and r[11] == "1" and r[13] == "1" and r[15] == "1", r
    radius = [r for r in rows if r[0] == "RADIUS"]
    assert len(radius) == 1 and int(radius[0][2]) > 0 and radius[0][4] == "1", radius
    assert [r for r in rows if r[0] == "REFUSE"] == [["REFUSE", "equal", "1"]]

"""The voxel-map searches restated in numpy, float64: which voxel or stored point a query is paired with.

No device and no project code.  The rules (ann/incremental_voxelmap.hpp:99-186, ann/knn_result.hpp:80-100, ann/flat_container.hpp:84-107,
ann/gaussian_voxelmap.hpp:83-86, util/fast_floor.hpp:12-15 of the reference):

  * the query's voxel is fast_floor((q + org) * (1 / leaf)): q in the frame the records are stored in, org that frame's origin;
  * the voxels at the search offsets are visited in order: the centre, then +x +y +z -x -y -z (7), or the centre and then the 3 x 3 x 3
    cube in i, j, k order (27: 28 visits, the centre twice);
  * a visited coordinate with abs(c) >= 2^20 on any axis offers nothing (the 21-bit hash key ends there);
  * a Gaussian voxel offers its mean, a flat voxel its points in slot order;
  * 1-NN: a strictly smaller distance wins, so the first of equal distances is kept;
  * k-NN: the list of KnnResult::push, one candidate after the other.

A map is given as `coords` (V, 3) integers, one row per voxel id, with either `means` (V, 3) or `points` (V, 16, 3) and `counts` (V,).
"""
import numpy as np

LIMIT = 1 << 20
CAP = 16
_CUBE = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
OFFSETS = {
    1: [(0, 0, 0)],
    7: [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1)],
    27: [(0, 0, 0)] + _CUBE,  # set_search_offsets(27) appends the cube to the default list
}


def fast_floor(x):
    """util/fast_floor.hpp: truncate, then subtract one where the value lies below its truncation"""
    x = np.asarray(x, dtype=np.float64)
    n = np.trunc(x)
    return (n - (x < n)).astype(np.int64)


def voxel_of(queries, leaf, org):
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    return fast_floor((q + np.asarray(org, dtype=np.float64)) * (1.0 / float(leaf)))


def _pack(c):
    """(n, 3) integer coordinates -> one int64 key each; -1 where a coordinate is out of the map's range"""
    c = np.asarray(c, dtype=np.int64).reshape(-1, 3)
    ok = (np.abs(c) < LIMIT).all(1)
    s = c + LIMIT
    key = (s[:, 0] << 42) | (s[:, 1] << 21) | s[:, 2]
    return np.where(ok, key, -1)


class _Table:
    def __init__(self, coords):
        key = _pack(coords)
        assert (key >= 0).all() and len(np.unique(key)) == len(key), "voxel coordinates must be distinct and within +-2^20"
        self.order = np.argsort(key, kind="stable")
        self.keys = key[self.order]

    def find(self, c):
        """voxel id per coordinate, -1 = no such voxel"""
        key = _pack(c)
        if len(self.keys) == 0:
            return np.full(len(key), -1, np.int64)
        pos = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        return np.where((key >= 0) & (self.keys[pos] == key), self.order[pos], -1).astype(np.int64)


def _records(means, points, counts):
    if means is not None:
        m = np.asarray(means, dtype=np.float64).reshape(-1, 1, 3)
        return m, np.ones(len(m), np.int64), False
    p = np.asarray(points, dtype=np.float64).reshape(-1, CAP, 3)
    return p, np.asarray(counts, dtype=np.int64).reshape(-1), True


def _sq_dist(p, q):
    d = p - q
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]


def nearest(coords, leaf, org, offsets, queries, means=None, points=None, counts=None):
    """-> (index (n,) int64, d2 (n,), runner-up d2 (n,)): the voxel id (Gaussian map), (voxel << 32) | slot (flat map) or -1; inf where
    there is none.  The runner-up is the smallest distance among the other candidates (the second visit of the centre aside)."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    rec, cnt, flat = _records(means, points, counts)
    table = _Table(coords)
    centre = voxel_of(q, leaf, org)
    n = len(q)
    idx = np.full(n, -1, np.int64)
    best = np.full(n, np.inf)
    second = np.full(n, np.inf)
    for v, o in enumerate(OFFSETS[offsets]):
        if offsets == 27 and v > 0 and o == (0, 0, 0):
            continue  # the centre again: an equal distance never replaces the first
        vox = table.find(centre + np.asarray(o, np.int64))
        safe = np.maximum(vox, 0)
        for s in range(rec.shape[1]):
            ok = (vox >= 0) & (s < cnt[safe])
            d2 = np.where(ok, _sq_dist(rec[safe, s], q), np.inf)
            win = ok & (d2 < best)
            second = np.where(win, best, np.where(ok & (d2 < second), d2, second))
            best = np.where(win, d2, best)
            idx = np.where(win, ((vox << 32) | s) if flat else vox, idx)
    return idx, best, second


def knn(coords, leaf, org, offsets, queries, k, max_sq=None, means=None, points=None, counts=None, dtype=np.float32):
    """-> (indices (n, k) int64, d2 (n, k) float64): the k-best list, -1 / inf in the unused slots.  Indices are (voxel << 32) | slot for
    both families.  Distances are formed in float64 and rounded to `dtype` before they are compared: float32 is the device's list
    (fp32 records, fp32 query), float64 the reference's."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    rec, cnt, _ = _records(means, points, counts)
    table = _Table(coords)
    centre = voxel_of(q, leaf, org)
    cap = np.inf if max_sq is None else float(dtype(max_sq))
    visits = [table.find(centre + np.asarray(o, np.int64)) for o in OFFSETS[offsets]]
    out_i = np.full((len(q), k), -1, np.int64)
    out_d = np.full((len(q), k), np.inf)
    for r in range(len(q)):
        ids, ds, found = out_i[r], out_d[r], 0
        for vox in (int(v[r]) for v in visits):
            if vox < 0:
                continue
            for s in range(int(cnt[vox])):
                d = float(dtype(_sq_dist(rec[vox, s], q[r])))
                if d > cap or d >= ds[k - 1]:
                    continue
                loc = min(found, k - 1)
                while loc > 0 and d < ds[loc - 1]:
                    ids[loc], ds[loc] = ids[loc - 1], ds[loc - 1]
                    loc -= 1
                ids[loc], ds[loc] = (vox << 32) | s, d
                found = min(found + 1, k)
    return out_i, out_d


def ambiguous(queries, leaf, org, delta, best, second, bound):
    """-> (near_face (n,) bool, near_tie (n,) bool).  near_face: the query lies within delta (n,) of a voxel face on some axis, so a query
    moved by up to delta may fall into the neighbouring voxel.  near_tie: the distances (not squared) to the best and to the runner-up
    candidate differ by less than bound (n,), so arithmetic that is off by up to bound / 2 per distance may order them the other way."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    x = (q + np.asarray(org, dtype=np.float64)) * (1.0 / float(leaf))
    to_face = np.abs(x - np.rint(x)) * float(leaf)
    near_face = (to_face <= np.asarray(delta, dtype=np.float64).reshape(-1, 1)).any(1)
    b, s = np.sqrt(np.asarray(best, dtype=np.float64)), np.sqrt(np.asarray(second, dtype=np.float64))
    with np.errstate(invalid="ignore"):
        near_tie = np.isfinite(s) & (s - b < np.asarray(bound, dtype=np.float64))
    return near_face, near_tie


def admissible(coords, leaf, org, offsets, query, delta, bound, means=None, points=None, counts=None):
    """What a search may answer for ONE query known only to within delta per axis, with distances known to within bound / 2: for every
    voxel the moved query can start from, every candidate of that start whose distance is within bound of that start's minimum (-1 where
    a start finds nothing).  -> {index: d2}"""
    q = np.asarray(query, dtype=np.float64).reshape(3)
    rec, cnt, flat = _records(means, points, counts)
    table = _Table(coords)
    axes = []
    for a in range(3):
        axes.append(sorted({int(voxel_of(np.array([q + e]), leaf, org)[0, a]) for e in (-delta, 0.0, delta)}))
    out = {}
    for cx in axes[0]:
        for cy in axes[1]:
            for cz in axes[2]:
                cand = {}
                for o in OFFSETS[offsets]:
                    vox = int(table.find(np.array([[cx + o[0], cy + o[1], cz + o[2]]]))[0])
                    if vox < 0:
                        continue
                    for s in range(int(cnt[vox])):
                        cand[((vox << 32) | s) if flat else vox] = float(_sq_dist(rec[vox, s], q))
                if not cand:
                    out[-1] = np.inf
                    continue
                dmin = np.sqrt(min(cand.values()))
                out.update({i: d for i, d in cand.items() if np.sqrt(d) <= dmin + bound})
    return out

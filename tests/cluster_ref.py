"""The fixed-radius rules of DESIGN.md section 3.26 restated in numpy float64, never through the library: the radius predicate over all
pairs, and DBSCAN with the deterministic border rule — core flags, the components of the core graph, the border points' nearest core
point (ties: the lowest index), the size filter, the numbering by seed, the boxes.  Also the BAND: the pairs, points and border ties
whose decision hangs on less than 1e-12 relative, where an implementation that forms its sums in another order may differ.

Records are the fp32 values the device holds (a cloud's points minus its origin); d2 = ((dx dx) + (dy dy)) + (dz dz) in double."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

BAND = 1e-12


def sq_dists(q64, rec64):
    """(len(q), len(rec)) squared distances in double: three squares, two sums, in that order"""
    dx = q64[:, None, 0] - rec64[None, :, 0]
    dy = q64[:, None, 1] - rec64[None, :, 1]
    dz = q64[:, None, 2] - rec64[None, :, 2]
    return (dx * dx + dy * dy) + dz * dz


def neighbours(records, queries64, radius, block=512):
    """For every query (float64 (m,3), the records' frame) the records (float32 (n,3)) with d2 <= radius^2.  Returns (lists, band_pairs):
    lists[i] = (indices ascending, their d2); band_pairs = the (query, record) pairs with |d2 - radius^2| <= 1e-12 radius^2."""
    rec = np.asarray(records, np.float32).reshape(-1, 3).astype(np.float64)
    q = np.asarray(queries64, np.float64).reshape(-1, 3)
    r2 = float(radius) * float(radius)
    lists, band = [], 0
    for s in range(0, len(q), block):
        d2 = sq_dists(q[s : s + block], rec)
        band += int((np.abs(d2 - r2) <= BAND * r2).sum())
        for row in d2:
            idx = np.nonzero(row <= r2)[0]
            lists.append((idx.astype(np.int64), row[idx]))
    return lists, band


def cluster(records, radius, min_points=1, min_size=1, max_size=None, origin=(0.0, 0.0, 0.0)):
    """The clustering of the fp32 records (n,3).  Returns a dict: labels int32, num_clusters, noise, dropped, seeds, sizes (int64), boxes
    (C,2,3) float64 = min / max of the members' records + origin, core (bool), and band = {"pairs", "points", "ties"}."""
    rec32 = np.asarray(records, np.float32).reshape(-1, 3)
    n = len(rec32)
    lists, band_qr = neighbours(rec32, rec32.astype(np.float64), radius)
    r2 = float(radius) * float(radius)
    count = np.array([len(i) for i, _ in lists], np.int64)
    # the count with every band pair taken out / put in: a point whose core decision differs between the two hangs on a band pair
    lo, hi = count.copy(), count.copy()
    band_pairs = 0
    if band_qr:
        rec = rec32.astype(np.float64)
        for s in range(0, n, 512):
            d2 = sq_dists(rec[s : s + 512], rec)
            b = np.abs(d2 - r2) <= BAND * r2
            inside = d2 <= r2
            lo[s : s + 512] -= (b & inside).sum(axis=1)
            hi[s : s + 512] += (b & ~inside).sum(axis=1)
            band_pairs += int(b.sum())
        band_pairs //= 2  # (each unordered pair was met twice; a point is never in the band with itself: radius > 0)
    core = count >= int(min_points)
    band_points = int(((lo >= int(min_points)) != (hi >= int(min_points))).sum())
    # components of the core graph
    root = np.full(n, -1, np.int64)
    ci = np.nonzero(core)[0]
    if len(ci):
        rows = np.concatenate([np.full(len(lists[i][0]), i, np.int64) for i in ci])
        cols = np.concatenate([lists[i][0] for i in ci])
        keep = core[cols]
        g = coo_matrix((np.ones(int(keep.sum()), np.int8), (rows[keep], cols[keep])), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        seed_of = {}
        for i in ci:  # ascending: the first core point met of a component is its seed
            seed_of.setdefault(comp[i], i)
        for i in ci:
            root[i] = seed_of[comp[i]]
    # border points
    ties = 0
    for i in np.nonzero(~core)[0]:
        idx, d2 = lists[i]
        m = core[idx]
        if not m.any():
            continue
        idx, d2 = idx[m], d2[m]
        order = np.lexsort((idx, d2))
        if len(order) > 1 and d2[order[1]] - d2[order[0]] <= BAND * d2[order[1]]:
            ties += 1
        root[i] = root[idx[order[0]]]
    seeds_all, sizes_all = np.unique(root[root >= 0], return_counts=True)
    top = np.iinfo(np.int64).max if max_size is None else int(max_size)
    ok = (sizes_all >= int(min_size)) & (sizes_all <= top)
    seeds, sizes = seeds_all[ok].astype(np.int64), sizes_all[ok].astype(np.int64)
    number = {int(s): k for k, s in enumerate(seeds)}
    labels = np.array([number.get(int(r), -1) for r in root], np.int32).reshape(n)
    o = np.asarray(origin, np.float64)
    boxes = np.zeros((len(seeds), 2, 3))
    for k in range(len(seeds)):
        mem = rec32[labels == k]
        boxes[k, 0] = mem.min(axis=0).astype(np.float64) + o
        boxes[k, 1] = mem.max(axis=0).astype(np.float64) + o
    return {
        "labels": labels,
        "num_clusters": len(seeds),
        "noise": int((root < 0).sum()),
        "dropped": int(sizes_all[~ok].sum()),
        "seeds": seeds,
        "sizes": sizes,
        "boxes": boxes,
        "core": core,
        "band": {"pairs": band_pairs, "points": band_points, "ties": ties},
    }

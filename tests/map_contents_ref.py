"""What a voxel map holds after insert() restated in numpy, float64: a plain loop over the points.

No device and no project code.  The rules (ann/incremental_voxelmap.hpp:55-92, ann/gaussian_voxelmap.hpp:32-53, ann/flat_container.hpp:33-58,
util/fast_floor.hpp:12-15 of the reference):

  * input: the records the device holds, p' = fl32(p - o) with the origin o of the cloud's frame, fp32 normals and covariances, a 4x4 pose;
  * the posed point is x = R (p' + o) + t, its voxel fast_floor(x * (1 / leaf));
  * (the project's) a point is dropped when a coordinate of x is NaN or a voxel coordinate has |c| >= 2^20 (the 21-bit hash key ends there);
    decided on the double, so +-inf, +-3e38 and +-2^31 * leaf are dropped;
  * points are taken in cloud order; a voxel is created at its first point, voxel ids are the creation order; lru = counter at every touch;
  * Gaussian voxel: un-finalize (mean *= N, cov *= N), N++, mean += x, cov += R C R^T, then divide by N;
  * flat voxel: the point is kept iff count < max_points and no kept point has squared distance < min_sq (strict); a kept point stores x,
    R n (no translation) and R C R^T in slot order; lru is refreshed even when the point is rejected;
  * after the points, for any cloud including an empty one: counter++; if counter % clear_cycle == 0 every voxel with lru + horizon < counter
    is removed (no wrap at horizon 2^32 - 1); survivors keep their order and are renumbered;
  * the one-shot map is a single insert at the identity into an empty map.

Ambiguity is decided on the inputs: x is evaluated in np.longdouble as well.  A point is EXACT when the float64 evaluations R (p' + o) + t
and R p' + (R o + t) both equal the long-double value bit for bit (dyadic points and translations, rotation entries in {0, +-1}): its voxel
is decided even on a face.  Any other point is ambiguous when floor differs across u +- delta, delta = 8 * 2^-53 * (sum_j |R_ij| |p'_j + o_j|
+ |t_i|) / leaf.  A flat-map distance is ambiguous when it is not exact and lies within 16 * 2^-53 * d^2 + 2 d (err_a + err_b) of min_sq
(err: the 8 * 2^-53 * (...) of the two points; the second term is what an error of the coordinates does to the distance).
"""
import numpy as np

LIMIT = 1 << 20
CAP = 16
EPS = 2.0 ** -53
GAUSSIAN, FLAT = "gaussian", "flat"


def fast_floor(x):
    """util/fast_floor.hpp: truncate, then subtract one where the value lies below its truncation; as doubles (inf stays inf)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        n = np.trunc(x)
        return n - (x < n)


def _pose(T, dtype):
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64).reshape(4, 4)
    return T[:3, :3].astype(dtype), T[:3, 3].astype(dtype)


def posed(records, origin, T, dtype=np.float64):
    """x = R (p' + o) + t, row i as R_i0 q_0 + R_i1 q_1 + R_i2 q_2 + t_i"""
    R, t = _pose(T, dtype)
    q = np.asarray(records, dtype=np.float64).reshape(-1, 3).astype(dtype) + np.asarray(origin, dtype=np.float64).astype(dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        return q[:, 0:1] * R[:, 0] + q[:, 1:2] * R[:, 1] + q[:, 2:3] * R[:, 2] + t


def posed_split(records, origin, T):
    """x = R p' + (R o + t) in float64: the other order of the same sum"""
    R, t = _pose(T, np.float64)
    o = np.asarray(origin, dtype=np.float64)
    p = np.asarray(records, dtype=np.float64).reshape(-1, 3)
    tt = t + (R[:, 0] * o[0] + R[:, 1] * o[1] + R[:, 2] * o[2])
    with np.errstate(invalid="ignore", over="ignore"):
        return p[:, 0:1] * R[:, 0] + p[:, 1:2] * R[:, 1] + p[:, 2:3] * R[:, 2] + tt


def magnitude(records, origin, T):
    """sum_j |R_ij| |p'_j + o_j| + |t_i| per point and axis: the scale of the rounding errors of x"""
    R, t = _pose(T, np.float64)
    q = np.abs(np.asarray(records, dtype=np.float64).reshape(-1, 3) + np.asarray(origin, dtype=np.float64))
    with np.errstate(invalid="ignore", over="ignore"):
        return q @ np.abs(R).T + np.abs(t)


def exact_points(records, origin, T):
    """(n,) bool: both float64 evaluations of x equal the long-double one bit for bit"""
    xl = posed(records, origin, T, np.longdouble)
    a, b = posed(records, origin, T), posed_split(records, origin, T)
    with np.errstate(invalid="ignore"):
        return ((a.astype(np.longdouble) == xl) & (b.astype(np.longdouble) == xl)).all(1)


def dropped_points(x, leaf):
    """(n,) bool: a NaN coordinate, or a voxel coordinate the key cannot hold; decided on the double"""
    c = fast_floor(x * (1.0 / float(leaf)))
    with np.errstate(invalid="ignore"):
        return np.isnan(x).any(1) | ~(np.abs(c) < LIMIT).all(1)


def near_face(records, origin, T, leaf):
    """(n,) bool: not exact, and floor(u - delta) != floor(u + delta) on some axis"""
    x = posed(records, origin, T)
    inv = 1.0 / float(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        u, delta = x * inv, 8.0 * EPS * magnitude(records, origin, T) * inv
        differs = (np.floor(u - delta) != np.floor(u + delta)) & np.isfinite(u)
    return differs.any(1) & ~exact_points(records, origin, T)


def rotated_covs(T, covs):
    R, _ = _pose(T, np.float64)
    return R @ np.asarray(covs, dtype=np.float64).reshape(-1, 3, 3) @ R.T


class Voxel:
    def __init__(self, coord, lru):
        self.coord, self.lru, self.n = coord, lru, 0
        self.mean, self.cov, self.finalized = np.zeros(3), np.zeros((3, 3)), False  # Gaussian
        self.mag_mean, self.mag_cov = np.zeros(3), np.zeros((3, 3))                 # sums of the terms' magnitudes: the scale of the fp64 slack
        self.points, self.normals, self.covs, self.mags, self.exact, self.source = [], [], [], [], [], []  # flat, in slot order
        self.nmags, self.cmags = [], []


class Map:
    """kind GAUSSIAN or FLAT; a flat map keeps normals / covariances where insert() is given them"""

    def __init__(self, leaf, kind=GAUSSIAN, min_sq=0.01, max_points=10, horizon=100, clear_cycle=10):
        self.leaf, self.kind, self.min_sq, self.max_points = float(leaf), kind, float(min_sq), int(max_points)
        self.horizon, self.clear_cycle, self.counter = int(horizon), int(clear_cycle), 0
        self.voxels, self.index, self.inserts = [], {}, 0
        self.sweeps = []  # (counter, horizon, lru (V,) before the sweep, removed (V,) bool) of every sweep, for the tests of the tests

    def set_lru(self, horizon, clear_cycle):
        self.horizon, self.clear_cycle = int(horizon), int(clear_cycle)

    def insert(self, records, origin=(0.0, 0.0, 0.0), T=None, normals=None, covs=None):
        """-> (dropped (n,), kept (n,), ambiguous (n,)) bool: kept = the point entered a voxel's sums or slots; ambiguous = near a face, or
        (flat maps) decided by a distance near min_sq"""
        p = np.asarray(records, dtype=np.float64).reshape(-1, 3)
        n = len(p)
        x = posed(p, origin, T)
        R, _ = _pose(T, np.float64)
        mag = magnitude(p, origin, T)
        exact = exact_points(p, origin, T)
        drop = dropped_points(x, self.leaf)
        ambiguous = near_face(p, origin, T, self.leaf)
        kept = np.zeros(n, bool)
        with np.errstate(invalid="ignore", over="ignore"):
            coord = fast_floor(x * (1.0 / self.leaf))
        rc = None if covs is None else rotated_covs(T, covs)
        rc_mag = None if covs is None else np.abs(R) @ np.abs(np.asarray(covs, dtype=np.float64).reshape(-1, 3, 3)) @ np.abs(R).T
        rn = None if normals is None else np.asarray(normals, dtype=np.float64).reshape(-1, 3) @ R.T
        rn_mag = None if normals is None else np.abs(np.asarray(normals, dtype=np.float64).reshape(-1, 3)) @ np.abs(R).T
        for i in range(n):
            if drop[i]:
                continue
            c = (int(coord[i, 0]), int(coord[i, 1]), int(coord[i, 2]))
            v = self.index.get(c)
            if v is None:
                v = self.index[c] = len(self.voxels)
                self.voxels.append(Voxel(c, self.counter))
            vox = self.voxels[v]
            vox.lru = self.counter
            if self.kind == GAUSSIAN:
                if vox.finalized:  # gaussian_voxelmap.hpp:33-37
                    vox.finalized = False
                    vox.mean, vox.cov = vox.mean * vox.n, vox.cov * vox.n
                vox.n += 1
                vox.mean = vox.mean + x[i]
                vox.cov = vox.cov + rc[i]
                vox.mag_mean, vox.mag_cov = vox.mag_mean + mag[i], vox.mag_cov + rc_mag[i]
                kept[i] = True
                continue
            if len(vox.points) >= self.max_points:  # flat_container.hpp:44-49
                continue
            reject = False
            for j, y in enumerate(vox.points):
                d = y - x[i]
                d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if not (exact[i] and vox.exact[j] and _exact_distance(y, x[i], d2)):
                    err = 8.0 * EPS * (np.abs(mag[i]).max() + np.abs(vox.mags[j]).max())
                    if abs(d2 - self.min_sq) <= 16.0 * EPS * d2 + 2.0 * np.sqrt(d2) * err:
                        ambiguous[i] = True
                if d2 < self.min_sq:
                    reject = True
                    break
            if reject:
                continue
            vox.points.append(x[i])
            vox.mags.append(mag[i])
            vox.exact.append(bool(exact[i]))
            vox.source.append((self.inserts, i))
            vox.normals.append(None if rn is None else rn[i])
            vox.covs.append(None if rc is None else rc[i])
            vox.nmags.append(None if rn is None else rn_mag[i])
            vox.cmags.append(None if rc is None else rc_mag[i])
            vox.n = len(vox.points)
            kept[i] = True
        self.inserts += 1
        self.counter += 1  # incremental_voxelmap.hpp:74-86
        if self.counter % self.clear_cycle == 0:
            removed = np.array([v.lru + self.horizon < self.counter for v in self.voxels], dtype=bool)
            self.sweeps.append((self.counter, self.horizon, self.lru(), removed))
            self.voxels = [v for v, r in zip(self.voxels, removed) if not r]
            self.index = {v.coord: k for k, v in enumerate(self.voxels)}
        for v in self.voxels:  # :89-91
            if self.kind == GAUSSIAN and not v.finalized:
                v.finalized = True
                v.mean, v.cov = v.mean / v.n, v.cov / v.n
        return drop, kept, ambiguous

    # ---- what the map holds ---------------------------------------------------------------------------------------------------------------
    def size(self):
        return len(self.voxels)

    def coords(self):
        return np.array([v.coord for v in self.voxels], dtype=np.int64).reshape(-1, 3)

    def counts(self):
        return np.array([v.n for v in self.voxels], dtype=np.int64)

    def lru(self):
        return np.array([v.lru for v in self.voxels], dtype=np.int64)

    def means(self):
        """(means (V, 3), covs (V, 3, 3), slack of the means, slack of the covs): slack = (N + 16) 2^-52 sum |terms| / N"""
        V = len(self.voxels)
        m, c = np.array([v.mean for v in self.voxels]).reshape(V, 3), np.array([v.cov for v in self.voxels]).reshape(V, 3, 3)
        f = np.array([(v.n + 16) * 2.0 * EPS / v.n for v in self.voxels])
        sm = np.array([v.mag_mean for v in self.voxels]).reshape(V, 3) * f.reshape(V, 1)
        sc = np.array([v.mag_cov for v in self.voxels]).reshape(V, 3, 3) * f.reshape(V, 1, 1)
        return m, c, sm, sc

    def slots(self):
        """voxel 0's slots first, then voxel 1's, ...: points (P, 3), normals (P, 3) or None, covs (P, 3, 3) or None, the slack of each
        (17 * 2^-52 * sum |terms|: one term, N = 1), source (P, 2): insert and index of the point kept"""
        def rows(name, shape):
            a = [y for v in self.voxels for y in getattr(v, name)]
            return None if (a and a[0] is None) else np.array(a, dtype=np.float64).reshape((len(a),) + shape)
        f = 17 * 2.0 * EPS
        slack = lambda a: None if a is None else f * a
        return dict(points=rows("points", (3,)), normals=rows("normals", (3,)), covs=rows("covs", (3, 3)), slack_points=slack(rows("mags", (3,))),
                    slack_normals=slack(rows("nmags", (3,))), slack_covs=slack(rows("cmags", (3, 3))),
                    source=np.array([y for v in self.voxels for y in v.source], dtype=np.int64).reshape(-1, 2))


def _exact_distance(a, b, d2):
    al, bl = a.astype(np.longdouble), b.astype(np.longdouble)
    d = al - bl
    return np.longdouble(d2) == d[0] * d[0] + d[1] * d[1] + d[2] * d[2]


def one_shot(records, origin, covs, leaf):
    """the one-shot Gaussian map: a single insert at the identity into an empty map -> (map, dropped)"""
    m = Map(leaf, GAUSSIAN)
    drop, _, _ = m.insert(records, origin, None, None, covs)
    return m, drop


def ambiguous(steps, leaf, kind=GAUSSIAN, min_sq=0.01, max_points=10, lru=None):
    """steps: a list of (records, origin, T); lru: (horizon, clear_cycle) per step, a single pair or None -> one (n,) bool mask per step"""
    m = Map(leaf, kind, min_sq, max_points)
    out = []
    for k, (rec, org, T) in enumerate(steps):
        if lru is not None:
            m.set_lru(*(lru[k] if isinstance(lru, list) else lru))
        n = len(np.asarray(rec).reshape(-1, 3))
        covs = np.tile(np.eye(3), (n, 1, 1))
        out.append(m.insert(rec, org, T, None, covs)[2])
    return out

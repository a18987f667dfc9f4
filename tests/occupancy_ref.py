"""sga_occupancy_* (include/small_gicp_amd.h) restated in numpy float64.  No device and no project code.

The grid: origin g, leaf, dims (nx, ny, nz); inv_leaf = 1.0 / leaf; cell (x, y, z) at the linear index (z ny + y) nx + x holds a uint32
stamp (0: never observed; else 2 epoch + (1 if the cell was an endpoint in that scan)) and an fp32 log-odds L.

integrate(scan, T, min_range, max_range, mode): the epoch advances by one; e is the new value.  The scan is in the sensor frame (fp32
record r at the origin o_c); T = [R t] maps it into the world.
 1. s = r + o_c; rho = sqrt((sx^2 + sy^2) + sz^2); non-finite or rho < min_range: IGNORED; rho > max_range: TRUNCATED, p = s *
    (max_range / rho); else a HIT.
 2. q0 = t - g, q = (R o_c + t) - g; go = q0 * inv_leaf; a hit's ge = ((R r) + q) * inv_leaf, a truncated beam's ge = ((R p) + q0) *
    inv_leaf; R v per component (R[k][0] v0 + R[k][1] v1) + R[k][2] v2.  c = floor(go), ce = floor(ge).
 3. d = ge - go; per axis a: rem_a = |ce_a - c_a|; ce_a > c_a: tmax_a = ((c_a + 1) - go_a) / d_a, tdel_a = 1 / d_a; ce_a < c_a: tmax_a =
    (go_a - c_a) / (-d_a), tdel_a = 1 / (-d_a).  While rem_x + rem_y + rem_z > 0: the current cell is a free candidate; step the axis of
    least tmax among those with rem_a > 0 (ties: the lowest axis): tmax_a += tdel_a, rem_a -= 1.  A truncated beam also offers ce as a
    free candidate, a hit beam offers ce as the hit cell.  Cells outside dims are walked, not touched.
 4. Once per scan and cell, an endpoint wins: the hit cells H: L = min(fp32(L + l_hit), l_max), stamp 2 e + 1; the free candidates not
    in H: L = max(fp32(L + l_miss), l_min), stamp 2 e.  mode 1 skips the free phase.
 The box farther than max_range from the sensor, or an empty scan: the epoch advances, nothing else happens.

After go and ge every operation of the walk is a single IEEE operation, so the device can differ from this file only through the pose
product and rho (it may contract a product into the sum that follows) and through floor at a face.  A beam is IN THE BAND when a
component of go or ge lies within BAND of an integer, when rho lies within BAND of a range limit, or when at some step another eligible
axis b has (tmax_b - tmax_a) * |d_b| < BAND: the beam passes that close to a cell edge.  ties: the beams whose tmax were EQUAL at some
step (exact inputs: the lowest axis must win; they are band beams as well)."""
import numpy as np

BAND = 1e-9
F32 = np.float32
UNKNOWN, FREE, OCCUPIED = 0, 1, 2
MAX_STEPS = 3 * (4096 + 2)


def _rot(R, v):
    """R v per component, (R[k][0] v0 + R[k][1] v1) + R[k][2] v2, for the rows of v"""
    return np.stack([(R[k, 0] * v[:, 0] + R[k, 1] * v[:, 1]) + R[k, 2] * v[:, 2] for k in range(3)], axis=1)


def _near_integer(x):
    return np.abs(x - np.rint(x)) < BAND


class Grid:
    def __init__(self, origin, leaf, dims, l_hit=0.85, l_miss=-0.4, l_min=-2.0, l_max=3.5):
        self.g = np.asarray(origin, dtype=np.float64).reshape(3)
        self.leaf = float(leaf)
        self.inv_leaf = 1.0 / self.leaf
        self.dims = np.asarray(dims, dtype=np.int64).reshape(3)
        self.cells = int(self.dims.prod())
        self.l_hit, self.l_miss, self.l_min, self.l_max = F32(l_hit), F32(l_miss), F32(l_min), F32(l_max)
        self.clear()

    def clear(self):
        self.stamp = np.zeros(self.cells, np.uint32)
        self.L = np.zeros(self.cells, F32)
        self.epoch = 0

    # ---- frames ---------------------------------------------------------------------------------------------------------------------------
    def _pose(self, T, o_c):
        T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
        R, t = T[:3, :3], T[:3, 3]
        o_c = np.asarray(o_c, dtype=np.float64).reshape(3)
        ro = np.array([(R[k, 0] * o_c[0] + R[k, 1] * o_c[1]) + R[k, 2] * o_c[2] for k in range(3)])
        return R, (ro + t) - self.g, t - self.g

    def _inside(self, c):
        return ((c >= 0) & (c < self.dims)).all(axis=1)

    def _linear(self, c):
        return (c[:, 2] * self.dims[1] + c[:, 1]) * self.dims[0] + c[:, 0]

    def reachable(self, T, max_range):
        _, _, q0 = self._pose(T, (0.0, 0.0, 0.0))
        hi = self.dims.astype(np.float64) * self.leaf
        d = np.where(q0 < 0.0, -q0, np.where(q0 > hi, q0 - hi, 0.0))
        return bool((d * d).sum() <= max_range * max_range)

    # ---- integrate ------------------------------------------------------------------------------------------------------------------------
    def integrate(self, scan_rel, T=None, min_range=0.0, max_range=60.0, mode=0, o_c=(0.0, 0.0, 0.0)):
        """-> dict: beams, ignored, hits, truncated, cells_hit, cells_freed, band (the beams in the band), ties (the beams that met equal
        tmax), steps (cells walked, all beams), longest (the longest walk)"""
        assert np.isfinite(max_range) and max_range * self.inv_leaf <= 4096.0 and self.epoch < 2**31 - 1
        r = np.asarray(scan_rel, dtype=F32).astype(np.float64).reshape(-1, 3)
        n = len(r)
        self.epoch += 1
        e = self.epoch
        out = dict(beams=n, ignored=0, hits=0, truncated=0, cells_hit=0, cells_freed=0, band=0, ties=0, steps=0, longest=0)
        if n == 0 or not self.reachable(T, max_range):
            return out
        R, q, q0 = self._pose(T, o_c)
        go = q0 * self.inv_leaf
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            s = r + np.asarray(o_c, dtype=np.float64)
            fin = np.isfinite(s).all(axis=1)
            s0 = np.where(fin[:, None], s, 0.0)
            rho = np.sqrt((s0[:, 0] * s0[:, 0] + s0[:, 1] * s0[:, 1]) + s0[:, 2] * s0[:, 2])
            used = fin & np.isfinite(rho) & ~(rho < min_range)
            trunc = used & (rho > max_range)
            hit = used & ~trunc
            scale = max_range / np.where(trunc, rho, 1.0)
            p = s0 * scale[:, None]
            ge = np.where(trunc[:, None], _rot(R, p) + q0, _rot(R, np.where(fin[:, None], r, 0.0)) + q) * self.inv_leaf
            used &= np.isfinite(ge).all(axis=1)
            trunc &= used
            hit &= used
        band = np.zeros(n, bool)
        band |= used & (_near_integer(ge).any(axis=1) | (np.abs(rho - min_range) < BAND) | (np.abs(rho - max_range) < BAND))
        if _near_integer(go).any():
            band |= used
        out.update(ignored=int((~used).sum()), hits=int(hit.sum()), truncated=int(trunc.sum()))
        # ---- the walk, all beams at once
        idx = np.nonzero(used)[0]
        ge, tr = ge[idx], trunc[idx]
        m = len(idx)
        c = np.broadcast_to(np.floor(go).astype(np.int64), (m, 3)).copy()
        ce = np.floor(ge).astype(np.int64)
        d = ge - go
        rem = np.abs(ce - c)
        step = np.sign(ce - c)
        with np.errstate(invalid="ignore", divide="ignore"):
            tmax = np.where(step > 0, ((c + 1).astype(np.float64) - go) / d, np.where(step < 0, (go - c.astype(np.float64)) / (-d), np.inf))
            tdel = np.where(step > 0, 1.0 / d, np.where(step < 0, 1.0 / (-d), 0.0))
        total = rem.sum(axis=1)
        assert total.max(initial=0) <= MAX_STEPS
        out.update(steps=int(total.sum()), longest=int(total.max(initial=0)))
        free = []
        wband, ties = np.zeros(m, bool), np.zeros(m, bool)
        rows = np.arange(m)
        while True:
            act = rem.sum(axis=1) > 0
            if not act.any():
                break
            k = rows[act]
            ck = c[k]
            ins = self._inside(ck)
            free.append(self._linear(ck[ins]))
            elig = rem[k] > 0
            tm = np.where(elig, tmax[k], np.inf)
            a = np.argmin(tm, axis=1)  # the first of equal values: the lowest axis
            ta = tm[np.arange(len(k)), a]
            with np.errstate(invalid="ignore"):
                gap = (tm - ta[:, None]) * np.abs(d[k])
            other = elig.copy()
            other[np.arange(len(k)), a] = False
            wband[k] |= (other & (gap < BAND)).any(axis=1)
            ties[k] |= (other & (tm == ta[:, None])).any(axis=1)
            c[k, a] += step[k, a]
            tmax[k, a] += tdel[k, a]
            rem[k, a] -= 1
        assert np.array_equal(c, ce)  # the walk ends in ce
        band[idx] |= wband
        out.update(band=int(band.sum()), ties=int(ties.sum()))
        ins = self._inside(ce)
        free.append(self._linear(ce[tr & ins]))
        H = np.unique(self._linear(ce[~tr & ins]))
        self.L[H] = np.minimum((self.L[H] + self.l_hit).astype(F32), self.l_max)
        self.stamp[H] = 2 * e + 1
        out["cells_hit"] = len(H)
        if mode == 0:
            Fc = np.setdiff1d(np.unique(np.concatenate(free)) if free else np.zeros(0, np.int64), H)
            self.L[Fc] = np.maximum((self.L[Fc] + self.l_miss).astype(F32), self.l_min)
            self.stamp[Fc] = 2 * e
            out["cells_freed"] = len(Fc)
        return out

    # ---- queries --------------------------------------------------------------------------------------------------------------------------
    def cell_states(self, threshold=0.0):
        return np.where(self.stamp == 0, UNKNOWN, np.where(self.L.astype(np.float64) < threshold, FREE, OCCUPIED)).astype(np.uint8)

    def stats(self, threshold=0.0):
        st = self.cell_states(threshold)
        return dict(total=self.cells, unknown=int((st == 0).sum()), free=int((st == 1).sum()), occupied=int((st == 2).sum()), epoch=self.epoch)

    def classify(self, rel, T=None, threshold=0.0, o_c=(0.0, 0.0, 0.0)):
        """-> dict: state (n,) uint8, counts, band (the indices of the points within BAND of a face: the device may see the other cell)"""
        r = np.asarray(rel, dtype=F32).astype(np.float64).reshape(-1, 3)
        R, q, _ = self._pose(T, o_c)
        with np.errstate(invalid="ignore", over="ignore"):
            gc = (_rot(R, r) + q) * self.inv_leaf
            ins = (gc >= 0.0).all(axis=1) & (gc < self.dims.astype(np.float64)).all(axis=1)
            near = np.isfinite(gc).all(axis=1) & _near_integer(np.where(np.isfinite(gc), gc, 0.5)).any(axis=1)
        cell = np.where(ins[:, None], gc, 0.0).astype(np.int64)
        state = np.where(ins, self.cell_states(threshold)[self._linear(cell)], UNKNOWN).astype(np.uint8)
        counts = dict(total=len(r), unknown=int((state == 0).sum()), free=int((state == 1).sum()), occupied=int((state == 2).sum()), epoch=self.epoch)
        return dict(state=state, counts=counts, band=np.nonzero(near)[0])

    def export(self, threshold=0.0, which_mask=4):
        """-> (linear indices ascending (m,) int64, log-odds (m,) float32, centres' records (m, 3) float32 relative to the origin g)"""
        st = self.cell_states(threshold)
        idx = np.nonzero((which_mask >> st.astype(np.int64)) & 1)[0].astype(np.int64)
        plane = self.dims[0] * self.dims[1]
        z, rest = idx // plane, idx % plane
        y, x = rest // self.dims[0], rest % self.dims[0]
        centres = ((np.stack([x, y, z], axis=1).astype(np.float64) + 0.5) * self.leaf).astype(F32)
        return idx, self.L[idx].copy(), centres

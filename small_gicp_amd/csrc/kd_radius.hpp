// Fixed-radius walk of the implicit kd-tree: every record within `radius` of a query is handed to a functor.
// A state for kd_walk<STRIDE, S> (kd_search.hpp) whose prune bound never tightens, with its own kd_scan_leaf / kd_visit_group; the stack
// stays in LDS as kd_walk keeps it.  One lane per query.  Device code, gfx950.
//
// THE PREDICATE is in double: record j is a neighbour of the query q iff d2(q, j) = dx dx + dy dy + dz dz <= radius * radius, all of it
// formed in double from the fp32 record and the query's double coordinates in the tree's device frame (a query of another frame arrives
// as its record + the origin difference, added in double by the caller).  Every record of every leaf the walk opens is tested with it.
//
// THE PRUNING is the tree's own fp32 arithmetic (plane cuts, kd_box_dist2), from q32 = float(q), against a bound that is widened far
// enough that no plane or box test can exclude a record the predicate accepts:
//   * an accepted record c has |c - q| <= radius (1 + 2^-52), so |c - q32| <= r := radius + e with e = |q - q32| (formed in double; 0 when
//     the query is a record of the tree's frame);
//   * the true squared distance from q32 to a plane that separates it from c, or to a box that holds c, is at most |c - q32|^2 <= r^2;
//   * the fp32 value of such a lower bound is a chain of at most one subtraction, one product and two fused multiply-adds per term, each
//     rounded once: (1 + 2^-24)^5 < 1 + 6 * 2^-24 times the true value at most (an underflow only lowers it; kd_pack stores a cut rounded
//     toward zero, which lowers it again);
//   * the bound itself goes from double to float once more (1 + 2^-24) and is never below the smallest normal float, so that the
//     relative figures hold.
// open = float(r^2 (1 + 2^-20)) covers 16 * 2^-24 > (6 + 1 + 1) * 2^-24: the factor cloud_overlap.hip's walk uses.  A bound that
// overflows the float range becomes +inf and nothing is pruned.  Slots a leaf does not fill are masked by the leaf's point count, not
// by their distance (a radius beyond kKdFar would accept them).
// A query whose coordinates are not finite floats in the tree's frame has no neighbours.
#pragma once
#include <type_traits>

#include "kd_search.hpp"

namespace sga {

template <class F>
struct KdRadius {
  float open;         // sub-trees with a lower bound <= open are explored: fixed for the whole walk
  float dropped;      // kd_walk's note of what it discarded: not read here
  double qx, qy, qz;  // the query, the tree's device frame
  double r2;          // radius * radius
  F& f;               // f(cloud index of the record, d2) or f(index, d2, dx, dy, dz) — the record minus the query, the terms of d2 —: called
                      // once per record within the radius, in the walk's order
};

__device__ __forceinline__ float kd_radius_open(double radius, double e) {
  const double r = radius + e;
  return fmaxf(static_cast<float>(r * r * (1.0 + 0x1p-20)), 1.17549435e-38f);
}

// every record of the leaf, in slot order, against the predicate
template <class F>
__device__ __forceinline__ void kd_scan_leaf(const KdView& t, uint32_t leaf_node, float, float, float, KdRadius<F>& s) {
  const uint32_t k = leaf_node - (1u << t.depth);
  const uint32_t count = kd_bound(t.n, t.depth, k + 1) - kd_bound(t.n, t.depth, k);
  const float4* __restrict__ b = t.leafblk + 8ull * k;
  const float4 x0 = b[0], x1 = b[1], y0 = b[2], y1 = b[3], z0 = b[4], z1 = b[5], i0 = b[6], i1 = b[7];
  const float X[8] = {x0.x, x0.y, x0.z, x0.w, x1.x, x1.y, x1.z, x1.w};
  const float Y[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
  const float Z[8] = {z0.x, z0.y, z0.z, z0.w, z1.x, z1.y, z1.z, z1.w};
  const float I[8] = {i0.x, i0.y, i0.z, i0.w, i1.x, i1.y, i1.z, i1.w};
#pragma unroll
  for (int i = 0; i < kKdLeafMax; i++) {
    const double dx = static_cast<double>(X[i]) - s.qx, dy = static_cast<double>(Y[i]) - s.qy, dz = static_cast<double>(Z[i]) - s.qz;
    const double d2 = dx * dx + dy * dy + dz * dz;
    if (static_cast<uint32_t>(i) < count && d2 <= s.r2) {
      if constexpr (std::is_invocable_v<F&, uint32_t, double, double, double, double>)
        s.f(__float_as_uint(I[i]), d2, dx, dy, dz);
      else
        s.f(__float_as_uint(I[i]), d2);
    }
  }
}

// the leaves of a group whose box the widened ball reaches, in leaf order (nothing tightens: no nearest-first order, no early end)
template <class F>
__device__ __forceinline__ void kd_visit_group(const KdView& t, uint32_t gnode, float qx, float qy, float qz, KdRadius<F>& s) {
  const float4* __restrict__ h = t.groups + 8ull * (gnode - (1u << t.gdepth));
  const float4 lox = h[0], loy = h[1], loz = h[2], hix = h[3], hiy = h[4], hiz = h[5];
  const float lb0 = kd_box_dist2_vals(lox.x, loy.x, loz.x, hix.x, hiy.x, hiz.x, qx, qy, qz);
  const float lb1 = kd_box_dist2_vals(lox.y, loy.y, loz.y, hix.y, hiy.y, hiz.y, qx, qy, qz);
  const float lb2 = kd_box_dist2_vals(lox.z, loy.z, loz.z, hix.z, hiy.z, hiz.z, qx, qy, qz);
  const float lb3 = kd_box_dist2_vals(lox.w, loy.w, loz.w, hix.w, hiy.w, hiz.w, qx, qy, qz);
  const uint32_t leaf0 = gnode << t.glevels;
  const int leaves = 1 << t.glevels;  // (a header of a tree of depth < 2 has fewer than four leaves: their slots hold empty boxes)
  if (lb0 <= s.open) kd_scan_leaf(t, leaf0, qx, qy, qz, s);
  if (leaves > 1 && lb1 <= s.open) kd_scan_leaf(t, leaf0 + 1u, qx, qy, qz, s);
  if (leaves > 2 && lb2 <= s.open) kd_scan_leaf(t, leaf0 + 2u, qx, qy, qz, s);
  if (leaves > 2 && lb3 <= s.open) kd_scan_leaf(t, leaf0 + 3u, qx, qy, qz, s);
}

// The walk of one query (qx, qy, qz: double, the tree's device frame) from the root.  stack: LDS, kKdMaxDepth * STRIDE words; this lane
// uses stack[level * STRIDE + tid].  radius: finite and > 0.
template <int STRIDE, class F>
__device__ __forceinline__ void kd_radius_walk(const KdView& t, double qx, double qy, double qz, double radius, uint32_t* __restrict__ stack, int tid, F& f) {
  if (t.n == 0) return;
  const float fx = static_cast<float>(qx), fy = static_cast<float>(qy), fz = static_cast<float>(qz);
  if (!(fabsf(fx) <= 3.4028234e38f && fabsf(fy) <= 3.4028234e38f && fabsf(fz) <= 3.4028234e38f)) return;
  const double ex = qx - fx, ey = qy - fy, ez = qz - fz;
  KdRadius<F> s{kd_radius_open(radius, sqrt(ex * ex + ey * ey + ez * ez)), INFINITY, qx, qy, qz, radius * radius, f};
  kd_walk<STRIDE>(t, fx, fy, fz, s, 1u, 0, 0, stack, tid);
}

// One workgroup's exclusive prefix over term(0) .. term(n - 1) in index order (kRadScanThreads threads; sh: that many words of LDS):
// thread t owns the run [t * per, (t + 1) * per), per = ceil(n / threads); it adds its run, the runs' totals meet in a Hillis-Steele scan
// in LDS, and the thread learns what lies before its run.  The caller walks the run again to write what it needs.  Integers only.
constexpr int kRadScanThreads = 1024;
template <class Term>
__device__ __forceinline__ unsigned long long one_block_prefix(uint32_t n, uint32_t& first, uint32_t& end, unsigned long long* __restrict__ sh, unsigned long long& total, Term term) {
  const uint32_t t = threadIdx.x;
  const uint32_t per = (n + kRadScanThreads - 1u) / kRadScanThreads;
  first = min(static_cast<unsigned long long>(t) * per, static_cast<unsigned long long>(n));
  end = min(static_cast<unsigned long long>(first) + per, static_cast<unsigned long long>(n));
  unsigned long long own = 0ull;
  for (uint32_t i = first; i < end; i++) own += term(i);
  sh[t] = own;
  __syncthreads();
  for (uint32_t off = 1; off < kRadScanThreads; off <<= 1) {
    const unsigned long long add = t >= off ? sh[t - off] : 0ull;
    __syncthreads();
    sh[t] += add;
    __syncthreads();
  }
  const unsigned long long before = sh[t] - own;
  total = sh[kRadScanThreads - 1];
  __syncthreads();
  return before;
}

}  // namespace sga

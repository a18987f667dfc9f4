// Equirectangular projective search (ann/projective_search.hpp) on the device: the projection, the pixel rule and the windowed scan that
// the index build (projective.hip), the standalone kNN (projective.hip) and the factor kernel (linearize.hip, TARGET == 3) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

namespace sga {

// What a kernel needs of a projective index.  img: u-major (pixel u * H + v), entry = target index + 1, 0 = none.  org: the device frame
// of the target's fp32 records (common.hpp: device frames); the projection is not translation invariant, so it adds org back in double.
struct ProjView {
  const uint32_t* __restrict__ img;
  int W, H;
  int wh, wv;              // search_window_h / search_window_v (projective_search.hpp:153-154)
  int repeat_h, repeat_v;  // 1: BorderRepeat (:36-39), 0: BorderClamp (:30-33)
  double org[3];
};

// a product the compiler may not fuse into the add that consumes it (the library builds with -ffp-contract=fast, which disregards
// `#pragma clang fp contract`): sums of squares in a fixed order, rounded after every operation, as tests/projective_ref.py restates them
template <typename T>
__device__ __forceinline__ T proj_sq(T x) {
  T p = x * x;
  asm volatile("" : "+v"(p));
  return p;
}

// EquirectangularProjection (projective_search.hpp:13-27) and the pixel of UnsafeProjectiveSearch (:56-58, :109-111), in double on the point
// in the caller's frame; |p|^2 = (x^2 + y^2) + z^2, each operation rounded.
// Returns false for a non-finite point or projection (undefined behaviour in the reference; here: not projected).  The pixel may lie out of the image
// (u == W for lon == pi): the callers decide.
__device__ __forceinline__ bool proj_pixel(double x, double y, double z, int W, int H, int& u, int& v) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
  const double n2 = (proj_sq(x) + proj_sq(y)) + proj_sq(z);
  double pu = 0.5, pv = 0.5;
  if (!(n2 < 1e-3)) {
    const double nrm = sqrt(n2);
    const double lat = -asin(y / nrm);
    const double lon = atan2(x / nrm, z / nrm);
    pu = lon / (2.0 * M_PI) + 0.5;
    pv = lat / M_PI + 0.5;
    if (!(isfinite(pu) && isfinite(pv))) return false;  // |y| / |p| rounded past 1: asin is NaN, whose int conversion the reference leaves undefined
  }
  u = static_cast<int>(pu * static_cast<double>(W));  // truncation toward zero, as the reference's int conversion
  v = static_cast<int>(pv * static_cast<double>(H));
  return true;
}

// a device-frame coordinate back in the caller's frame; origin 0 leaves it as it is (x + 0.0 would turn a -0.0 into +0.0, and atan2 tells them apart)
__device__ __forceinline__ double proj_add(double x, double o) { return o == 0.0 ? x : x + o; }

// BorderRepeat wraps ONCE (:36-39); BorderClamp leaves the value as it is (:30-33).  Out-of-range afterwards: skipped by the caller.
__device__ __forceinline__ int proj_border(int x, int width, int repeat) { return repeat ? (x < 0 ? x + width : (x >= width ? x - width : x)) : x; }

// squared distance of a stored fp32 record to the query in the pair arithmetic, (pt - query).squaredNorm() as (dx^2 + dy^2) + dz^2
template <typename Real>
__device__ __forceinline__ Real proj_dist2(const float4& t, Real qx, Real qy, Real qz) {
  const Real dx = static_cast<Real>(t.x) - qx, dy = static_cast<Real>(t.y) - qy, dz = static_cast<Real>(t.z) - qz;
  return (proj_sq(dx) + proj_sq(dy)) + proj_sq(dz);
}

// The nearest neighbour of UnsafeProjectiveSearch::knn_search<1> (:107-140 with KnnResult<1>::push, knn_result.hpp:80-100): du outer over
// -wh..wh, dv inner over -wv..wv, a candidate replaces the best only if strictly nearer (first in scan order wins a tie); the distances are
// in Real (fp64: double, the reference's; fp32: float).  (qx, qy, qz): the query in the target's device frame.  Returns the target index
// (original order) or -1; d2 = its squared distance.
template <typename Real>
__device__ __forceinline__ int projective_nearest(const ProjView& pv, const float4* __restrict__ pts, Real qx, Real qy, Real qz, Real& d2) {
  int best = -1;
  Real best_d = FLT_MAX;
  if constexpr (sizeof(Real) == 8) best_d = DBL_MAX;  // KnnResult's initial worst distance (knn_result.hpp:60)
  d2 = best_d;
  int u, v;
  if (!proj_pixel(proj_add(qx, pv.org[0]), proj_add(qy, pv.org[1]), proj_add(qz, pv.org[2]), pv.W, pv.H, u, v)) return -1;
  for (int du = -pv.wh; du <= pv.wh; du++) {
    const int uc = proj_border(u + du, pv.W, pv.repeat_h);
    if (uc < 0 || uc >= pv.W) continue;
    const uint32_t* __restrict__ col = pv.img + static_cast<size_t>(uc) * pv.H;  // one contiguous run per window column
    for (int dv = -pv.wv; dv <= pv.wv; dv++) {
      const int vc = proj_border(v + dv, pv.H, pv.repeat_v);
      if (vc < 0 || vc >= pv.H) continue;
      const uint32_t e = col[vc];
      if (e == 0u) continue;
      const Real d = proj_dist2<Real>(pts[e - 1u], qx, qy, qz);
      if (d < best_d) {
        best_d = d;
        best = static_cast<int>(e - 1u);
      }
    }
  }
  d2 = best_d;
  return best;
}

// k nearest neighbours (KnnResult<-1>, knn_result.hpp:80-100) into idx[0, k) / dist[0, k), which the caller has set to -1 / the initial
// worst distance: a candidate enters only if strictly nearer than the current worst and is inserted behind the entries it does not beat.
// A column that the single wrap visits twice (W < 2 wh + 1) pushes its points twice: duplicates are kept, as in the reference.
template <typename Real, typename Idx>
__device__ __forceinline__ int projective_knn(const ProjView& pv, const float4* __restrict__ pts, Real qx, Real qy, Real qz, int k, Idx* __restrict__ idx, Real* __restrict__ dist) {
  int found = 0;
  int u, v;
  if (!proj_pixel(proj_add(qx, pv.org[0]), proj_add(qy, pv.org[1]), proj_add(qz, pv.org[2]), pv.W, pv.H, u, v)) return 0;
  for (int du = -pv.wh; du <= pv.wh; du++) {
    const int uc = proj_border(u + du, pv.W, pv.repeat_h);
    if (uc < 0 || uc >= pv.W) continue;
    const uint32_t* __restrict__ col = pv.img + static_cast<size_t>(uc) * pv.H;
    for (int dv = -pv.wv; dv <= pv.wv; dv++) {
      const int vc = proj_border(v + dv, pv.H, pv.repeat_v);
      if (vc < 0 || vc >= pv.H) continue;
      const uint32_t e = col[vc];
      if (e == 0u) continue;
      const Real d = proj_dist2<Real>(pts[e - 1u], qx, qy, qz);
      if (!(d < dist[k - 1])) continue;
      int loc = found < k - 1 ? found : k - 1;
      for (; loc > 0 && d < dist[loc - 1]; loc--) {
        idx[loc] = idx[loc - 1];
        dist[loc] = dist[loc - 1];
      }
      idx[loc] = static_cast<Idx>(e - 1u);
      dist[loc] = d;
      found = found + 1 < k ? found + 1 : k;
    }
  }
  return found;
}

}  // namespace sga

// What the hypothesis kernel (ransac.hip), the host solver (rigid_fit.hip) and their debug entry points share.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace sga {

// The counter-based generator of sga_ransac_correspondences (small_gicp_amd.h states it; any restatement repeats it exactly)
__host__ __device__ inline uint64_t ransac_mix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t ransac_idx(uint64_t u, uint64_t R) { return ((u >> 32) * R) >> 32; }
// the three distinct pair numbers of hypothesis h among M >= 3 pairs (M < 2^32)
__host__ __device__ inline void ransac_draw(uint64_t seed, uint64_t h, uint64_t M, uint64_t out[3]) {
  const uint64_t u0 = ransac_mix64(seed ^ ransac_mix64(4ull * h + 0ull)), u1 = ransac_mix64(seed ^ ransac_mix64(4ull * h + 1ull)), u2 = ransac_mix64(seed ^ ransac_mix64(4ull * h + 2ull));
  const uint64_t i0 = ransac_idx(u0, M);
  uint64_t i1 = ransac_idx(u1, M - 1);
  if (i1 >= i0) i1++;
  const uint64_t lo = i0 < i1 ? i0 : i1, hi = i0 < i1 ? i1 : i0;
  uint64_t i2 = ransac_idx(u2, M - 2);
  if (i2 >= lo) i2++;
  if (i2 >= hi) i2++;
  out[0] = i0;
  out[1] = i1;
  out[2] = i2;
}

// rigid_fit.hip: the least-squares rigid motion of n point pairs from their plain sums (Horn's quaternion form over a Jacobi eigen-solver).
// T column-major 4x4.  false, T untouched: n < 3, or the centred cross-covariance has rank < 2.
bool rigid_from_sums(uint64_t n, const double sum_s[3], const double sum_t[3], const double cross[9], double T[16]);
// rigid_fit.hip: the same Jacobi solver on a symmetric 3x3 matrix S = {xx, xy, xz, yy, yz, zz}: the eigenvalues in ascending order and
// their unit eigenvectors, vectors[k] belonging to values[k].  The refit of sga_cloud_segment_plane (cloud_plane.hip).
void sym3_eigen(const double S[6], double values[3], double vectors[3][3]);

}  // namespace sga

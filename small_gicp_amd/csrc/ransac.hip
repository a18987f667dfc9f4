// RANSAC over correspondences on the device: sga_ransac_correspondences — the points of the M pairs gathered
// once in double, one lane per hypothesis (a counter-based draw, the edge and degeneracy tests, the pose from the two triangle frames),
// the poses that pass scored over all pairs by their whole workgroup, the best by ONE 64-bit integer atomic max, and the sums of the refit over the best
// hypothesis' inliers by one workgroup in a fixed order.  The host solves the rotation (rigid_fit.hip) after the call's one wait.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "ransac.hpp"

#include <cmath>

namespace sga {
namespace {

constexpr int kRsBlock = 256;       // hypotheses of a workgroup, and the threads that score a pose
constexpr int kRsSums = 17;         // count, sum x (3), sum y (3), sum x y^T (9), sum of squared residuals
constexpr int kRsSlotDoubles = 40;  // best word, scored, the sums, a_s, a_t, R (row-major), t

struct RansacArgs {
  const double* P;  // 6 x M: source x y z, target x y z of every pair (record + origin)
  uint32_t M;
  uint64_t H, seed;
  double max2, edge_similarity, min_edge;
  unsigned long long* status;  // [0] the best word (score << 32 | 0xFFFFFFFF - h), [1] hypotheses scored
};

struct Vec3 {
  double x, y, z;
};
__device__ __forceinline__ Vec3 operator-(const Vec3 a, const Vec3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ Vec3 cross3(const Vec3 a, const Vec3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double norm3(const Vec3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
__device__ __forceinline__ Vec3 pair_point(const RansacArgs& a, uint64_t q, int side) { return {a.P[(3 * side + 0) * static_cast<size_t>(a.M) + q], a.P[(3 * side + 1) * static_cast<size_t>(a.M) + q], a.P[(3 * side + 2) * static_cast<size_t>(a.M) + q]}; }

struct Pose {
  double R[9], t[3];  // row-major
};

// frame of a triangle: rows e1, e2, e3; false when it is degenerate
__device__ __forceinline__ bool triangle_frame(const Vec3 a, const Vec3 b, const Vec3 c, double F[9]) {
  const Vec3 ab = b - a, ac = c - a;
  const double lab = norm3(ab);
  if (!(lab > 0.0)) return false;
  const Vec3 e1{ab.x / lab, ab.y / lab, ab.z / lab};
  const Vec3 n = cross3(e1, ac);
  const double ln = norm3(n);
  if (!(ln > 0.0) || ln < 1e-9 * norm3(ac)) return false;
  const Vec3 e3{n.x / ln, n.y / ln, n.z / ln};
  const Vec3 e2 = cross3(e3, e1);
  F[0] = e1.x, F[1] = e1.y, F[2] = e1.z, F[3] = e2.x, F[4] = e2.y, F[5] = e2.z, F[6] = e3.x, F[7] = e3.y, F[8] = e3.z;
  return true;
}

// the pose of hypothesis h, or false when it is dropped by the edge test or for a degenerate triangle
__device__ __forceinline__ bool hypothesis_pose(const RansacArgs& a, uint64_t h, Pose& T, Vec3* first_s = nullptr, Vec3* first_t = nullptr) {
  uint64_t id[3];
  ransac_draw(a.seed, h, a.M, id);
  Vec3 s[3], t[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    s[k] = pair_point(a, id[k], 0);
    t[k] = pair_point(a, id[k], 1);
  }
  if (first_s != nullptr) *first_s = s[0], *first_t = t[0];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double ls = norm3(s[(k + 1) % 3] - s[k]), lt = norm3(t[(k + 1) % 3] - t[k]);
    const double lo = fmin(ls, lt), hi = fmax(ls, lt);
    if (!(lo >= a.edge_similarity * hi) || !(lo >= a.min_edge)) return false;
  }
  double Fs[9], Ft[9];
  if (!triangle_frame(s[0], s[1], s[2], Fs) || !triangle_frame(t[0], t[1], t[2], Ft)) return false;
  // R = F_t F_s^T with the frames' vectors as columns: R[r][c] = sum_k e_k^t[r] e_k^s[c]
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) T.R[3 * r + c] = (Ft[r] * Fs[c] + Ft[3 + r] * Fs[3 + c]) + Ft[6 + r] * Fs[6 + c];
  const Vec3 cs{((s[0].x + s[1].x) + s[2].x) / 3.0, ((s[0].y + s[1].y) + s[2].y) / 3.0, ((s[0].z + s[1].z) + s[2].z) / 3.0};
  const Vec3 ct{((t[0].x + t[1].x) + t[2].x) / 3.0, ((t[0].y + t[1].y) + t[2].y) / 3.0, ((t[0].z + t[1].z) + t[2].z) / 3.0};
  T.t[0] = ct.x - ((T.R[0] * cs.x + T.R[1] * cs.y) + T.R[2] * cs.z);
  T.t[1] = ct.y - ((T.R[3] * cs.x + T.R[4] * cs.y) + T.R[5] * cs.z);
  T.t[2] = ct.z - ((T.R[6] * cs.x + T.R[7] * cs.y) + T.R[8] * cs.z);
  return true;
}

__device__ __forceinline__ double residual2(const Pose& T, const double sx, const double sy, const double sz, const double tx, const double ty, const double tz) {
  const double rx = (((T.R[0] * sx + T.R[1] * sy) + T.R[2] * sz) + T.t[0]) - tx;
  const double ry = (((T.R[3] * sx + T.R[4] * sy) + T.R[5] * sz) + T.t[1]) - ty;
  const double rz = (((T.R[6] * sx + T.R[7] * sy) + T.R[8] * sz) + T.t[2]) - tz;
  return (rx * rx + ry * ry) + rz * rz;
}

}  // namespace

// The points of the pairs, record + origin in double: pairs = 2 M indices in a slot of the staging ring (checked on the host)
__global__ __launch_bounds__(256) void ransac_points_kernel(const uint32_t* __restrict__ pairs, uint32_t M, const float4* __restrict__ src, const float4* __restrict__ tgt, double osx, double osy, double osz, double otx, double oty, double otz,
                                                            double* __restrict__ P) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= M) return;
  const float4 s = src[pairs[2 * q]], t = tgt[pairs[2 * q + 1]];
  const size_t m = M;
  P[0 * m + q] = static_cast<double>(s.x) + osx;
  P[1 * m + q] = static_cast<double>(s.y) + osy;
  P[2 * m + q] = static_cast<double>(s.z) + osz;
  P[3 * m + q] = static_cast<double>(t.x) + otx;
  P[4 * m + q] = static_cast<double>(t.y) + oty;
  P[5 * m + q] = static_cast<double>(t.z) + otz;
}

// One lane per hypothesis for the draw, the tests and the pose; the poses that pass are then scored by the WHOLE workgroup, one after the
// other: thread t takes the pairs t, t + 256, ... (coalesced loads of the gathered points), the counts of the waves meet in an integer
// atomic in LDS.  With the edge test on, a few hypotheses in a hundred reach this point: their scores cost a dozen steps of every
// thread instead of M steps of a few.  A pose's slot in LDS depends on arrival, its score and its key do not; the keys meet in one
// integer atomic max, the workgroup's number of poses in one integer atomic add: no arrival order enters the result.
__global__ __launch_bounds__(kRsBlock) void ransac_hypotheses_kernel(const RansacArgs a) {
  __shared__ Pose poses[kRsBlock];
  __shared__ unsigned long long hyp[kRsBlock];
  __shared__ unsigned score[kRsBlock];
  __shared__ unsigned count;
  const int tid = threadIdx.x;
  const uint64_t h = static_cast<uint64_t>(blockIdx.x) * kRsBlock + tid;
  if (tid == 0) count = 0u;
  score[tid] = 0u;
  __syncthreads();
  Pose T;
  if (h < a.H && hypothesis_pose(a, h, T)) {
    const unsigned slot = atomicAdd(&count, 1u);
    poses[slot] = T;
    hyp[slot] = h;
  }
  __syncthreads();
  const unsigned n = count;  // (uniform over the workgroup)
  if (n == 0u) return;
  for (unsigned s = 0; s < n; s++) {
    const Pose& P = poses[s];
    unsigned mine = 0u;
    for (uint32_t q = tid; q < a.M; q += kRsBlock) {
      const size_t m = a.M;
      mine += residual2(P, a.P[q], a.P[m + q], a.P[2 * m + q], a.P[3 * m + q], a.P[4 * m + q], a.P[5 * m + q]) <= a.max2 ? 1u : 0u;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
    if ((tid & 63) == 0 && mine != 0u) atomicAdd(&score[s], mine);
  }
  __syncthreads();
  unsigned long long key = static_cast<unsigned>(tid) < n ? (static_cast<unsigned long long>(score[tid]) << 32) | (0xFFFFFFFFull - hyp[tid]) : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if ((tid & 63) == 0 && key != 0ull) atomicMax(&a.status[0], key);
  if (tid == 0) atomicAdd(&a.status[1], static_cast<unsigned long long>(n));
}

// The best hypothesis' pose formed again from its triple, and over its inliers — x = p_s - a_s, y = p_t - a_t, a the first point of the
// triple: sums of small numbers wherever the clouds lie — the count, sum x, sum y, sum x y^T and the sum of squared residuals, in
// double by ONE workgroup: thread t adds the pairs t, t + 256, ... in order, the threads' partials meet in a fixed tree in LDS.
// out (a slot of the staging ring): the best word, the number scored, the 17 sums, a_s, a_t, R (row-major), t.
__global__ __launch_bounds__(kRsBlock) void ransac_refit_kernel(const RansacArgs a, double* __restrict__ out) {
  __shared__ double sh[kRsSums][kRsBlock];
  const int tid = threadIdx.x;
  const unsigned long long best = a.status[0];
  if (best == 0ull) {  // nothing scored (uniform)
    if (tid == 0) {
      reinterpret_cast<unsigned long long*>(out)[0] = 0ull;
      reinterpret_cast<unsigned long long*>(out)[1] = a.status[1];
      __threadfence_system();
    }
    return;
  }
  const uint64_t h = 0xFFFFFFFFull - (best & 0xFFFFFFFFull);
  Pose T;
  Vec3 as, at;
  (void)hypothesis_pose(a, h, T, &as, &at);
  double acc[kRsSums];
#pragma unroll
  for (int c = 0; c < kRsSums; c++) acc[c] = 0.0;
  for (uint32_t q = tid; q < a.M; q += kRsBlock) {
    const Vec3 s = pair_point(a, q, 0), t = pair_point(a, q, 1);
    const double r2 = residual2(T, s.x, s.y, s.z, t.x, t.y, t.z);
    if (!(r2 <= a.max2)) continue;
    const double x[3] = {s.x - as.x, s.y - as.y, s.z - as.z}, y[3] = {t.x - at.x, t.y - at.y, t.z - at.z};
    acc[0] += 1.0;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      acc[1 + r] += x[r];
      acc[4 + r] += y[r];
#pragma unroll
      for (int c = 0; c < 3; c++) acc[7 + 3 * r + c] += x[r] * y[c];
    }
    acc[16] += r2;
  }
#pragma unroll
  for (int c = 0; c < kRsSums; c++) sh[c][tid] = acc[c];
  __syncthreads();
  for (int off = kRsBlock / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int c = 0; c < kRsSums; c++) sh[c][tid] += sh[c][tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  reinterpret_cast<unsigned long long*>(out)[0] = best;
  reinterpret_cast<unsigned long long*>(out)[1] = a.status[1];
  for (int c = 0; c < kRsSums; c++) out[2 + c] = sh[c][0];
  out[19] = as.x, out[20] = as.y, out[21] = as.z;
  out[22] = at.x, out[23] = at.y, out[24] = at.z;
  for (int c = 0; c < 9; c++) out[25 + c] = T.R[c];
  for (int c = 0; c < 3; c++) out[34 + c] = T.t[c];
  __threadfence_system();
}

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

int ransac_check(const sga_ransac& p, size_t M) {
  if (!(is_finite(p.max_distance) && p.max_distance > 0.0)) return fail(SGA_ERR_INVALID, "ransac: max_distance must be finite and > 0");
  if (p.iterations < 1 || p.iterations >= (1ull << 32)) return fail(SGA_ERR_INVALID, "ransac: iterations must be in [1, 2^32)");
  if (!(p.edge_similarity >= 0.0 && p.edge_similarity <= 1.0)) return fail(SGA_ERR_INVALID, "ransac: edge_similarity must be in [0,1]");
  if (!(is_finite(p.min_edge) && p.min_edge >= 0.0)) return fail(SGA_ERR_INVALID, "ransac: min_edge must be finite and >= 0");
  if (M >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many pairs (%zu; limit 2^31-1)", M);
  return SGA_OK;
}

void set_identity(double T[16]) {
  for (int k = 0; k < 16; k++) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_ransac_default(sga_ransac* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_distance = 1.0;
  p->iterations = 20000;
  p->edge_similarity = 0.9;
}

int sga_ransac_correspondences(sga_context* ctx, const sga_cloud* source, const sga_cloud* target, const int64_t* pairs, size_t M, const sga_ransac* params, double T[16], sga_ransac_result* result) {
  if (!ctx || !source || !target || !params || !T || !result || (M > 0 && !pairs)) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(ransac_check(*params, M));
  // ---- (from here on the handles are read)
  if (source->device != ctx->device || target->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  for (size_t q = 0; q < M; q++) {
    if (pairs[2 * q] < 0 || static_cast<unsigned long long>(pairs[2 * q]) >= source->n)
      return fail(SGA_ERR_INVALID, "pairs[%zu] names source point %lld, outside a cloud of %zu points", q, static_cast<long long>(pairs[2 * q]), source->n);
    if (pairs[2 * q + 1] < 0 || static_cast<unsigned long long>(pairs[2 * q + 1]) >= target->n)
      return fail(SGA_ERR_INVALID, "pairs[%zu] names target point %lld, outside a cloud of %zu points", q, static_cast<long long>(pairs[2 * q + 1]), target->n);
  }
  std::memset(result, 0, sizeof(*result));
  set_identity(T);
  if (M < 3) return SGA_OK;  // no triple: nothing is launched
  if (source->n >= (1ull << 32) || target->n >= (1ull << 32)) return fail(SGA_ERR_INVALID, "too many points");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, source->ready));
  SGA_TRY(wait_ready(ctx, target->ready));
  DevBuf<double> P;  // both live to the end of the call (then: the stream's free list)
  DevBuf<unsigned long long> status;
  SGA_TRY(P.alloc(6 * M));
  SGA_TRY(status.alloc(2));
  sga_context::StageSlot* in = nullptr;
  SGA_TRY(stage_acquire(ctx, 2 * M * sizeof(uint32_t), &in));
  uint32_t* idx = static_cast<uint32_t*>(in->host);
  for (size_t q = 0; q < 2 * M; q++) idx[q] = static_cast<uint32_t>(pairs[q]);
  count_launch(Chain::Ransac);
  hipLaunchKernelGGL(ransac_points_kernel, dim3(static_cast<unsigned>((M + 255) / 256)), dim3(256), 0, ctx->stream, static_cast<const uint32_t*>(in->dev), static_cast<uint32_t>(M), source->pts.p, target->pts.p, source->origin[0],
                     source->origin[1], source->origin[2], target->origin[0], target->origin[1], target->origin[2], P.p);
  SGA_HIP(hipGetLastError());
  SGA_TRY(stage_release(ctx, in));
  count_launch(Chain::Ransac);
  SGA_HIP(hipMemsetAsync(status.p, 0, 2 * sizeof(unsigned long long), ctx->stream));
  RansacArgs a;
  a.P = P.p;
  a.M = static_cast<uint32_t>(M);
  a.H = params->iterations;
  a.seed = params->seed;
  a.max2 = params->max_distance * params->max_distance;
  a.edge_similarity = params->edge_similarity;
  a.min_edge = params->min_edge;
  a.status = status.p;
  count_launch(Chain::Ransac);
  hipLaunchKernelGGL(ransac_hypotheses_kernel, dim3(static_cast<unsigned>((a.H + kRsBlock - 1) / kRsBlock)), dim3(kRsBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, kRsSlotDoubles * sizeof(double), &slot));
  count_launch(Chain::Ransac);
  hipLaunchKernelGGL(ransac_refit_kernel, dim3(1), dim3(kRsBlock), 0, ctx->stream, a, static_cast<double*>(slot->dev));
  SGA_HIP(hipGetLastError());
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait: the sums are in the slot
  const double* o = static_cast<const double*>(slot->host);
  const unsigned long long best = reinterpret_cast<const unsigned long long*>(o)[0];
  result->scored = reinterpret_cast<const unsigned long long*>(o)[1];
  if (best == 0ull) return SGA_OK;  // no hypothesis passed the tests: inliers 0, the identity
  result->best_hypothesis = 0xFFFFFFFFull - (best & 0xFFFFFFFFull);
  result->inliers = best >> 32;
  const double* sums = o + 2;
  result->inlier_rmse = result->inliers > 0 ? std::sqrt(sums[16] / static_cast<double>(result->inliers)) : 0.0;
  const double *as = o + 19, *at = o + 22, *R = o + 25, *t = o + 34;
  double Rf[9], tf[3];
  for (int k = 0; k < 9; k++) Rf[k] = R[k];
  for (int k = 0; k < 3; k++) tf[k] = t[k];
  double L[16];
  if (rigid_from_sums(result->inliers, sums + 1, sums + 4, sums + 7, L)) {  // y = R' x + t' about (a_s, a_t) -> p_t = R' p_s + (a_t + t' - R' a_s)
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) Rf[3 * r + c] = L[4 * c + r];
    for (int r = 0; r < 3; r++) tf[r] = (at[r] + L[12 + r]) - ((Rf[3 * r] * as[0] + Rf[3 * r + 1] * as[1]) + Rf[3 * r + 2] * as[2]);
    result->refit = 1;
  }
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * c + r] = Rf[3 * r + c];
    T[12 + r] = tf[r];
  }
  return SGA_OK;
}

int sga_debug_ransac_launches(unsigned long long* launches) { return report_launches(Chain::Ransac, launches); }

int sga_debug_ransac_draw(uint64_t seed, uint64_t h, uint64_t M, uint64_t out[3]) {
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  if (M < 3 || M >= (1ull << 31)) return fail(SGA_ERR_INVALID, "ransac draw: M must be in [3, 2^31)");
  ransac_draw(seed, h, M, out);
  return SGA_OK;
}

int sga_debug_rigid_from_sums(uint64_t n, const double sum_s[3], const double sum_t[3], const double cross[9], double T[16]) {
  if (!sum_s || !sum_t || !cross || !T) return 0;
  return rigid_from_sums(n, sum_s, sum_t, cross, T) ? 1 : 0;
}

}  // extern "C"

// Sweep registration on the device: the pose T (target <- sensor at ref_time) and the twist xi (the sensor's
// motion per unit of time) of a RAW sweep estimated together.  Source point i, with the time s_i, has a pose of its own:
//     a_i = double(s_i) - ref_time,  E_i = exp(a_i xi) (lie.hpp: twist_pose),  p'_i = E_i p_i,  q_i = T p'_i,
// its pair is the exact nearest target record of q_i (cloud_overlap.hip's walk), and the factors are those of the lone registration with
// p'_i in the place of the source point:  r = t_j - q_i,  J_T = [R_T skew(p'_i) | -R_T],  J_xi = J_T a_i J_l(a_i xi),  J = [J_T | J_xi],
//     H += J^T M J (12 x 12),  b += J^T M r,  e += r^T M r / 2,
// M = (C^t_j + (R_T R_Ei) C_i (R_T R_Ei)^T)^-1 (GICP), diag(n_j^2) (PLANE_ICP) or I (ICP).  Everything is double from the fp32 records.
// A linearization is TWO launches and one host wait: sweep_pass_kernel (one lane per point, a row of partial sums per workgroup) and
// sweep_sum_kernel (one workgroup adds the rows in an order that depends on nothing but n).  No floating-point atomics, no spin.
// The error pass is the same two steps over the stored pairs (and the stored M) at another state.
#include <cmath>

#include "cloud_ops.hpp"
#include "forest.hpp"
#include "kd_search.hpp"
#include "lie.hpp"
#include "voxel_steps.hpp"

namespace sga {
namespace {

constexpr int kSwBlock = 256;  // points of a workgroup: one lane each, four waves
constexpr int kSwWaves = kSwBlock / 64;
// a row of sums: [0, 78) the upper triangle of H row-wise, [78, 90) b, 90 e, 91 the inliers
constexpr int kSwCols = 92, kSwColB = 78, kSwColE = 90, kSwColN = 91;
constexpr int kSwStride = 96;  // doubles between two rows of partials
constexpr int kSwSumThreads = 1024, kSwSumGroups = 8, kSwSumCols = kSwSumThreads / kSwSumGroups;
static_assert(kSwCols <= kSwSumCols && kSwCols <= kSwStride && kSwCols <= kSwBlock, "a thread per column");
// J_l(x) = sum_k ad(x)^k / (k + 1)!, x = a xi, summed until the bound rho^k / (k + 1)! of a term (rho = |a| (|omega| + |v|) >=
// |ad(x)|_2) is below 1e-17 AND k + 2 > 2 rho: the terms left out then sum to less than that bound, relative to |J_T|.  A call is
// refused when rho exceeds kSwRhoMax for a finite time of the sweep, so the loop ends within kSwSeriesMax terms (8^48 / 49! < 4e-20).
constexpr double kSwRhoMax = 8.0;
constexpr int kSwSeriesMax = 56;

// What a pass receives (kernel arguments: read with scalar loads)
struct SweepArgs {
  const float4* pts;   // the source's records, the caller's order
  const Cov8* cov;     // ... its covariances (GICP), or null
  const float* times;  // n times, in a slot of the staging ring by its device address
  Pose12 T;            // the source's device frame -> the target's: R_T, (R_T o_s + t_T) - o_t
  double os[3];        // the source's origin: p'_i = record + os
  TwistConst c;        // xi, for records of the frame at os (lie.hpp)
  double xi[6];
  double rho_unit;     // |omega| + |v|
  double ref_time;
  double max_dist_sq;  // < 0: no rejector
  KdView g;            // the target
  const float4* tnrm;  // ... its normals (PLANE_ICP) and covariances (GICP), kd order
  const Cov8* tcov;
  int* j;              // n: the winner's kd position or -1 (written by a linearization, read by an error pass)
  double* m;           // GICP: 6 n, entry-major
  double* partials;    // a row per workgroup: kSwStride apart (a linearization), 1 apart (an error pass)
  long long* nearest_host;  // the winners' ORIGINAL indices into the staging ring, or null
  uint32_t n, tn;
  int factor;
};

__device__ __forceinline__ bool sw_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

__device__ __forceinline__ void sw_cross(const double a[3], const double b[3], double out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace

// ERR = false: the pose of every point, the walk, the pair, the 92 sums; the pair (and GICP's M) stored.
// ERR = true:  the error of the stored pairs at this state, one sum.
// Lanes without a point, or without a pair, add zeros: every lane takes part in the reduction — a butterfly inside the wave (the same
// bits in every lane), the four waves' totals through LDS in a fixed order, one row per workgroup.
template <bool ERR>
__global__ __launch_bounds__(kSwBlock) void sweep_pass_kernel(const SweepArgs a) {
  extern __shared__ uint32_t sw_stack[];  // [kKdMaxDepth][kSwBlock] words (a linearization)
  __shared__ double sh[kSwWaves][kSwStride];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kSwBlock) + tid;
  bool inl = false;
  double J[3][12], MJ[3][12], r[3] = {0.0, 0.0, 0.0}, e = 0.0;
#pragma unroll
  for (int m = 0; m < 3; m++)
#pragma unroll
    for (int c = 0; c < 12; c++) J[m][c] = MJ[m][c] = 0.0;
  if (i < a.n) {
    const double al = static_cast<double>(a.times[i]) - a.ref_time;
    Pose12 E;
    twist_pose(a.c, al, E.r, E.t);
    double px, py, pz, qx, qy, qz;
    posed_point(E, a.pts[i], px, py, pz);  // p'_i - os
    qx = a.T.r[0] * px + a.T.r[1] * py + a.T.r[2] * pz + a.T.t[0];
    qy = a.T.r[3] * px + a.T.r[4] * py + a.T.r[5] * pz + a.T.t[1];
    qz = a.T.r[6] * px + a.T.r[7] * py + a.T.r[8] * pz + a.T.t[2];
    const bool finite = sw_finite(qx) && sw_finite(qy) && sw_finite(qz);  // (a non-finite time makes every entry of E a NaN)
    int idx = -1;
    if constexpr (ERR) {
      idx = finite ? a.j[i] : -1;
    } else {
      long long win = -1ll;
      if (a.tn != 0u && finite) {
        const float fx = static_cast<float>(qx), fy = static_cast<float>(qy), fz = static_cast<float>(qz);
        if (fabsf(fx) <= 3.4028234e38f && fabsf(fy) <= 3.4028234e38f && fabsf(fz) <= 3.4028234e38f) {
          float bound2 = INFINITY;
          if (a.max_dist_sq >= 0.0) {
            const double ex = qx - fx, ey = qy - fy, ez = qz - fz;
            const double reach = sqrt(a.max_dist_sq) + sqrt(ex * ex + ey * ey + ez * ez);
            bound2 = static_cast<float>(reach * reach * (1.0 + 0x1p-20));
          }
          idx = kd_nearest<kSwBlock>(a.g, fx, fy, fz, bound2, -1, sw_stack, tid).idx;
        }
      }
      if (idx >= 0) {
        const float4 c = a.g.pts[idx];
        const double dx = static_cast<double>(c.x) - qx, dy = static_cast<double>(c.y) - qy, dz = static_cast<double>(c.z) - qz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (a.max_dist_sq >= 0.0 && !(d2 <= a.max_dist_sq)) idx = -1;
        if (idx >= 0) win = static_cast<long long>(__float_as_uint(c.w));  // the target point's ORIGINAL index
      }
      a.j[i] = idx;
      if (a.nearest_host != nullptr) a.nearest_host[i] = win;
    }
    if (idx >= 0) {
      inl = true;
      const float4 c = a.g.pts[idx];
      r[0] = static_cast<double>(c.x) - qx, r[1] = static_cast<double>(c.y) - qy, r[2] = static_cast<double>(c.z) - qz;
      Sym3<double> M = {1.0, 0.0, 0.0, 1.0, 0.0, 1.0};
      if (a.factor == SGA_GICP) {
        if constexpr (ERR) {
          const size_t n = a.n;
          M = {a.m[i], a.m[n + i], a.m[2 * n + i], a.m[3 * n + i], a.m[4 * n + i], a.m[5 * n + i]};
        } else {
          Pose12 RE;  // R_T R_Ei
#pragma unroll
          for (int row = 0; row < 3; row++)
#pragma unroll
            for (int col = 0; col < 3; col++) RE.r[3 * row + col] = a.T.r[3 * row] * E.r[col] + a.T.r[3 * row + 1] * E.r[3 + col] + a.T.r[3 * row + 2] * E.r[6 + col];
          double cs[6];
          posed_cov(RE, a.cov[i], cs);
          const Cov8 ct = a.tcov[idx];
          const Sym3<double> S = {ct.xx + cs[0], ct.xy + cs[1], ct.xz + cs[2], ct.yy + cs[3], ct.yz + cs[4], ct.zz + cs[5]};
          M = inverse_sym<double>(S);
          const size_t n = a.n;
          a.m[i] = M.xx, a.m[n + i] = M.xy, a.m[2 * n + i] = M.xz, a.m[3 * n + i] = M.yy, a.m[4 * n + i] = M.yz, a.m[5 * n + i] = M.zz;
        }
      } else if (a.factor == SGA_PLANE_ICP) {
        const float4 nr = a.tnrm[idx];
        M = {static_cast<double>(nr.x) * nr.x, 0.0, 0.0, static_cast<double>(nr.y) * nr.y, 0.0, static_cast<double>(nr.z) * nr.z};
      }
      const double v0 = M.xx * r[0] + M.xy * r[1] + M.xz * r[2], v1 = M.xy * r[0] + M.yy * r[1] + M.yz * r[2], v2 = M.xz * r[0] + M.yz * r[1] + M.zz * r[2];
      e = 0.5 * (r[0] * v0 + r[1] * v1 + r[2] * v2);
      if constexpr (!ERR) {
        const double P[3] = {px + a.os[0], py + a.os[1], pz + a.os[2]};  // p'_i
#pragma unroll
        for (int m = 0; m < 3; m++) {
          const double* R = a.T.r + 3 * m;
          J[m][0] = R[1] * P[2] - R[2] * P[1];
          J[m][1] = R[2] * P[0] - R[0] * P[2];
          J[m][2] = R[0] * P[1] - R[1] * P[0];
          J[m][3] = -R[0], J[m][4] = -R[1], J[m][5] = -R[2];
        }
        // J_xi = a J_T J_l(a xi), a row y of J_T at a time: y ad(x) = [yw x w + yv x v | yv x w] with x = (w, v)
        const double w[3] = {al * a.xi[0], al * a.xi[1], al * a.xi[2]}, v[3] = {al * a.xi[3], al * a.xi[4], al * a.xi[5]};
        const double rho = fabs(al) * a.rho_unit;
        double tw[3][3], tv[3][3], sw[3][3], sv[3][3];
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
          for (int c = 0; c < 3; c++) tw[m][c] = sw[m][c] = J[m][c], tv[m][c] = sv[m][c] = J[m][3 + c];
        double bound = 1.0;
        for (int k = 1; k <= kSwSeriesMax; k++) {
          const double inv = 1.0 / static_cast<double>(k + 1);
          bound *= rho * inv;
          if (bound < 1e-17 && static_cast<double>(k + 2) > 2.0 * rho) break;  // (k = 1 at a = 0: J_xi is zero exactly)
#pragma unroll
          for (int m = 0; m < 3; m++) {
            double c1[3], c2[3], c3[3];
            sw_cross(tw[m], w, c1);
            sw_cross(tv[m], v, c2);
            sw_cross(tv[m], w, c3);
#pragma unroll
            for (int c = 0; c < 3; c++) {
              tw[m][c] = (c1[c] + c2[c]) * inv, tv[m][c] = c3[c] * inv;
              sw[m][c] += tw[m][c], sv[m][c] += tv[m][c];
            }
          }
        }
#pragma unroll
        for (int m = 0; m < 3; m++)
#pragma unroll
          for (int c = 0; c < 3; c++) J[m][6 + c] = al * sw[m][c], J[m][9 + c] = al * sv[m][c];
#pragma unroll
        for (int c = 0; c < 12; c++) {
          MJ[0][c] = M.xx * J[0][c] + M.xy * J[1][c] + M.xz * J[2][c];
          MJ[1][c] = M.xy * J[0][c] + M.yy * J[1][c] + M.yz * J[2][c];
          MJ[2][c] = M.xz * J[0][c] + M.yz * J[1][c] + M.zz * J[2][c];
        }
      }
    }
    if constexpr (!ERR)
      if (a.nearest_host != nullptr) __threadfence_system();
  }
  auto put = [&](int col, double v) {
    v = wave_sum_f64(inl ? v : 0.0);
    if (lane == 0) sh[wave][col] = v;
  };
  if constexpr (ERR) {
    put(0, e);
  } else {
    int col = 0;
#pragma unroll
    for (int p = 0; p < 12; p++)
#pragma unroll
      for (int q = p; q < 12; q++) put(col++, J[0][p] * MJ[0][q] + J[1][p] * MJ[1][q] + J[2][p] * MJ[2][q]);
#pragma unroll
    for (int p = 0; p < 12; p++) put(kSwColB + p, MJ[0][p] * r[0] + MJ[1][p] * r[1] + MJ[2][p] * r[2]);
    put(kSwColE, e);
    put(kSwColN, 1.0);
  }
  __syncthreads();
  constexpr int cols = ERR ? 1 : kSwCols, stride = ERR ? 1 : kSwStride;
  if (tid < cols) a.partials[static_cast<size_t>(blockIdx.x) * stride + tid] = (sh[0][tid] + sh[1][tid]) + (sh[2][tid] + sh[3][tid]);
}

// The rows of partial sums added by ONE workgroup: thread (g, c) adds column c of the rows g, g + 8, ... in turn, the eight groups meet
// in a fixed tree — the order depends on nothing but the number of rows.  out: `cols` sums in a slot of the staging ring.
__global__ __launch_bounds__(kSwSumThreads) void sweep_sum_kernel(const double* __restrict__ partials, uint32_t rows, int stride, int cols, double* __restrict__ out) {
  __shared__ double sh[kSwSumGroups][kSwSumCols];
  const int c = threadIdx.x % kSwSumCols, g = threadIdx.x / kSwSumCols;
  double acc = 0.0;
  if (c < cols)
    for (uint32_t row = g; row < rows; row += kSwSumGroups) acc += partials[static_cast<size_t>(row) * stride + c];
  sh[g][c] = acc;
  __syncthreads();
  if (g != 0 || c >= cols) return;
  out[c] = ((sh[0][c] + sh[1][c]) + (sh[2][c] + sh[3][c])) + ((sh[4][c] + sh[5][c]) + (sh[6][c] + sh[7][c]));
  __threadfence_system();
}

namespace {

bool finite_all(const double* v, int count) {
  for (int k = 0; k < count; k++)
    if (!(v[k] - v[k] == 0.0)) return false;
  return true;
}

// what the sweep calls refuse of their state and their factor (no handle is read)
int sweep_state_check(const sga_factor_params* fp, const double* T, const double* twist, double ref_time) {
  if (T != nullptr && !finite_all(T, 16)) return fail(SGA_ERR_INVALID, "sweep: T has a non-finite entry");
  if (twist != nullptr && !finite_all(twist, 6)) return fail(SGA_ERR_INVALID, "sweep: the twist has a non-finite entry");
  if (!finite_all(&ref_time, 1)) return fail(SGA_ERR_INVALID, "sweep: the reference time is not finite");
  if (fp->robust_kind != SGA_ROBUST_NONE) return fail(SGA_ERR_UNSUPPORTED, "sweep: robust kernels are not available");
  if (fp->factor_kind < 0 || fp->factor_kind > 2) return fail(SGA_ERR_INVALID, "invalid factor_kind %d", fp->factor_kind);
  return SGA_OK;
}

// ... and of their handles
int sweep_handles_check(const sga_context* ctx, const sga_index* target, const sga_cloud* source, const sga_factor_params* fp) {
  if (source->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (target->device != ctx->device) return fail(SGA_ERR_INVALID, "index lives on another device");
  if (target->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_UNSUPPORTED, "sweep registration needs a kd-tree target, not a voxel map or a projective search");
  if (source->n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", source->n);
  if (fp->factor_kind == SGA_GICP && ((source->n > 0 && !source->has_covs) || (target->n > 0 && !target->has_covs))) return fail(SGA_ERR_INVALID, "GICP needs covariances on both source and target");
  if (fp->factor_kind == SGA_PLANE_ICP && target->n > 0 && !target->has_normals) return fail(SGA_ERR_UNSUPPORTED, "PLANE_ICP needs a kd-tree index over a target with normals");
  return SGA_OK;
}

static const double kI16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};

// whose pairs the context holds
void sweep_remember(sga_context* ctx, const sga_index* target, const sga_cloud* source, int factor) {
  ctx->sweep_source = source, ctx->sweep_source_serial = source->serial;
  ctx->sweep_target = target, ctx->sweep_target_serial = target->serial;
  ctx->sweep_n = source->n;
  ctx->sweep_factor = factor;
}
bool sweep_remembered(const sga_context* ctx, const sga_index* target, const sga_cloud* source, int factor) {
  return ctx->sweep_source == source && ctx->sweep_source_serial == source->serial && ctx->sweep_target == target && ctx->sweep_target_serial == target->serial && ctx->sweep_n == source->n && ctx->sweep_factor == factor;
}

// One pass over a non-empty source: the times into a slot of the staging ring, two launches, one wait.  err_only: out[0] = e over the
// stored pairs; otherwise out[0, 92) = the sums and nearest (or null) the winners.
int sweep_pass(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* fp, const double* T, const double* twist, double ref_time, bool err_only, double* out,
               int64_t* nearest) {
  const size_t n = source->n;
  {
    bool on_device = false;
    (void)pinned_device_view(times, n * sizeof(float), &on_device);
    if (on_device) return fail(SGA_ERR_INVALID, "sweep: times is device memory");
  }
  static const double zero6[6] = {0, 0, 0, 0, 0, 0};
  const double* xi = twist ? twist : zero6;
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, target->ready));
  SGA_TRY(wait_ready(ctx, source->ready));
  // one slot: [96 doubles: the sums][n winners, when asked for][n times]
  const size_t words = kSwStride + (nearest != nullptr ? n : 0);
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, words * sizeof(double) + n * sizeof(float), &slot));
  float* times_host = reinterpret_cast<float*>(static_cast<double*>(slot->host) + words);
  double amax = 0.0;
  for (size_t k = 0; k < n; k++) {
    const float s = times[k];
    times_host[k] = s;
    const double al = std::fabs(static_cast<double>(s) - ref_time);
    if (al > amax && al <= 1.7976931348623157e308) amax = al;
  }
  const double rho_unit = std::sqrt(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]) + std::sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
  if (!(amax * rho_unit <= kSwRhoMax)) return fail(SGA_ERR_INVALID, "sweep: the twist moves a point by %g (rad + m) over the sweep; the limit is %g", amax * rho_unit, kSwRhoMax);
  const uint32_t rows = static_cast<uint32_t>((n + kSwBlock - 1) / kSwBlock);
  if (!err_only) {
    ctx->sweep_source = nullptr;  // (until the pairs are stored)
    SGA_TRY(ctx->sweep_j.reserve(n));
    if (fp->factor_kind == SGA_GICP) SGA_TRY(ctx->sweep_m.reserve(6 * n));
    SGA_TRY(ctx->sweep_partials.reserve(static_cast<size_t>(rows) * kSwStride));
  }
  SweepArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pts = source->pts.p;
  a.cov = source->has_covs ? source->cov.p : nullptr;
  a.times = reinterpret_cast<const float*>(static_cast<double*>(slot->dev) + words);
  a.T = insert_pose(T ? T : kI16, source->origin);  // R_T, R_T o_s + t_T
  for (int k = 0; k < 3; k++) a.T.t[k] -= target->origin[k];
  for (int k = 0; k < 3; k++) a.os[k] = source->origin[k];
  a.c = twist_const(xi, source->origin);
  for (int k = 0; k < 6; k++) a.xi[k] = xi[k];
  a.rho_unit = rho_unit;
  a.ref_time = ref_time;
  a.max_dist_sq = fp->max_dist_sq;
  a.g = make_kd_view(target);
  a.tnrm = target->has_normals ? target->nrm.p : nullptr;
  a.tcov = target->has_covs ? target->cov.p : nullptr;
  a.j = ctx->sweep_j.p;
  a.m = ctx->sweep_m.p;
  a.partials = ctx->sweep_partials.p;
  a.nearest_host = nearest != nullptr ? reinterpret_cast<long long*>(static_cast<double*>(slot->dev) + kSwStride) : nullptr;
  a.n = static_cast<uint32_t>(n);
  a.tn = static_cast<uint32_t>(target->n);
  a.factor = fp->factor_kind;
  count_launch(Chain::Sweep);
  if (err_only)
    hipLaunchKernelGGL((sweep_pass_kernel<true>), dim3(rows), dim3(kSwBlock), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL((sweep_pass_kernel<false>), dim3(rows), dim3(kSwBlock), static_cast<size_t>(kKdMaxDepth) * 4 * kSwBlock, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::Sweep);
  hipLaunchKernelGGL(sweep_sum_kernel, dim3(1), dim3(kSwSumThreads), 0, ctx->stream, ctx->sweep_partials.p, rows, err_only ? 1 : kSwStride, err_only ? 1 : kSwCols, static_cast<double*>(slot->dev));
  SGA_HIP(hipGetLastError());
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the pass's one wait: the sums (and the winners) are in the slot
  const double* host = static_cast<const double*>(slot->host);
  std::memcpy(out, host, (err_only ? 1 : kSwCols) * sizeof(double));
  if (nearest != nullptr) std::memcpy(nearest, host + kSwStride, n * sizeof(int64_t));
  if (!err_only) sweep_remember(ctx, target, source, fp->factor_kind);
  return SGA_OK;
}

void sweep_unpack(const double sums[kSwCols], double* H, double* b, double* e, uint64_t* inliers) {
  int col = 0;
  for (int p = 0; p < 12; p++)
    for (int q = p; q < 12; q++) H[12 * p + q] = H[12 * q + p] = sums[col++];
  for (int p = 0; p < 12; p++) b[p] = sums[kSwColB + p];
  *e = sums[kSwColE];
  *inliers = static_cast<uint64_t>(sums[kSwColN]);
}

int sweep_linearize(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* fp, const double* T, const double* twist, double ref_time, double* H, double* b, double* e,
                    uint64_t* inliers, int64_t* nearest) {
  double sums[kSwCols];
  if (source->n == 0) {  // nothing is launched: zero sums, no pairs
    std::memset(sums, 0, sizeof(sums));
    sweep_remember(ctx, target, source, fp->factor_kind);
  } else {
    SGA_TRY(sweep_pass(ctx, target, source, times, fp, T, twist, ref_time, false, sums, nearest));
  }
  sweep_unpack(sums, H, b, e, inliers);
  return SGA_OK;
}

int sweep_error(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* fp, const double* T, const double* twist, double ref_time, double* e) {
  if (!sweep_remembered(ctx, target, source, fp->factor_kind)) return fail(SGA_ERR_INVALID, "sweep: no pairs of this (context, target, source, factor): call sga_sweep_linearize first");
  *e = 0.0;
  if (source->n == 0) return SGA_OK;
  return sweep_pass(ctx, target, source, times, fp, T, twist, ref_time, true, e, nullptr);
}

// (A + lambda I) x = -b for a symmetric 12 x 12: LDL^T with diagonal pivoting (optimizer.hip's, in 12 dimensions)
void solve_damped12(const double* H, const double* b, double lambda, double* x) {
  constexpr int N = 12;
  double A[N][N];
  int p[N];
  for (int i = 0; i < N; i++) {
    p[i] = i;
    for (int j = 0; j < N; j++) A[i][j] = H[N * i + j] + (i == j ? lambda : 0.0);
  }
  for (int k = 0; k < N; k++) {
    int piv = k;
    for (int i = k + 1; i < N; i++)
      if (std::fabs(A[i][i]) > std::fabs(A[piv][piv])) piv = i;
    if (piv != k) {
      for (int j = 0; j < N; j++) std::swap(A[k][j], A[piv][j]);
      for (int i = 0; i < N; i++) std::swap(A[i][k], A[i][piv]);
      std::swap(p[k], p[piv]);
    }
    const double dk = A[k][k];
    if (dk == 0.0) continue;
    for (int i = k + 1; i < N; i++) A[i][k] /= dk;
    for (int i = k + 1; i < N; i++)
      for (int j = k + 1; j <= i; j++) {
        A[i][j] -= A[i][k] * dk * A[j][k];
        A[j][i] = A[i][j];
      }
  }
  double y[N];
  for (int i = 0; i < N; i++) y[i] = -b[p[i]];
  for (int i = 0; i < N; i++)
    for (int j = 0; j < i; j++) y[i] -= A[i][j] * y[j];
  for (int i = 0; i < N; i++) y[i] = A[i][i] != 0.0 ? y[i] / A[i][i] : 0.0;
  for (int i = N - 1; i >= 0; i--)
    for (int j = i + 1; j < N; j++) y[i] -= A[j][i] * y[j];
  for (int i = 0; i < N; i++) x[p[i]] = y[i];
}

double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// T <- T exp(d), column-major
void pose_step(const double T[16], const double d[6], double out[16]) {
  double X[16];
  sga_se3_exp(d, X);
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++) {
      double s = 0.0;
      for (int k = 0; k < 4; k++) s += T[4 * k + r] * X[4 * c + k];
      out[4 * c + r] = s;
    }
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_sweep_params_default(sga_sweep_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->ref_time = 1.0;
}

int sga_sweep_linearize(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* params, const double T[16], const double twist[6], double ref_time, double H[144],
                        double b[12], double* e, uint64_t* num_inliers, int64_t* nearest) {
  if (!ctx || !target || !source || !times || !params || !T || !twist || !H || !b || !e || !num_inliers) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(sweep_state_check(params, T, twist, ref_time));
  // ---- (from here on the handles are read)
  SGA_TRY(sweep_handles_check(ctx, target, source, params));
  return sweep_linearize(ctx, target, source, times, params, T, twist, ref_time, H, b, e, num_inliers, nearest);
}

int sga_sweep_error(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* params, const double T[16], const double twist[6], double ref_time, double* e) {
  if (!ctx || !target || !source || !times || !params || !T || !twist || !e) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(sweep_state_check(params, T, twist, ref_time));
  // ---- (from here on the handles are read)
  SGA_TRY(sweep_handles_check(ctx, target, source, params));
  return sweep_error(ctx, target, source, times, params, T, twist, ref_time, e);
}

// The loop of sga_align (optimizer.hip: optimizer.hpp:83-149, its quirks included) in 12 dimensions: delta = (pose step | twist step)
int sga_align_sweep(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const double init_T[16], const double init_twist[6], const sga_registration_setting* setting,
                    const sga_sweep_params* sweep_params, sga_sweep_result* out) {
  if (!ctx || !target || !source || !times || !setting || !sweep_params || !out) return fail(SGA_ERR_INVALID, "null argument");
  const sga_registration_setting& s = *setting;
  const sga_sweep_params& sp = *sweep_params;
  SGA_TRY(sweep_state_check(&s.factor, init_T, init_twist, sp.ref_time));
  if (!finite_all(sp.twist_prior, 6)) return fail(SGA_ERR_INVALID, "sweep: the twist prior has a non-finite entry");
  if (!finite_all(sp.twist_information, 36)) return fail(SGA_ERR_INVALID, "sweep: the twist information has a non-finite entry");
  bool prior = false;
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      if (sp.twist_information[6 * i + j] != sp.twist_information[6 * j + i]) return fail(SGA_ERR_INVALID, "sweep: the twist information is not symmetric (%d, %d)", i, j);
      prior = prior || sp.twist_information[6 * i + j] != 0.0;
    }
  if (s.restrict_dof_lambda > 0.0) return fail(SGA_ERR_UNSUPPORTED, "sweep: restrict_dof is not available");
  // ---- (from here on the handles are read)
  SGA_TRY(sweep_handles_check(ctx, target, source, &s.factor));
  double T[16], xi[6];
  std::memcpy(T, init_T ? init_T : kI16, sizeof(T));
  for (int k = 0; k < 6; k++) xi[k] = init_twist ? init_twist[k] : 0.0;
  std::memset(out, 0, sizeof(*out));
  std::memcpy(out->T_target_source, T, sizeof(T));
  std::memcpy(out->twist, xi, sizeof(xi));
  if (source->n == 0) return SGA_OK;  // the initial state, not converged; nothing is launched
  if (target->n <= 10) std::fprintf(stderr, "warning: target point cloud is too small. |target|=%zu\n", target->n);
  if (source->n <= 10) std::fprintf(stderr, "warning: source point cloud is too small. |source|=%zu\n", source->n);
  // the prior's share of H, b and e at a twist
  auto prior_error = [&](const double* x) {
    double sum = 0.0;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) sum += (x[i] - sp.twist_prior[i]) * sp.twist_information[6 * i + j] * (x[j] - sp.twist_prior[j]);
    return 0.5 * sum;
  };
  auto linearize = [&](double* H, double* b, double* e, uint64_t* inliers) -> int {
    SGA_TRY(sweep_linearize(ctx, target, source, times, &s.factor, T, xi, sp.ref_time, H, b, e, inliers, nullptr));
    if (!prior) return SGA_OK;
    for (int i = 0; i < 6; i++)
      for (int j = 0; j < 6; j++) {
        H[12 * (6 + i) + 6 + j] += sp.twist_information[6 * i + j];
        b[6 + i] += sp.twist_information[6 * i + j] * (xi[j] - sp.twist_prior[j]);
      }
    *e += prior_error(xi);
    return SGA_OK;
  };
  auto converged = [&](const double* d) { return norm3(d) <= s.rotation_eps && norm3(d + 3) <= s.translation_eps && norm3(d + 6) <= s.rotation_eps && norm3(d + 9) <= s.translation_eps; };
  double H[144], b[12], e = 0.0, delta[12];
  uint64_t inliers = 0;
  if (s.optimizer == SGA_GAUSS_NEWTON) {
    for (int i = 0; i < s.max_iterations && !out->converged; i++) {
      SGA_TRY(linearize(H, b, &e, &inliers));
      solve_damped12(H, b, s.gn_lambda, delta);
      if (s.verbose) std::printf("iter=%d e=%g lambda=%g dt=%g dr=%g dv=%g dw=%g\n", i, e, s.gn_lambda, norm3(delta + 3), norm3(delta), norm3(delta + 9), norm3(delta + 6));
      out->converged = converged(delta);
      double next[16];
      pose_step(T, delta, next);
      std::memcpy(T, next, sizeof(T));
      for (int k = 0; k < 6; k++) xi[k] += delta[6 + k];
      out->iterations = i;
      std::memcpy(out->H, H, sizeof(H));
      std::memcpy(out->b, b, sizeof(b));
      out->error = e;
    }
  } else {
    double lambda = s.init_lambda;
    for (int i = 0; i < s.max_iterations && !out->converged; i++) {
      SGA_TRY(linearize(H, b, &e, &inliers));
      bool success = false;
      for (int j = 0; j < s.max_inner_iterations; j++) {
        solve_damped12(H, b, lambda, delta);
        double new_T[16], new_xi[6], new_e = 0.0;
        pose_step(T, delta, new_T);
        for (int k = 0; k < 6; k++) new_xi[k] = xi[k] + delta[6 + k];
        SGA_TRY(sweep_error(ctx, target, source, times, &s.factor, new_T, new_xi, sp.ref_time, &new_e));
        if (prior) new_e += prior_error(new_xi);
        if (s.verbose) std::printf("iter=%d inner=%d e=%g new_e=%g lambda=%g dt=%g dr=%g dv=%g dw=%g\n", i, j, e, new_e, lambda, norm3(delta + 3), norm3(delta), norm3(delta + 9), norm3(delta + 6));
        if (new_e <= e) {
          out->converged = converged(delta);
          std::memcpy(T, new_T, sizeof(T));
          std::memcpy(xi, new_xi, sizeof(xi));
          lambda /= s.lambda_factor;
          success = true;
          e = new_e;
          break;
        }
        lambda *= s.lambda_factor;
      }
      out->iterations = i;
      std::memcpy(out->H, H, sizeof(H));
      std::memcpy(out->b, b, sizeof(b));
      out->error = e;
      if (!success) break;
    }
  }
  out->num_inliers = inliers;
  std::memcpy(out->T_target_source, T, sizeof(T));
  std::memcpy(out->twist, xi, sizeof(xi));
  return SGA_OK;
}

int sga_debug_sweep_launches(unsigned long long* launches) { return report_launches(Chain::Sweep, launches); }

}  // extern "C"

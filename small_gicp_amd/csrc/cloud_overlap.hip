// A posed cloud compared with a target on the device: sga_cloud_overlap — the distance from every point of a
// cloud, under a pose, to its nearest record of a target index (the exact 1-NN walk of a kd-tree, or the lookup of a Gaussian / flat
// voxel map), the number of points matched within max_distance with the sums behind fitness, RMSE and mean distance formed in double in
// a fixed order, and the crop's stable compaction (cloud_crop.hip: cloud_crop_stat, cloud_ops.hpp) over the matched or the unmatched.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "kd_search.hpp"
#include "voxel_steps.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kOvBlock = 64;  // queries of a workgroup: one lane each, one wave
constexpr int kOvSumThreads = 1024;
enum { kOvKd = 0, kOvGaussian = 1, kOvFlat = 2 };

// What the statistic kernel receives (kernel arguments: read with scalar loads)
struct OverlapArgs {
  const float4* pts;    // the cloud's records, its order
  Pose12 T;             // the cloud's device frame -> the target's: R, (R o_c + t) - o_t
  double max_distance;  // > 0, or +inf
  KdView g;             // kd-tree target
  FlatView v;           // voxel-map target (a Gaussian map reads everything but vnum)
  const float4* tpts;   // ... its means (voxel order) or stored points (kFlatCap slots per voxel)
  double* d;            // n distances, the cloud's order: +inf for a point without a match
  double* flag;         // n, or null: 0.0 where the compaction keeps the point, 1.0 where it does not (held against 0.5)
  double* d_host;       // the distances and the winners into a slot of the staging ring, by its device address; or null
  long long* nearest_host;
  uint32_t n;
  uint32_t tn;          // records of the target: 0 = nothing can be found
  int keep;             // 1: the matched are kept, 2: the unmatched
};

__device__ __forceinline__ bool ov_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

}  // namespace

// d_i, the winner and the keep flag of every point, each written at the point's own index.  One lane per query.
//   KIND kOvKd       the walk of the cold pass (kd_nearest, no seed, no slack) from q32 = float(q_i), its stack in dynamic LDS; the bound
//                    is knn_kernel<true>'s: a record within max_distance of q_i lies within max_distance + |q_i - q32| of q32.  The
//                    winner's distance is then measured in double from q_i.
//   KIND kOvGaussian voxel_nearest<double> over the map's search offsets: the distance to the winning voxel's mean.
//   KIND kOvFlat     flat_nearest<double>: the distance to the stored point.
// A point is matched iff it has a winner and d_i <= max_distance; a q_i with a non-finite coordinate (or beyond fp32's range, for the
// walk) is not searched.
template <int KIND>
__global__ __launch_bounds__(kOvBlock) void overlap_stat_kernel(const OverlapArgs a) {
  extern __shared__ uint32_t ov_stack[];  // kOvKd: [kKdMaxDepth][kOvBlock] words
  const int lane = threadIdx.x;
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kOvBlock) + lane;
  if (i >= a.n) return;  // (the wave-level steps of the walk involve only the lanes that walk)
  const float4 p = a.pts[i];
  double qx, qy, qz;
  posed_point(a.T, p, qx, qy, qz);
  double d = static_cast<double>(INFINITY);
  long long win = -1ll;
  if (a.tn != 0u && ov_finite(qx) && ov_finite(qy) && ov_finite(qz)) {
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (KIND == kOvKd) {
      const float fx = static_cast<float>(qx), fy = static_cast<float>(qy), fz = static_cast<float>(qz);
      if (fabsf(fx) <= 3.4028234e38f && fabsf(fy) <= 3.4028234e38f && fabsf(fz) <= 3.4028234e38f) {
        const double ex = qx - fx, ey = qy - fy, ez = qz - fz;
        const double r = a.max_distance + sqrt(ex * ex + ey * ey + ez * ez);
        const float bound2 = a.max_distance < static_cast<double>(INFINITY) ? static_cast<float>(r * r * (1.0 + 0x1p-20)) : INFINITY;
        const KdBest nb = kd_nearest<kOvBlock>(a.g, fx, fy, fz, bound2, -1, ov_stack, lane);
        if (nb.idx >= 0) {
          c = a.g.pts[nb.idx];
          win = static_cast<long long>(__float_as_uint(c.w));  // the target point's ORIGINAL index
        }
      }
    } else if constexpr (KIND == kOvGaussian) {
      const VoxelView vv{a.v.hkeys, a.v.hvals, a.v.hmask, a.v.inv_leaf, {a.v.org[0], a.v.org[1], a.v.org[2]}, a.v.offsets};
      const int vox = voxel_nearest<double>(vv, a.tpts, qx, qy, qz);
      if (vox >= 0) {
        c = a.tpts[vox];
        win = vox;
      }
    } else {
      win = flat_nearest<double>(a.v, a.tpts, qx, qy, qz, c);  // voxel * kFlatCap + slot
    }
    if (win >= 0) {
      const double dx = static_cast<double>(c.x) - qx, dy = static_cast<double>(c.y) - qy, dz = static_cast<double>(c.z) - qz;
      d = sqrt(dx * dx + dy * dy + dz * dz);
    }
  }
  const bool matched = win >= 0 && d <= a.max_distance;
  if (!matched) {
    d = static_cast<double>(INFINITY);
    win = -1ll;
  }
  a.d[i] = d;
  if (a.flag != nullptr) a.flag[i] = matched == (a.keep == 1) ? 0.0 : 1.0;
  if (a.d_host != nullptr) a.d_host[i] = d;
  if (a.nearest_host != nullptr) a.nearest_host[i] = win;
  if (a.d_host != nullptr || a.nearest_host != nullptr) __threadfence_system();
}

// The number of matched points (the finite d_i), the sum of their d_i^2 and the sum of their d_i, in double, by ONE workgroup and with
// the tree of outlier_threshold_kernel (cloud_outliers.hip): thread t adds the values t, t + 1024, ... into eight partials taken in
// turn, the partials of all threads meet in a fixed tree in LDS — the order depends on nothing but n, and there are no floating-point
// atomics.  out3 = {matched, sum d^2, sum d} in a slot of the staging ring.
__global__ __launch_bounds__(kOvSumThreads) void overlap_sum_kernel(const double* __restrict__ d, uint32_t n, double* __restrict__ out3) {
  __shared__ double sh[3][kOvSumThreads];
  const int tid = threadIdx.x;
  double cnt[8], sq[8], su[8];
#pragma unroll
  for (int u = 0; u < 8; u++) cnt[u] = sq[u] = su[u] = 0.0;
  auto add = [&](int u, double v) {
    const bool m = v < static_cast<double>(INFINITY);  // matched: every other point carries +inf
    const double w = m ? v : 0.0;
    cnt[u] += m ? 1.0 : 0.0;
    sq[u] += w * w;
    su[u] += w;
  };
  uint32_t i = tid;  // (n < 2^31: the index arithmetic does not wrap)
  for (; i + 7u * kOvSumThreads < n; i += 8u * kOvSumThreads) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; u++) v[u] = d[i + u * kOvSumThreads];
#pragma unroll
    for (int u = 0; u < 8; u++) add(u, v[u]);
  }
#pragma unroll
  for (int u = 0; u < 8; u++, i += kOvSumThreads)
    if (i < n) add(u, d[i]);
  auto eight = [](const double* acc) { return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7])); };
  sh[0][tid] = eight(cnt);
  sh[1][tid] = eight(sq);
  sh[2][tid] = eight(su);
  __syncthreads();
  for (int off = kOvSumThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sh[0][tid] += sh[0][tid + off];
      sh[1][tid] += sh[1][tid + off];
      sh[2][tid] += sh[2][tid + off];
    }
    __syncthreads();
  }
  if (tid != 0) return;
  out3[0] = sh[0][0];
  out3[1] = sh[1][0];
  out3[2] = sh[2][0];
  __threadfence_system();
}

namespace {

// what sga_cloud_overlap refuses of its arguments (no handle is read)
int overlap_check(const double* T, const sga_overlap& p, const int64_t* kept, sga_cloud* const* out) {
  if (p.keep < 0 || p.keep > 2) return fail(SGA_ERR_INVALID, "overlap: keep %d is not 0 (no cloud), 1 (the matched) or 2 (the unmatched)", p.keep);
  if (p.keep == 0 && out != nullptr) return fail(SGA_ERR_INVALID, "overlap: keep is 0 but an output cloud is asked for");
  if (p.keep != 0 && out == nullptr) return fail(SGA_ERR_INVALID, "overlap: keep is %d but there is no place for the output cloud", p.keep);
  if (p.keep == 0 && kept != nullptr) return fail(SGA_ERR_INVALID, "overlap: kept is given but keep is 0");
  if (!(p.max_distance > 0.0)) return fail(SGA_ERR_INVALID, "overlap: max_distance must be > 0 (+inf is allowed)");
  for (int k = 0; T != nullptr && k < 16; k++)
    if (!(T[k] - T[k] == 0.0)) return fail(SGA_ERR_INVALID, "overlap: T has a non-finite entry");
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_overlap_default(sga_overlap* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_distance = 1.0;
}

int sga_cloud_overlap(sga_context* ctx, const sga_cloud* cloud, const sga_index* target, const double T[16], const sga_overlap* params, double* dist, int64_t* nearest, int64_t* kept, sga_overlap_stats* stats, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !cloud || !target || !params) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(overlap_check(T, *params, kept, out));
  // ---- (from here on the handles are read)
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (target->device != ctx->device) return fail(SGA_ERR_INVALID, "index lives on another device");
  if (target->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "overlap needs a kd-tree or a voxel map, not a projective search");
  const size_t n = cloud->n;
  CropStat cs{nullptr, nullptr, 0.5, Chain::Overlap};
  if (n == 0) return out ? cloud_crop_stat(ctx, cloud, cs, kept, out) : SGA_OK;  // an empty cloud, zeroed stats; nothing is launched
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", n);
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, target->ready));  // built on another context that returned before its kernels had run
  SGA_TRY(wait_ready(ctx, cloud->ready));
  DevBuf<double> d;  // the distances and, behind them, the keep flags; lives to the end of the call (then: the stream's free list)
  SGA_TRY(d.alloc(out ? 2 * n : n));
  // the three sums, the distances and the winners leave through ONE slot of the staging ring, which the kernels write by its device address
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, (4 + (dist != nullptr ? n : 0) + (nearest != nullptr ? n : 0)) * sizeof(double), &slot));
  double* slot_dev = static_cast<double*>(slot->dev);
  const bool is_kd = target->kind == SGA_INDEX_KDTREE;
  OverlapArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pts = cloud->pts.p;
  a.T = insert_pose(T, cloud->origin);  // R, R o_c + t
  for (int k = 0; k < 3; k++) a.T.t[k] -= target->origin[k];
  a.max_distance = params->max_distance;
  if (is_kd) {
    a.g = make_kd_view(target);
    a.tn = static_cast<uint32_t>(target->n);
  } else {
    a.v = FlatView{target->hkeys.p, target->hvals.p, target->hmask, 1.0 / target->leaf, target->vcounts.p, target->search_offsets, {target->origin[0], target->origin[1], target->origin[2]}};
    a.tpts = target->pts.p;
    a.tn = target->hkeys.p != nullptr ? static_cast<uint32_t>(target->n) : 0u;  // (a map without voxels has no table)
  }
  a.d = d.p;
  a.flag = out ? d.p + n : nullptr;
  a.d_host = dist != nullptr ? slot_dev + 4 : nullptr;
  a.nearest_host = nearest != nullptr ? reinterpret_cast<long long*>(slot_dev + 4 + (dist != nullptr ? n : 0)) : nullptr;
  a.n = static_cast<uint32_t>(n);
  a.keep = params->keep;
  const dim3 grid(static_cast<unsigned>((n + kOvBlock - 1) / kOvBlock));
  count_launch(Chain::Overlap);
  if (is_kd)
    hipLaunchKernelGGL((overlap_stat_kernel<kOvKd>), grid, dim3(kOvBlock), static_cast<size_t>(kKdMaxDepth) * 4 * kOvBlock, ctx->stream, a);
  else if (target->kind == SGA_INDEX_FLATMAP)
    hipLaunchKernelGGL((overlap_stat_kernel<kOvFlat>), grid, dim3(kOvBlock), 0, ctx->stream, a);
  else
    hipLaunchKernelGGL((overlap_stat_kernel<kOvGaussian>), grid, dim3(kOvBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::Overlap);
  hipLaunchKernelGGL(overlap_sum_kernel, dim3(1), dim3(kOvSumThreads), 0, ctx->stream, d.p, a.n, slot_dev);
  SGA_HIP(hipGetLastError());
  sga_cloud* made = nullptr;
  if (out) {
    cs.d = a.flag;
    SGA_TRY(cloud_crop_stat(ctx, cloud, cs, kept, &made));  // (its wait shows that everything above has run)
  } else {
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait: the sums are in the slot
  }
  const double* host = static_cast<const double*>(slot->host);
  if (stats) {
    stats->points = n;
    stats->matched = static_cast<size_t>(host[0]);
    stats->fitness = static_cast<double>(stats->matched) / static_cast<double>(n);
    stats->rmse = stats->matched > 0 ? std::sqrt(host[1] / static_cast<double>(stats->matched)) : 0.0;
    stats->mean_distance = stats->matched > 0 ? host[2] / static_cast<double>(stats->matched) : 0.0;
  }
  if (dist) std::memcpy(dist, host + 4, n * sizeof(double));
  if (nearest) std::memcpy(nearest, host + 4 + (dist != nullptr ? n : 0), n * sizeof(int64_t));
  if (out) *out = made;
  return SGA_OK;
}

int sga_debug_cloud_overlap_launches(unsigned long long* launches) { return report_launches(Chain::Overlap, launches); }

}  // extern "C"

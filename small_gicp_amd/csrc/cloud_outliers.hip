// Outliers removed on the device: sga_cloud_remove_outliers — the mean distance to the k nearest neighbours
// (statistical mode) or the distance to the k-th (radius mode) of every point from the exact k-NN of the cloud's own kd-tree, a threshold
// formed in double on the device, and the crop's stable compaction over the points within it (cloud_crop.hip: cloud_crop_stat,
// cloud_ops.hpp).  No host wait but the crop's.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "knn_wave.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kOutBlock = 64;     // lane route: queries of a workgroup (one wave)
constexpr int kOutWindow = 128;   // ... and the kd positions around them that are scanned before the walk (local_features_kernel's window)
constexpr int kOutMaxK = 63;      // k + 1 entries fit the 64 lanes of the wave route
constexpr int kOutSumThreads = 1024;

// What the statistic kernel receives (kernel arguments: read with scalar loads)
struct OutlierArgs {
  KdView g;        // the tree over the cloud: the queries are its own points
  double* d;       // n values, the cloud's order
  double* d_host;  // the same values into a slot of the staging ring, by its device address; or null
  uint32_t n;
  int k, mode;     // mode 0: mean of the k' = min(k, n - 1) smallest distances to other records; 1: the k-th smallest, +inf when n <= k
};

__device__ __forceinline__ void outlier_write(const OutlierArgs& a, const float4 p, double v) {
  const uint32_t orig = __float_as_uint(p.w);  // the point's position in the cloud (features_from_neighbours' use of the index word)
  a.d[orig] = v;
  if (a.d_host != nullptr) {
    a.d_host[orig] = v;
    __threadfence_system();
  }
}

}  // namespace

// The statistic of every point, written at the point's ORIGINAL index.  The point itself is its own nearest record at distance 0, so
// the search asks for k + 1 entries; distances are the search's fp32 squares (kd_dist2), square-rooted and summed in double.
//   ROUTE 0 — one wave per query (knn_wave.hpp): lane j ends up with the j-th nearest squared distance; lanes 1 .. k' take the root, a
//             butterfly over the wave adds them (a fixed order), lane 0 writes.
//   ROUTE 1 — one lane per query: kd_knn with its list in LDS, unsorted, as local_features_kernel<0> calls it, the lane summing its own
//             list (KS = 0: any k); or, for the k the estimation specialises too (KS = k + 1 = 11 / 21), kd_knn_own_points with the
//             list in registers, as local_features_kernel<10 / 20> calls it.  That search orders TRUNCATED distances and is exact in
//             the SET it returns, so the distances are formed again from the neighbours' records (kd_dist2: the values of the other
//             forms); ties at the k-th distance change the set, never the multiset of distances.
// Neither route stores a neighbour list in memory.
template <int ROUTE, int KS = 0>
__global__ __launch_bounds__(kOutBlock) void outlier_stat_kernel(const OutlierArgs a) {
  const int lane = threadIdx.x;
  const int k = a.k;
  if constexpr (ROUTE == 0) {
    __shared__ uint32_t stack[2 * kKdMaxDepth + 2];
    const uint32_t i = blockIdx.x;  // < n: the grid is n workgroups
    float bd;
    int bid;
    knn_wave_query(a.g, i, k + 1, lane, stack, bd, bid);
    const int kp = min(static_cast<uint32_t>(k), a.n - 1u);
    double v;
    if (a.mode == 0) {  // (uniform)
      v = lane >= 1 && lane <= kp ? sqrt(static_cast<double>(bd)) : 0.0;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
      v = kp > 0 ? v / static_cast<double>(kp) : 0.0;
    } else {
      v = a.n > static_cast<uint32_t>(k) ? sqrt(static_cast<double>(wave_read_f(bd, k))) : static_cast<double>(INFINITY);
    }
    if (lane == 0) outlier_write(a, a.g.pts[i], v);
  } else {
    extern __shared__ float sh[];
    __shared__ float4 window[kOutWindow];
    const int kk = k + 1;
    const int kpad = KS > 0 ? 0 : (kk + 3) & ~3;  // kd_knn sweeps the list four slots at a time; KS > 0: the dynamic LDS is the stack alone
    float* sd = sh;
    int* si = reinterpret_cast<int*>(sh + static_cast<size_t>(kpad) * kOutBlock);
    uint32_t* stack = reinterpret_cast<uint32_t*>(sh + 2 * static_cast<size_t>(kpad) * kOutBlock);
    const uint32_t base = blockIdx.x * kOutBlock;
    const uint32_t i = base + lane;
    for (int j = 0; j < kpad; j++) {
      sd[j * kOutBlock + lane] = INFINITY;
      si[j * kOutBlock + lane] = -1;
    }
    const uint32_t pre_first = base > (kOutWindow - kOutBlock) / 2 ? base - (kOutWindow - kOutBlock) / 2 : 0u;
    const uint32_t pre_end = min(pre_first + kOutWindow, a.n);
    for (uint32_t w = lane; w < pre_end - pre_first; w += kOutBlock) window[w] = a.g.pts[pre_first + w];
    __syncthreads();
    if (i >= a.n) return;
    const float4 p = a.g.pts[i];
    double sum = 0.0;
    float far2 = 0.f;
    int found = 0;  // the list is filled from the front; the point itself (distance 0) is one of its entries
    if constexpr (KS > 0) {
      KnnRegs<KS> L;
      kd_knn_own_points<KS, kOutBlock>(a.g, p.x, p.y, p.z, L, window, pre_first, pre_end, min(base, pre_end), min(base + kOutBlock, pre_end), stack, lane);
#pragma unroll
      for (int j = 0; j < KS; j++) {
        if (L.id[j] < 0) continue;  // (the entries behind the last neighbour)
        const float4 q = a.g.pts[L.id[j]];
        const float d2 = kd_dist2(q.x, q.y, q.z, p.x, p.y, p.z);
        sum += sqrt(static_cast<double>(d2));
        far2 = fmaxf(far2, d2);
        found++;
      }
    } else {
      kd_knn<kOutBlock>(a.g, p.x, p.y, p.z, kk, INFINITY, sd, si, stack, lane, false, pre_first, pre_end, window, base, base + kOutBlock);
      for (int j = 0; j < kk; j++) {
        if (si[j * kOutBlock + lane] < 0) break;
        const float d2 = sd[j * kOutBlock + lane];
        sum += sqrt(static_cast<double>(d2));
        far2 = fmaxf(far2, d2);
        found++;
      }
    }
    double v;
    if (a.mode == 0)
      v = found > 1 ? sum / static_cast<double>(found - 1) : 0.0;
    else
      v = found == kk ? sqrt(static_cast<double>(far2)) : static_cast<double>(INFINITY);
    outlier_write(a, p, v);
  }
}

// mean, stddev (n - 1) and the threshold of the n values, in double, by ONE workgroup: thread t adds the values t, t + 1024, ... into
// eight partials taken in turn (eight loads in flight), the partials of all threads meet in a fixed tree — the order depends on nothing
// but n, and there are no floating-point atomics — once for the mean and once for the squared deviations from it.  limit (statistical
// mode) receives the threshold for the compaction behind this launch; out3 (or null): {mean, stddev, threshold} into a slot of the
// staging ring.
__global__ __launch_bounds__(kOutSumThreads) void outlier_threshold_kernel(const double* __restrict__ d, uint32_t n, int mode, double std_mul, double radius, double* __restrict__ limit, double* __restrict__ out3) {
  __shared__ double sh[kOutSumThreads];
  const int tid = threadIdx.x;
  auto block_sum = [&](double v) {
    sh[tid] = v;
    __syncthreads();
    for (int off = kOutSumThreads / 2; off > 0; off >>= 1) {
      if (tid < off) sh[tid] += sh[tid + off];
      __syncthreads();
    }
    const double total = sh[0];
    __syncthreads();
    return total;
  };
  auto strided_sum = [&](auto term) {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    uint32_t i = tid;  // (n < 2^31: the index arithmetic does not wrap)
    for (; i + 7u * kOutSumThreads < n; i += 8u * kOutSumThreads) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = d[i + u * kOutSumThreads];
#pragma unroll
      for (int u = 0; u < 8; u++) acc[u] += term(v[u]);
    }
#pragma unroll
    for (int u = 0; u < 8; u++, i += kOutSumThreads)
      if (i < n) acc[u] += term(d[i]);
    return ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
  };
  const double mean = block_sum(strided_sum([](double v) { return v; })) / static_cast<double>(n);
  const double ssq = block_sum(strided_sum([mean](double v) { return (v - mean) * (v - mean); }));
  if (tid != 0) return;
  const double stddev = n > 1u ? sqrt(ssq / static_cast<double>(n - 1u)) : 0.0;
  const double threshold = mode == 0 ? mean + std_mul * stddev : radius;
  if (limit != nullptr) *limit = threshold;
  if (out3 != nullptr) {
    out3[0] = mean;
    out3[1] = stddev;
    out3[2] = threshold;
    __threadfence_system();
  }
}

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

// what sga_cloud_remove_outliers refuses of the filter (nothing but the struct is read)
int outlier_check(const sga_outlier_filter& f) {
  if (f.mode != 0 && f.mode != 1) return fail(SGA_ERR_INVALID, "outlier filter: mode %d is not 0 (statistical) or 1 (radius)", f.mode);
  if (f.k < 1 || f.k > kOutMaxK) return fail(SGA_ERR_INVALID, "outlier filter: k must be in [1,%d] (the point and its k neighbours fill the 64 lanes of a wave)", kOutMaxK);
  if (f.mode == 0 && !(is_finite(f.std_mul) && f.std_mul >= 0.0)) return fail(SGA_ERR_INVALID, "outlier filter: std_mul must be finite and >= 0");
  if (f.mode == 1 && !(is_finite(f.radius) && f.radius > 0.0)) return fail(SGA_ERR_INVALID, "outlier filter: radius must be finite and > 0");
  return SGA_OK;
}

struct IndexDestroy {
  void operator()(sga_index* i) const { (void)sga_index_destroy(i); }
};

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_outlier_filter_default(sga_outlier_filter* filter) {
  if (!filter) return;
  std::memset(filter, 0, sizeof(*filter));
  filter->k = 10;
  filter->std_mul = 1.0;
}

int sga_cloud_remove_outliers(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree, const sga_outlier_filter* filter, int64_t* kept, double* stat, sga_outlier_stats* stats, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !cloud || !filter || !out) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(outlier_check(*filter));
  // ---- (from here on the handles are read)
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (kdtree) {  // checked as sga_estimate_normals_covariances checks it
    if (kdtree->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "outlier removal needs a kd-tree index, not a projective search");
    if (kdtree->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_INVALID, "a kd-tree index is required");
    if (kdtree->n != n) return fail(SGA_ERR_INVALID, "index was built over a cloud of %zu points, got %zu", kdtree->n, n);
    for (int a = 0; a < 3; a++)
      if (kdtree->origin[a] != cloud->origin[a]) return fail(SGA_ERR_INVALID, "the index was not built over this cloud (their device frames differ)");
  }
  CropStat cs{nullptr, nullptr, filter->radius};
  if (n == 0) return cloud_crop_stat(ctx, cloud, cs, kept, out);  // an empty cloud, zeroed stats; nothing is launched
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", n);
  SGA_ENTER(ctx);
  std::unique_ptr<sga_index, IndexDestroy> temp;
  const sga_index* index = kdtree;
  if (!index) {  // (refuses a cloud with a non-finite coordinate)
    sga_index* made = nullptr;
    SGA_TRY(sga_index_build_kdtree(ctx, cloud, &made));
    temp.reset(made);
    index = made;
  } else {
    SGA_TRY(wait_ready(ctx, index->ready));  // built on another context that returned before its kernels had run
  }
  SGA_TRY(wait_ready(ctx, cloud->ready));
  DevBuf<double> d;  // the statistic and, behind it, the threshold; lives to the end of the call (then: the stream's free list)
  SGA_TRY(d.alloc(n + 1));
  // mean / stddev / threshold and the statistic leave through ONE slot of the staging ring, which the kernels write by its device address
  const bool reduce = filter->mode == 0 || stats != nullptr;
  sga_context::StageSlot* slot = nullptr;
  if (stat != nullptr || stats != nullptr) SGA_TRY(stage_acquire(ctx, (4 + (stat != nullptr ? n : 0)) * sizeof(double), &slot));
  double* slot_dev = slot ? static_cast<double*>(slot->dev) : nullptr;
  OutlierArgs a;
  a.g = make_kd_view(index);
  a.d = d.p;
  a.d_host = stat != nullptr ? slot_dev + 4 : nullptr;
  a.n = static_cast<uint32_t>(n);
  a.k = filter->k;
  a.mode = filter->mode;
  count_launch(Chain::Outliers);
  if (n <= static_cast<size_t>(knn_wave_max_points())) {  // the rule of sga_estimate_normals_covariances: clouds that do not fill the chip
    hipLaunchKernelGGL((outlier_stat_kernel<0>), dim3(static_cast<unsigned>(n)), dim3(kOutBlock), 0, ctx->stream, a);
  } else {
    const dim3 grid(static_cast<unsigned>((n + kOutBlock - 1) / kOutBlock));
    const size_t stack_bytes = static_cast<size_t>(kKdMaxDepth) * 4 * kOutBlock;
    if (a.k == 10)  // (k = 10 / 20: the list lives in registers, as in sga_estimate_normals_covariances)
      hipLaunchKernelGGL((outlier_stat_kernel<1, 11>), grid, dim3(kOutBlock), stack_bytes, ctx->stream, a);
    else if (a.k == 20)
      hipLaunchKernelGGL((outlier_stat_kernel<1, 21>), grid, dim3(kOutBlock), stack_bytes, ctx->stream, a);
    else
      hipLaunchKernelGGL((outlier_stat_kernel<1>), grid, dim3(kOutBlock), static_cast<size_t>((a.k + 1 + 3) & ~3) * 8 * kOutBlock + stack_bytes, ctx->stream, a);
  }
  SGA_HIP(hipGetLastError());
  if (reduce) {
    count_launch(Chain::Outliers);
    hipLaunchKernelGGL(outlier_threshold_kernel, dim3(1), dim3(kOutSumThreads), 0, ctx->stream, d.p, a.n, a.mode, filter->std_mul, filter->radius, a.mode == 0 ? d.p + n : nullptr, stats != nullptr ? slot_dev : nullptr);
    SGA_HIP(hipGetLastError());
  }
  cs.d = d.p;
  cs.limit = a.mode == 0 ? d.p + n : nullptr;
  sga_cloud* made = nullptr;
  SGA_TRY(cloud_crop_stat(ctx, cloud, cs, kept, &made));  // (its wait shows that everything above has run)
  const double* host = slot ? static_cast<const double*>(slot->host) : nullptr;
  if (stats) {
    stats->mean = host[0];
    stats->stddev = host[1];
    stats->threshold = host[2];
    stats->kept = made->n;
  }
  if (stat) std::memcpy(stat, host + 4, n * sizeof(double));
  *out = made;
  return SGA_OK;
}

int sga_debug_cloud_outliers_launches(unsigned long long* launches) { return report_launches(Chain::Outliers, launches); }

}  // extern "C"

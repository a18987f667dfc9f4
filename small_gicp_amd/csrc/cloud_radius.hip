// Radius search on the device: sga_index_radius_search — for every point of a query cloud the records of a
// kd-tree within a radius, by the fixed-radius walk of kd_radius.hpp (the predicate in double, the pruning in widened fp32): a count
// pass, a prefix by one workgroup, a fill pass.  The counts and the offsets leave through a slot of the staging ring; the lists, whose
// size is known only after the prefix, through two copies behind the fill.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "kd_radius.hpp"

#include <cmath>

namespace sga {
namespace {

constexpr int kRadBlock = 64;  // queries of a workgroup: one lane each, one wave

// What the walk kernels receive (kernel arguments: read with scalar loads)
struct RadiusArgs {
  KdView g;
  const float4* q;      // the query cloud's records, its order
  double ox, oy, oz;    // the query frame's origin minus the tree's
  double radius;
  uint32_t m;
  uint32_t* count;                    // m, device
  long long* count_host;              // m, a slot of the staging ring by its device address
  const unsigned long long* offset;   // m + 1 (fill)
  long long* indices;                 // total (fill)
  double* sq_dists;
};

__device__ __forceinline__ void radius_query(const RadiusArgs& a, uint32_t i, double& qx, double& qy, double& qz) {
  const float4 p = a.q[i];
  qx = static_cast<double>(p.x) + a.ox, qy = static_cast<double>(p.y) + a.oy, qz = static_cast<double>(p.z) + a.oz;
}

}  // namespace

// FILL false: counts[i]; true: the list of query i from offset[i] on, in the walk's order.  One lane per query.
template <bool FILL>
__global__ __launch_bounds__(kRadBlock) void radius_walk_kernel(const RadiusArgs a) {
  extern __shared__ uint32_t rad_stack[];  // [kKdMaxDepth][kRadBlock] words
  const int lane = threadIdx.x;
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kRadBlock) + lane;
  if (i >= a.m) return;  // (the walk has no wave-level step)
  double qx, qy, qz;
  radius_query(a, i, qx, qy, qz);
  if constexpr (FILL) {
    unsigned long long at = a.offset[i];
    auto put = [&](uint32_t j, double d2) {
      a.indices[at] = static_cast<long long>(j);
      a.sq_dists[at] = d2;
      at++;
    };
    kd_radius_walk<kRadBlock>(a.g, qx, qy, qz, a.radius, rad_stack, lane, put);
  } else {
    uint32_t c = 0;
    auto add = [&](uint32_t, double) { c++; };
    kd_radius_walk<kRadBlock>(a.g, qx, qy, qz, a.radius, rad_stack, lane, add);
    a.count[i] = c;
    a.count_host[i] = static_cast<long long>(c);
    __threadfence_system();
  }
}

// offsets[0 .. m] = the exclusive prefix of the counts and their total, to the device and to the slot: one workgroup (kd_radius.hpp)
__global__ __launch_bounds__(kRadScanThreads) void radius_prefix_kernel(const uint32_t* __restrict__ count, uint32_t m, unsigned long long* __restrict__ offset, long long* __restrict__ offset_host) {
  __shared__ unsigned long long sh[kRadScanThreads];
  uint32_t first, end;
  unsigned long long total;
  unsigned long long at = one_block_prefix(m, first, end, sh, total, [&](uint32_t i) { return static_cast<unsigned long long>(count[i]); });
  for (uint32_t i = first; i < end; i++) {
    offset[i] = at;
    offset_host[i] = static_cast<long long>(at);
    at += count[i];
  }
  if (threadIdx.x == 0) {
    offset[m] = total;
    offset_host[m] = static_cast<long long>(total);
  }
  __threadfence_system();
}

}  // namespace sga

using namespace sga;

extern "C" {

int sga_index_radius_search(sga_context* ctx, const sga_index* kdtree, const sga_cloud* queries, double radius, size_t capacity, int64_t* counts, int64_t* offsets, int64_t* indices, double* sq_dists, sga_radius_result* result) {
  if (!ctx || !kdtree || !queries || !counts || !result) return fail(SGA_ERR_INVALID, "null argument");
  if (offsets != nullptr && (indices == nullptr || sq_dists == nullptr)) return fail(SGA_ERR_INVALID, "radius search: lists are asked for (offsets) without room for indices and sq_dists");
  if (!(radius - radius == 0.0 && radius > 0.0)) return fail(SGA_ERR_INVALID, "radius search: radius must be finite and > 0");
  // ---- (from here on the handles are read)
  std::memset(result, 0, sizeof(*result));
  if (queries->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (kdtree->device != ctx->device) return fail(SGA_ERR_INVALID, "index lives on another device");
  if (kdtree->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "radius search needs a kd-tree index, not a projective search");
  if (kdtree->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_INVALID, "a kd-tree index is required");
  const size_t m = queries->n;
  if (m >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", m);
  const bool lists = offsets != nullptr;
  if (m == 0 || kdtree->n == 0) {  // nothing can be found: no device work
    std::memset(counts, 0, m * sizeof(int64_t));
    if (lists) std::memset(offsets, 0, (m + 1) * sizeof(int64_t));
    return SGA_OK;
  }
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, kdtree->ready));
  SGA_TRY(wait_ready(ctx, queries->ready));
  DevBuf<uint32_t> count;
  DevBuf<unsigned long long> offset;
  SGA_TRY(count.alloc(m));
  SGA_TRY(offset.alloc(m + 1));
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, (2 * m + 1) * sizeof(long long), &slot));
  long long* slot_dev = static_cast<long long*>(slot->dev);
  RadiusArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = make_kd_view(kdtree);
  a.q = queries->pts.p;
  a.ox = queries->origin[0] - kdtree->origin[0], a.oy = queries->origin[1] - kdtree->origin[1], a.oz = queries->origin[2] - kdtree->origin[2];
  a.radius = radius;
  a.m = static_cast<uint32_t>(m);
  a.count = count.p;
  a.count_host = slot_dev;
  const dim3 grid(static_cast<unsigned>((m + kRadBlock - 1) / kRadBlock));
  const size_t stack_bytes = static_cast<size_t>(kKdMaxDepth) * 4 * kRadBlock;
  count_launch(Chain::RadiusSearch);
  hipLaunchKernelGGL((radius_walk_kernel<false>), grid, dim3(kRadBlock), stack_bytes, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::RadiusSearch);
  hipLaunchKernelGGL(radius_prefix_kernel, dim3(1), dim3(kRadScanThreads), 0, ctx->stream, count.p, a.m, offset.p, slot_dev + m);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::RadiusWait);
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the counts, the offsets and the total are in the slot
  const long long* host = static_cast<const long long*>(slot->host);
  std::memcpy(counts, host, m * sizeof(int64_t));
  if (lists) std::memcpy(offsets, host + m, (m + 1) * sizeof(int64_t));
  const uint64_t total = static_cast<uint64_t>(host[2 * m]);
  result->total = total;
  if (!lists || total == 0) return SGA_OK;
  if (total > capacity) {
    result->overflow = 1;
    return SGA_OK;
  }
  DevBuf<long long> d_idx;
  DevBuf<double> d_d2;
  SGA_TRY(d_idx.alloc(total));
  SGA_TRY(d_d2.alloc(total));
  a.offset = offset.p;
  a.indices = d_idx.p;
  a.sq_dists = d_d2.p;
  count_launch(Chain::RadiusSearch);
  hipLaunchKernelGGL((radius_walk_kernel<true>), grid, dim3(kRadBlock), stack_bytes, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::RadiusSearch);
  SGA_HIP(hipMemcpyAsync(indices, d_idx.p, total * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  count_launch(Chain::RadiusSearch);
  SGA_HIP(hipMemcpyAsync(sq_dists, d_d2.p, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  count_launch(Chain::RadiusWait);
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  result->written = total;
  return SGA_OK;
}

int sga_debug_radius_search_launches(unsigned long long* launches) { return report_launches(Chain::RadiusSearch, launches); }
int sga_debug_radius_waits(unsigned long long* waits) { return report_launches(Chain::RadiusWait, waits); }

}  // extern "C"

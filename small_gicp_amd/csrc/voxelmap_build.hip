// The one-shot GaussianVoxelMap on the device, lone and batched: what IncrementalVoxelMap::insert + GaussianVoxel::add / finalize
// (ann/incremental_voxelmap.hpp:55-92, ann/gaussian_voxelmap.hpp:32-53) leave behind after ONE insert of a whole cloud.  gfx950.
// Keys -> stable sort by voxel key -> run heads -> scan -> voxel id = rank of the run's first point -> one lane per voxel sums its points
// in insertion order in fp64.  The steps are voxel_steps.hpp's; the sorts are rocPRIM's.
#include <climits>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hpp"
#include "sort_util.hpp"
#include "voxel_steps.hpp"

namespace sga {

// ---- the lone build's kernels -------------------------------------------------------------------------------------------------------------
__global__ void voxel_keys_kernel(const float4* __restrict__ pts, size_t n, double inv_leaf, double ox, double oy, double oz, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int cx, cy, cz;
  const bool bad = build_coords(p, ox, oy, oz, inv_leaf, cx, cy, cz);
  keys[i] = bad ? SGA_HASH_EMPTY : voxel_key(cx, cy, cz);  // out-of-range points sort last and are dropped
  vals[i] = static_cast<uint32_t>(i);
}

__global__ void segment_heads_kernel(const unsigned long long* __restrict__ keys, size_t n, uint32_t* __restrict__ flags) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  flags[i] = (k != SGA_HASH_EMPTY && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
}
void segment_heads(sga_context* ctx, const unsigned long long* keys_sorted, size_t n, uint32_t* flags) {
  hipLaunchKernelGGL(segment_heads_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, keys_sorted, n, flags);
}

__global__ void segment_starts_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ seg_id, const uint32_t* __restrict__ order, size_t n, uint32_t* __restrict__ seg_start, uint32_t* __restrict__ seg_first_idx, uint32_t* __restrict__ seg_ids) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) {
    const uint32_t s = seg_id[i];
    seg_start[s] = static_cast<uint32_t>(i);
    seg_first_idx[s] = order[i];  // stable sort: the first entry of a segment is the earliest inserted point
    seg_ids[s] = s;
  }
}

// One thread per voxel (in voxel-id order)
__global__ void voxel_finalize_kernel(
  const uint32_t* __restrict__ seg_by_rank, uint32_t nvox, const uint32_t* __restrict__ seg_start, uint32_t n_valid, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order,
  const float4* __restrict__ pts, const Cov8* __restrict__ cov, float4* __restrict__ means, Cov8* __restrict__ mcov, int* __restrict__ coords, uint32_t* __restrict__ counts,
  unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hvals, uint32_t hmask) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nvox) return;
  const uint32_t seg = seg_by_rank[v];
  const uint32_t s = seg_start[seg];
  const unsigned long long key = keys[s];
  const uint32_t cnt = voxel_mean_of_run(v, s, n_valid, key, keys, order, pts, cov, means, mcov);
  voxel_key_coords(key, coords + 3 * v);
  counts[v] = cnt;
  voxel_hash_insert(hkeys, hvals, hmask, key, v);
}

__global__ void count_valid_keys_kernel(const unsigned long long* __restrict__ keys, size_t n, unsigned long long* __restrict__ out) {
  unsigned int local = 0;
  for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * blockDim.x) local += keys[i] != SGA_HASH_EMPTY;
  for (int off = 32; off > 0; off >>= 1) local += __shfl_xor(local, off);
  if ((threadIdx.x & 63) == 0 && local) atomicAdd(out, static_cast<unsigned long long>(local));
}

// ---- the build forest: the one-shot maps of B clouds in one chain of launches (voxel_steps.hpp) ----------------------
// Kernels of their own beside the lone ones: a member's pointers and origin come from the call's table instead of the kernel's arguments;
// what decides a map's contents — the voxel coordinates, the fp64 sums — are the functions the lone kernels call.
static_assert(sizeof(VoxMember) % 8 == 0, "table entries are copied as 8-byte words");

// workgroup b: 256 points of the member m with prefix[m] <= b < prefix[m + 1].  Key and value of every point, and the range of the
// member's voxel coordinates.
__global__ __launch_bounds__(256) void voxel_keys_forest_kernel(const VoxMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, double inv_leaf, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const VoxMember& g = *uniform_const(members + m);
  const uint32_t i = (blockIdx.x - prefix[m]) * 256u + threadIdx.x;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < g.n) {
    const float4 p = g.pts[i];
    int cx, cy, cz;
    const bool bad = build_coords(p, g.ox, g.oy, g.oz, inv_leaf, cx, cy, cz);
    keys[g.off + i] = forest_voxel_key(m, cx, cy, cz, bad);
    vals[g.off + i] = i;  // the index within the member
    if (!bad) lo[0] = hi[0] = cx, lo[1] = hi[1] = cy, lo[2] = hi[2] = cz;
  }
  forest_range_reduce(lo, hi, g.range);
}

__global__ void segment_heads_forest_kernel(const unsigned long long* __restrict__ keys, uint32_t n, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];  // (the member number is part of the key: a member's first voxel never continues its neighbour's last)
  flags[i] = ((k & (1ull << 48)) == 0ull && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
}
void segment_heads_forest(sga_context* ctx, const unsigned long long* keys_sorted, uint32_t n, uint32_t* flags) {
  hipLaunchKernelGGL(segment_heads_forest_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, keys_sorted, n, flags);
}

// Sorted position i of the concatenation: the head of a run records the run's start, its number and its rank key (member, index of the
// run's first point: the sort is stable, so the first entry of a run is the earliest inserted point).  The thread at a member's first
// position hands the member's run count and its overflow word to the host; the last member to arrive publishes the call.
__global__ void segment_starts_forest_kernel(const VoxMember* __restrict__ members, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ seg_id, const uint32_t* __restrict__ order, uint32_t n,
                                             uint32_t* __restrict__ seg_start, unsigned long long* __restrict__ rank_keys, uint32_t* __restrict__ seg_ids, const ForestBoxes hand) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = static_cast<uint32_t>(keys[i] >> kVoxKeyMemberShift);
  if (m >= hand.total) return;  // (cannot happen: the keys launch wrote every key with its member's number)
  if (flags[i]) {
    const uint32_t s = seg_id[i];
    seg_start[s] = i;
    rank_keys[s] = (static_cast<unsigned long long>(m) << kVoxRankMemberShift) | order[i];
    seg_ids[s] = s;
  }
  const VoxMember& g = members[m];
  if (i == g.off) {
    const uint32_t end = g.off + g.n;
    const uint32_t r0 = seg_id[i], r1 = end < n ? seg_id[end] : seg_id[n - 1] + flags[n - 1];
    g.count_slot[1] = r1 - r0;
    g.count_slot[2] = forest_range_overflows(g.range) ? 1ull : 0ull;
    forest_box_arrive(hand);
  }
}

// workgroup b: 256 slots of the hash table of the member that owns it
__global__ __launch_bounds__(256) void voxel_clear_forest_kernel(const VoxMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const VoxMember& g = *uniform_const(members + m);
  const uint32_t slot = (blockIdx.x - prefix[m]) * 256u + threadIdx.x;
  if (slot > g.hmask) return;
  g.hkeys[slot] = SGA_HASH_EMPTY;
  g.hvals[slot] = 0u;
}

// workgroup b: 128 voxels (in voxel-id order) of the member that owns it.  The lone kernel's sums over the run's entries up to the end of
// the member's stretch (its dropped points carry another key); the coordinates are those of the run's first point, by the keys kernel's
// function; the voxel goes into the member's own table under the lone build's key.
__global__ __launch_bounds__(128) void voxel_finalize_forest_kernel(const VoxMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, double inv_leaf, const uint32_t* __restrict__ seg_by_rank, const uint32_t* __restrict__ seg_start,
                                                                    const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int mem = forest_member_of(prefix, count, blockIdx.x);
  const VoxMember& g = *uniform_const(members + mem);
  const uint32_t v = (blockIdx.x - prefix[mem]) * 128u + threadIdx.x;
  if (v >= g.nvox) return;
  const uint32_t seg = seg_by_rank[g.run0 + v];
  const uint32_t s = seg_start[seg];
  const float4* __restrict__ pts = g.pts;
  const uint32_t cnt = voxel_mean_of_run(v, s, g.off + g.n, keys[s], keys, order, pts, g.cov, g.means, g.mcov);
  const float4 p0 = pts[order[s]];
  int cx, cy, cz;
  build_coords(p0, g.ox, g.oy, g.oz, inv_leaf, cx, cy, cz);
  g.coords[3 * v + 0] = cx;
  g.coords[3 * v + 1] = cy;
  g.coords[3 * v + 2] = cz;
  g.counts[v] = cnt;
  const unsigned long long hkey = voxel_key(cx, cy, cz);
  const uint32_t hmask = g.hmask;
  unsigned long long* __restrict__ hkeys = g.hkeys;
  uint32_t slot = voxel_hash(hkey) & hmask;
  for (uint32_t probe = 0; probe <= hmask; ++probe) {  // (the table holds 2 x nvox slots: a free one is met long before the probes run out)
    const unsigned long long prev = atomicCAS(&hkeys[slot], SGA_HASH_EMPTY, hkey);
    if (prev == SGA_HASH_EMPTY) {
      g.hvals[slot] = v;
      break;
    }
    slot = (slot + 1) & hmask;
  }
}

int voxel_forest_runs(sga_context* ctx, VoxelForestChain& ch, size_t points, int member_bits, int end_bit, Chain chain, const std::function<int()>& keys_stage) {
  ch.member_bits = member_bits;
  SGA_TRY(ch.keys.alloc(points));
  SGA_TRY(ch.keys_sorted.alloc(points));
  SGA_TRY(ch.vals.alloc(points));
  SGA_TRY(ch.order.alloc(points));
  SGA_TRY(ch.flags.alloc(points));
  SGA_TRY(ch.seg_id.alloc(points));
  SGA_TRY(ch.seg_start.alloc(points));
  SGA_TRY(ch.rank_keys.alloc(points));
  SGA_TRY(ch.seg_ids.alloc(points));
  SGA_TRY(keys_stage());
  count_launch(chain);
  SGA_TRY(sort_pairs(ctx, ch.keys.p, ch.keys_sorted.p, ch.vals.p, ch.order.p, points, 0, static_cast<unsigned>(end_bit)));
  count_launch(chain);
  segment_heads_forest(ctx, ch.keys_sorted.p, static_cast<uint32_t>(points), ch.flags.p);
  SGA_HIP(hipGetLastError());
  count_launch(chain);
  return exclusive_scan(ctx, ch.flags.p, ch.seg_id.p, points);
}

int gaussian_map_new(sga_context* ctx, const sga_cloud* cloud, double leaf, uint32_t nvox, std::unique_ptr<sga_index>& idx) {
  idx.reset(new sga_index);
  idx->kind = SGA_INDEX_VOXELMAP;
  idx->device = ctx->device;
  idx->leaf = leaf;
  idx->has_covs = true;
  idx->has_normals = false;
  for (int k = 0; k < 3; k++) idx->origin[k] = cloud->origin[k];  // the means are averages of the cloud's device-frame records
  idx->n = nvox;
  uint32_t hsize = 16;
  while (hsize < 2 * static_cast<uint64_t>(nvox)) hsize <<= 1;
  idx->hmask = hsize - 1;
  SGA_TRY(idx->hkeys.alloc(hsize));
  return idx->hvals.alloc(hsize);
}
int gaussian_map_alloc_voxels(sga_index* idx) {
  if (idx->n == 0) return SGA_OK;
  SGA_TRY(idx->pts.alloc(idx->n));
  SGA_TRY(idx->cov.alloc(idx->n));
  SGA_TRY(idx->vcoords.alloc(idx->n * 3));
  return idx->vcounts.alloc(idx->n);
}

// `table1`: [members][ranges: 6 ints per member][ticket][prefix of the key grid: count + 1]
int vox_forest_enqueue_runs(sga_context* ctx, const sga_cloud* const* clouds, double leaf, const VoxForestPlan& plan, unsigned long long seq, VoxelForestChain& ch) {
  const size_t count = plan.forest.size();
  if (count == 0) return SGA_OK;
  TableLayout L;
  const auto s_members = L.add<VoxMember>(count);
  const auto s_range = L.add<int>(6 * count);
  const auto s_ticket = L.add<unsigned>(1);
  const auto s_prefix = L.add_prefixes(1, count);
  const uint32_t n32 = static_cast<uint32_t>(plan.points);
  const VoxMember* d_members = nullptr;
  SGA_TRY(voxel_forest_runs(ctx, ch, plan.points, plan.member_bits, plan.end_bit, Chain::VoxBuild, [&]() -> int {
    std::vector<VoxMember> members(count);
    std::vector<uint32_t> prefix(count + 1, 0u);
    SGA_TRY(ch.table1.alloc(L.words()));
    uint32_t off = 0;
    for (size_t j = 0; j < count; j++) {
      const sga_cloud* c = clouds[plan.forest[j]];
      VoxMember& g = members[j];
      std::memset(&g, 0, sizeof(g));
      g.pts = c->pts.p;
      g.cov = c->cov.p;
      g.ox = c->origin[0], g.oy = c->origin[1], g.oz = c->origin[2];
      g.range = L.at(s_range, ch.table1.p) + 6 * j;
      g.count_slot = forest_slot_dev(ctx, j);
      g.n = static_cast<uint32_t>(c->n);
      g.off = off;
      off += g.n;
      prefix[j + 1] = prefix[j] + (g.n + 255u) / 256u;
    }
    count_launch(Chain::VoxBuild);
    SGA_TRY(upload_table(ctx, ch.table1.p, L.words(), [&](unsigned long long* host) {
      L.put(s_members, host, members.data());
      L.put(s_prefix, host, prefix.data());
      voxel_range_identity(L.at(s_range, host), count);
    }));
    d_members = L.at(s_members, ch.table1.p);
    count_launch(Chain::VoxBuild);
    hipLaunchKernelGGL(voxel_keys_forest_kernel, dim3(prefix[count]), dim3(256), 0, ctx->stream, d_members, L.at(s_prefix, ch.table1.p), static_cast<int>(count), 1.0 / leaf, ch.keys.p, ch.vals.p);
    SGA_HIP(hipGetLastError());
    return SGA_OK;
  }));
  const ForestBoxes hand{L.at(s_ticket, ch.table1.p), static_cast<unsigned>(count), ctx->h_forest_dev, seq};
  count_launch(Chain::VoxBuild);
  hipLaunchKernelGGL(segment_starts_forest_kernel, dim3((n32 + 255u) / 256u), dim3(256), 0, ctx->stream, d_members, ch.keys_sorted.p, ch.flags.p, ch.seg_id.p, ch.order.p, n32, ch.seg_start.p, ch.rank_keys.p, ch.seg_ids.p, hand);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// `table2`: [members][prefix of the clearing grid: count + 1][prefix of the finalize grid: count + 1]
int vox_forest_enqueue_finalize(sga_context* ctx, const std::vector<VoxMember>& members, size_t runs, double leaf, VoxelForestChain& ch) {
  const size_t count = members.size();
  if (count == 0) return SGA_OK;
  std::vector<uint32_t> prefix(2 * (count + 1), 0u);
  for (size_t j = 0; j < count; j++) {
    prefix[j + 1] = prefix[j] + (members[j].hmask + 256u) / 256u;
    prefix[count + 1 + j + 1] = prefix[count + 1 + j] + (members[j].nvox + 127u) / 128u;
  }
  const uint32_t* d_prefix = nullptr;
  count_launch(Chain::VoxBuild);
  SGA_TRY(upload_entries(ctx, ch.table2, members, prefix, &d_prefix));
  const VoxMember* d_members = reinterpret_cast<const VoxMember*>(ch.table2.p);
  count_launch(Chain::VoxBuild);
  hipLaunchKernelGGL(voxel_clear_forest_kernel, dim3(prefix[count]), dim3(256), 0, ctx->stream, d_members, d_prefix, static_cast<int>(count));
  SGA_HIP(hipGetLastError());
  if (runs == 0 || prefix[2 * count + 1] == 0) return SGA_OK;  // (every map of the call is empty)
  // voxel id = rank of the voxel's first inserted point within its member: one sort of all runs under (member, index of the first point)
  SGA_TRY(ch.rank_keys_sorted.alloc(runs));
  SGA_TRY(ch.seg_by_rank.alloc(runs));
  count_launch(Chain::VoxBuild);
  SGA_TRY(sort_pairs(ctx, ch.rank_keys.p, ch.rank_keys_sorted.p, ch.seg_ids.p, ch.seg_by_rank.p, runs, 0, static_cast<unsigned>(kVoxRankMemberShift + ch.member_bits)));
  count_launch(Chain::VoxBuild);
  hipLaunchKernelGGL(voxel_finalize_forest_kernel, dim3(prefix[2 * count + 1]), dim3(128), 0, ctx->stream, d_members, d_prefix + count + 1, static_cast<int>(count), 1.0 / leaf, ch.seg_by_rank.p, ch.seg_start.p, ch.keys_sorted.p, ch.order.p);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

}  // namespace sga

using namespace sga;

extern "C" {

int sga_index_build_gaussian_voxelmap(sga_context* ctx, const sga_cloud* cloud, double leaf, sga_index** out) {
  if (!ctx || !cloud || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (!(leaf > 0)) return fail(SGA_ERR_INVALID, "leaf size must be positive");
  if (!cloud->has_covs) return fail(SGA_ERR_INVALID, "GaussianVoxelMap needs point covariances");
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  *out = nullptr;
  SGA_ENTER(ctx);
  const size_t n = cloud->n;
  SGA_TRY(wait_ready(ctx, cloud->ready));
  uint32_t nvox = 0;
  DevBuf<unsigned long long> keys, keys_sorted;
  DevBuf<uint32_t> vals, order, flags, seg_id, seg_start, seg_first, seg_ids, seg_first_sorted, seg_by_rank;
  DevBuf<unsigned long long> d_count;
  unsigned long long n_valid = 0;
  if (n > 0) {
    SGA_TRY(keys.alloc(n));
    SGA_TRY(keys_sorted.alloc(n));
    SGA_TRY(vals.alloc(n));
    SGA_TRY(order.alloc(n));
    SGA_TRY(flags.alloc(n));
    SGA_TRY(seg_id.alloc(n));
    SGA_TRY(d_count.alloc(1));
    hipLaunchKernelGGL(voxel_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, cloud->pts.p, n, 1.0 / leaf, cloud->origin[0], cloud->origin[1], cloud->origin[2], keys.p, vals.p);
    SGA_TRY(sort_pairs(ctx, keys.p, keys_sorted.p, vals.p, order.p, n, 0, 64));
    segment_heads(ctx, keys_sorted.p, n, flags.p);
    SGA_TRY(exclusive_scan(ctx, flags.p, seg_id.p, n));
    SGA_HIP(hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(count_valid_keys_kernel, dim3(256), dim3(256), 0, ctx->stream, keys_sorted.p, n, d_count.p);
    uint32_t last_flag = 0, last_seg = 0;
    SGA_HIP(hipMemcpyAsync(&last_flag, flags.p + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipMemcpyAsync(&last_seg, seg_id.p + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipMemcpyAsync(&n_valid, d_count.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipStreamSynchronize(ctx->stream));
    nvox = last_seg + last_flag;
  }
  std::unique_ptr<sga_index> idx;
  SGA_TRY(gaussian_map_new(ctx, cloud, leaf, nvox, idx));
  SGA_HIP(hipMemsetAsync(idx->hkeys.p, 0xff, idx->hkeys.n * sizeof(unsigned long long), ctx->stream));
  SGA_HIP(hipMemsetAsync(idx->hvals.p, 0, idx->hvals.n * sizeof(uint32_t), ctx->stream));
  if (nvox > 0) {
    SGA_TRY(seg_start.alloc(nvox));
    SGA_TRY(seg_first.alloc(nvox));
    SGA_TRY(seg_ids.alloc(nvox));
    SGA_TRY(seg_first_sorted.alloc(nvox));
    SGA_TRY(seg_by_rank.alloc(nvox));
    hipLaunchKernelGGL(segment_starts_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, flags.p, seg_id.p, order.p, n, seg_start.p, seg_first.p, seg_ids.p);
    // voxel id = rank of the voxel's first inserted point (incremental_voxelmap.hpp:63-69: flat_voxels grows in first-touch order)
    size_t tb = 0;
    SGA_HIP(rocprim::radix_sort_pairs(nullptr, tb, seg_first.p, seg_first_sorted.p, seg_ids.p, seg_by_rank.p, nvox, 0, 32, ctx->stream));
    SGA_TRY(ensure_temp(ctx, tb));
    SGA_HIP(rocprim::radix_sort_pairs(ctx->d_temp.p, tb, seg_first.p, seg_first_sorted.p, seg_ids.p, seg_by_rank.p, nvox, 0, 32, ctx->stream));
    SGA_TRY(gaussian_map_alloc_voxels(idx.get()));
    hipLaunchKernelGGL(
      voxel_finalize_kernel, dim3((nvox + 127) / 128), dim3(128), 0, ctx->stream, seg_by_rank.p, nvox, seg_start.p, static_cast<uint32_t>(n_valid), keys_sorted.p, order.p, cloud->pts.p, cloud->cov.p, idx->pts.p, idx->cov.p,
      idx->vcoords.p, idx->vcounts.p, idx->hkeys.p, idx->hvals.p, idx->hmask);
    SGA_HIP(hipGetLastError());
  }
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  *out = idx.release();
  return SGA_OK;
}

int sga_index_voxelmap_download(sga_context* ctx, const sga_index* index, int32_t* coords, float* means, float* cov6, uint32_t* counts) {
  if (!ctx || !index) return fail(SGA_ERR_INVALID, "null argument");
  if (index->kind != SGA_INDEX_VOXELMAP) return fail(SGA_ERR_INVALID, "not a voxel map");
  const size_t n = index->n;
  if (n == 0) return SGA_OK;
  SGA_ENTER(ctx);
  std::vector<float4> hp;
  std::vector<Cov8> hc;
  if (means) {
    hp.resize(n);
    SGA_HIP(hipMemcpyAsync(hp.data(), index->pts.p, n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (cov6) {
    hc.resize(n);
    SGA_HIP(hipMemcpyAsync(hc.data(), index->cov.p, n * sizeof(Cov8), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (coords) SGA_HIP(hipMemcpyAsync(coords, index->vcoords.p, n * 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (counts) SGA_HIP(hipMemcpyAsync(counts, index->vcounts.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n; i++) {
    if (means) {  // device frame -> the caller's
      means[3 * i] = static_cast<float>(static_cast<double>(hp[i].x) + index->origin[0]);
      means[3 * i + 1] = static_cast<float>(static_cast<double>(hp[i].y) + index->origin[1]);
      means[3 * i + 2] = static_cast<float>(static_cast<double>(hp[i].z) + index->origin[2]);
    }
    if (cov6) {
      cov6[6 * i] = hc[i].xx;
      cov6[6 * i + 1] = hc[i].xy;
      cov6[6 * i + 2] = hc[i].xz;
      cov6[6 * i + 3] = hc[i].yy;
      cov6[6 * i + 4] = hc[i].yz;
      cov6[6 * i + 5] = hc[i].zz;
    }
  }
  return SGA_OK;
}

}  // extern "C"

// Incremental GaussianVoxelMap on the device: repeated insert(points, T) with running per-voxel means and LRU removal — the
// scan-to-model target of the reference (ann/incremental_voxelmap.hpp:55-92 with GaussianVoxel::add / finalize,
// ann/gaussian_voxelmap.hpp:32-53; used by src/benchmark/odometry_benchmark_small_vgicp_model_omp.cpp).  gfx950.
//
// Reference semantics kept:  coord = fast_floor(T p / leaf) in double;  a voxel is created at its first point, voxel ids follow the
// creation order (flat_voxels);  add = un-finalize (mean *= N, cov *= N), N++, mean += T p, cov += T C T^T, point by point in
// insertion order;  finalize = divide by N;  every `clear_cycle` inserts the voxels with lru + horizon < counter are removed
// (order of the others preserved) and the table is rebuilt.
//
// One insert = key generation -> stable radix sort by voxel key (segments = the batch's voxels, points inside a segment in
// insertion order) -> per segment: look the voxel up; new voxels are ranked by their first point = creation order -> one lane per
// segment updates the voxel's fp64 state exactly in the reference's operation order (no floating-point atomics) -> the fp32
// records the VGICP factor kernel reads are refreshed.  The hash table is open addressing on the packed coordinate
// (voxel_hash.hpp), rebuilt when it gets half full or after an LRU sweep.
#include "common.hpp"

#include <cmath>
#include <memory>
#include <rocprim/rocprim.hpp>

#include "sort_util.hpp"
#include "voxel_steps.hpp"

namespace sga {

__global__ void ivm_keys_kernel(const float4* __restrict__ pts, size_t n, Pose12 T, double inv_leaf, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int cx, cy, cz;
  const bool bad = insert_coords(T, p, inv_leaf, cx, cy, cz);
  keys[i] = bad ? SGA_HASH_EMPTY : voxel_key(cx, cy, cz);  // out-of-range points sort last and are dropped
  vals[i] = static_cast<uint32_t>(i);
}

__global__ void ivm_segments_kernel(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ seg_id, const uint32_t* __restrict__ order, size_t n, uint32_t* __restrict__ seg_start, uint32_t* __restrict__ seg_first) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) {
    const uint32_t s = seg_id[i];
    seg_start[s] = static_cast<uint32_t>(i);
    seg_first[s] = order[i];  // stable sort: the first entry of a segment is the earliest inserted point
  }
}

__device__ __forceinline__ uint32_t ivm_find(const unsigned long long* __restrict__ hkeys, const uint32_t* __restrict__ hvals, uint32_t hmask, unsigned long long key) {
  uint32_t slot = voxel_hash(key) & hmask;
  for (;;) {
    const unsigned long long k = hkeys[slot];
    if (k == key) return hvals[slot];
    if (k == SGA_HASH_EMPTY) return 0xffffffffu;
    slot = (slot + 1) & hmask;
  }
}

// existing voxel -> its id; new voxel -> rank key = index of its first point (creation order), counted
__global__ void ivm_lookup_kernel(
  uint32_t nseg, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_first, const unsigned long long* __restrict__ keys, const unsigned long long* __restrict__ hkeys, const uint32_t* __restrict__ hvals,
  uint32_t hmask, uint32_t* __restrict__ seg_vid, uint32_t* __restrict__ rank_key, uint32_t* __restrict__ seg_ids, unsigned int* __restrict__ n_new) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t v = hmask ? ivm_find(hkeys, hvals, hmask, keys[seg_start[s]]) : 0xffffffffu;
  seg_vid[s] = v;
  rank_key[s] = v == 0xffffffffu ? seg_first[s] : 0xffffffffu;
  seg_ids[s] = s;
  if (v == 0xffffffffu) atomicAdd(n_new, 1u);
}

__global__ void ivm_assign_kernel(uint32_t n_new, const uint32_t* __restrict__ seg_by_rank, uint32_t n_old, uint32_t* __restrict__ seg_vid) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r < n_new) seg_vid[seg_by_rank[r]] = n_old + r;
}

__global__ void ivm_rehash_kernel(uint32_t n, const int* __restrict__ coords, unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hvals, uint32_t hmask) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  voxel_hash_insert(hkeys, hvals, hmask, voxel_key(coords[3 * v], coords[3 * v + 1], coords[3 * v + 2]), v);
}

// One lane per voxel of the batch
__global__ void ivm_update_kernel(
  uint32_t nseg, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_vid, uint32_t n_valid, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order, const float4* __restrict__ pts,
  const Cov8* __restrict__ cov, Pose12 T, uint32_t n_old, uint32_t lru_counter, double* __restrict__ mean64, double* __restrict__ cov64, uint32_t* __restrict__ counts, uint32_t* __restrict__ lru, int* __restrict__ coords,
  unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hvals, uint32_t hmask) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t v = seg_vid[s];
  const uint32_t first = seg_start[s];
  const unsigned long long key = keys[first];
  const bool is_new = v >= n_old;
  gaussian_voxel_add(v, is_new, first, n_valid, key, keys, order, pts, cov, T, mean64, cov64, counts);
  lru[v] = lru_counter;
  if (is_new) {
    voxel_key_coords(key, coords + 3 * v);
    voxel_hash_insert(hkeys, hvals, hmask, key, v);
  }
}

__global__ void ivm_keep_kernel(uint32_t n, const uint32_t* __restrict__ lru, uint32_t horizon, uint32_t counter, uint32_t* __restrict__ keep) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n) keep[v] = (static_cast<unsigned long long>(lru[v]) + horizon < counter) ? 0u : 1u;
}

__global__ void ivm_compact_kernel(
  uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, const double* __restrict__ m_in, const double* __restrict__ c_in, const uint32_t* __restrict__ cnt_in, const uint32_t* __restrict__ lru_in,
  const int* __restrict__ co_in, double* __restrict__ m_out, double* __restrict__ c_out, uint32_t* __restrict__ cnt_out, uint32_t* __restrict__ lru_out, int* __restrict__ co_out) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || !keep[v]) return;
  const uint32_t w = pos[v];
  for (int k = 0; k < 3; k++) {
    m_out[3 * w + k] = m_in[3 * v + k];
    co_out[3 * w + k] = co_in[3 * v + k];
  }
  for (int k = 0; k < 6; k++) c_out[6 * w + k] = c_in[6 * v + k];
  cnt_out[w] = cnt_in[v];
  lru_out[w] = lru_in[v];
}

__global__ void ivm_export_kernel(uint32_t n, const double* __restrict__ mean64, const double* __restrict__ cov64, double ox, double oy, double oz, float4* __restrict__ means, Cov8* __restrict__ mcov) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  gaussian_voxel_export(v, mean64, cov64, ox, oy, oz, means, mcov);
}

// ---- the insert forest: B inserts in one chain of launches (voxel_steps.hpp) -------------------------------------
// Kernels of their own beside the lone ones: the pose and the pointers come from the call's tables instead of the kernel's arguments; what
// decides a map's contents — the posed point, the voxel coordinates, the fp64 un-finalize / add / finalize — are the functions the lone
// kernels call.
static_assert(sizeof(IvmMember) % 8 == 0 && sizeof(IvmUpdate) % 8 == 0 && sizeof(IvmExport) % 8 == 0, "table entries are copied as 8-byte words");

// workgroup b: 256 points of the member m with prefix[m] <= b < prefix[m + 1].  ivm_keys_kernel's coordinates under the forests' key, and
// the range of the member's voxel coordinates.
__global__ __launch_bounds__(256) void ivm_keys_forest_kernel(const IvmMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const IvmMember& g = *uniform_const(members + m);
  const uint32_t i = (blockIdx.x - prefix[m]) * 256u + threadIdx.x;
  int lo[3] = {INT_MAX, INT_MAX, INT_MAX}, hi[3] = {INT_MIN, INT_MIN, INT_MIN};
  if (i < g.n) {
    const float4 p = g.pts[i];
    int cx, cy, cz;
    const bool bad = insert_coords(g.T, p, g.inv_leaf, cx, cy, cz);
    keys[g.off + i] = forest_voxel_key(m, cx, cy, cz, bad);  // a member's dropped points sort last in its stretch
    vals[g.off + i] = i;  // the index within the member
    if (!bad) lo[0] = hi[0] = cx, lo[1] = hi[1] = cy, lo[2] = hi[2] = cz;
  }
  forest_range_reduce(lo, hi, g.range);
}

// Sorted position i of the concatenation.  The head of a run records the run's start and number and does ivm_lookup_kernel's work: the
// voxel's LONE key, recomputed from the run's first point (the sort is stable: the earliest inserted one), looked up in the member's own
// table; an existing voxel's id, or the rank key (member, index of the first point) of a new one, counted per member.  An existing voxel's
// rank key carries the member number `total`: those runs sort behind every new one, in run order.
// A member's counts are final when the launch has finished all its positions: every workgroup adds the positions it covered to the
// member's second counter, and the one that completes the member hands run count, overflow word and new-voxel count to the host (the
// last member to arrive publishes the call).
__global__ __launch_bounds__(256) void ivm_starts_forest_kernel(const IvmMember* __restrict__ members, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ flags, const uint32_t* __restrict__ seg_id, const uint32_t* __restrict__ order,
                                                                uint32_t n, uint32_t* __restrict__ seg_start, uint32_t* __restrict__ seg_vid, unsigned long long* __restrict__ rank_keys, uint32_t* __restrict__ seg_ids, const ForestBoxes hand) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < n && flags[i]) {
    const uint32_t m = static_cast<uint32_t>(keys[i] >> kVoxKeyMemberShift);
    if (m < hand.total) {  // (always: the keys launch wrote every key with its member's number)
      const IvmMember& g = members[m];
      const uint32_t s = seg_id[i], first = order[i];
      const float4 p = g.pts[first];
      int cx, cy, cz;
      insert_coords(g.T, p, g.inv_leaf, cx, cy, cz);
      const uint32_t hmask = g.hmask;
      const uint32_t v = hmask ? ivm_find(g.hkeys, g.hvals, hmask, voxel_key(cx, cy, cz)) : 0xffffffffu;
      seg_start[s] = i;
      seg_vid[s] = v;
      rank_keys[s] = v == 0xffffffffu ? ((static_cast<unsigned long long>(m) << kVoxRankMemberShift) | first) : (static_cast<unsigned long long>(hand.total) << kVoxRankMemberShift);
      seg_ids[s] = s;
      if (v == 0xffffffffu) atomicAdd(g.counters, 1u);
    }
  }
  __syncthreads();
  const uint32_t b0 = blockIdx.x * 256u, b1 = min(b0 + 256u, n);
  const uint32_t m0 = static_cast<uint32_t>(keys[b0] >> kVoxKeyMemberShift), m1 = min(static_cast<uint32_t>(keys[b1 - 1u] >> kVoxKeyMemberShift), hand.total - 1u);
  for (uint32_t m = m0 + threadIdx.x; m <= m1; m += 256u) {  // the members with positions in [b0, b1)
    const IvmMember& g = members[m];
    const uint32_t end = g.off + g.n;
    const uint32_t covered = min(b1, end) - max(b0, g.off);
    __threadfence();
    if (__hip_atomic_fetch_add(g.counters + 1, covered, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) + covered != g.n) continue;
    const uint32_t r0 = seg_id[g.off], r1 = end < n ? seg_id[end] : seg_id[n - 1] + flags[n - 1];
    g.count_slot[1] = r1 - r0;
    g.count_slot[2] = forest_range_overflows(g.range) ? 1ull : 0ull;
    g.count_slot[3] = __hip_atomic_load(g.counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    forest_box_arrive(hand);
  }
}

// workgroup b: 128 runs of the member that owns it, the member's new voxels first (in creation order: the ranks' order), then its existing
// ones.  ivm_assign_kernel (voxel id = n_old + rank) and ivm_update_kernel's add over the run's entries up to the end of the member's
// stretch (its dropped points carry another key); a new voxel's coordinates are those of the run's first point, by the keys kernel's
// function, and it goes into the member's own table under the lone key.
__global__ __launch_bounds__(128) void ivm_update_forest_kernel(const IvmUpdate* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, uint32_t total_new, const uint32_t* __restrict__ seg_by_rank,
                                                                const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_vid, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int mem = forest_member_of(prefix, count, blockIdx.x);
  const IvmUpdate& g = *uniform_const(members + mem);
  const uint32_t j = (blockIdx.x - prefix[mem]) * 128u + threadIdx.x;
  if (j >= g.nseg) return;
  const bool is_new = j < g.n_new;
  const uint32_t s = seg_by_rank[is_new ? g.new0 + j : total_new + g.old0 + (j - g.n_new)];
  const uint32_t v = is_new ? g.n_old + j : seg_vid[s];
  const uint32_t first = seg_start[s];
  const float4* __restrict__ pts = g.pts;
  gaussian_voxel_add(v, is_new, first, g.end, keys[first], keys, order, pts, g.cov, g.T, g.mean64, g.cov64, g.counts);
  g.lru[v] = g.lru_counter;
  if (is_new) {
    const float4 p = pts[order[first]];
    int cx, cy, cz;
    insert_coords(g.T, p, g.inv_leaf, cx, cy, cz);
    g.coords[3 * v + 0] = cx;
    g.coords[3 * v + 1] = cy;
    g.coords[3 * v + 2] = cz;
    voxel_hash_insert(g.hkeys, g.hvals, g.hmask, voxel_key(cx, cy, cz), v);
  }
}

// workgroup b: 256 voxels of the map that owns it
__global__ __launch_bounds__(256) void ivm_export_forest_kernel(const IvmExport* __restrict__ maps, const uint32_t* __restrict__ prefix_g, int count) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int mem = forest_member_of(prefix, count, blockIdx.x);
  const IvmExport& g = *uniform_const(maps + mem);
  const uint32_t v = (blockIdx.x - prefix[mem]) * 256u + threadIdx.x;
  if (v >= g.n) return;
  gaussian_voxel_export(v, g.mean64, g.cov64, g.ox, g.oy, g.oz, g.means, g.mcov);
}

// ---- flat maps: IncrementalVoxelMap<FlatContainer<NRM, COV>> ------------------------------------------------------------------------
// One lane per voxel of the batch: FlatContainer::add for its points in insertion order (flat_container.hpp:33-58): a point is
// kept iff the cell holds fewer than max_points and no kept point lies closer than sqrt(min_sq); kept = T p, with the normal R n
// (T.matrix() * normal, w = 0) and the covariance R C R^T where the map keeps them.  The decision reads the points alone: every kind of
// contents keeps the same points in the same slots.  Kinds without covariances (normals) read no cloud covariances (normals).
template <bool NRM, bool COV>
__global__ void fvm_update_kernel(
  uint32_t nseg, const uint32_t* __restrict__ seg_start, const uint32_t* __restrict__ seg_vid, uint32_t n_valid, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order, const float4* __restrict__ pts,
  const float4* __restrict__ nrm, const Cov8* __restrict__ cov, Pose12 T, uint32_t n_old, uint32_t lru_counter, uint32_t max_points, double min_sq, double* __restrict__ fpts64, double* __restrict__ fnrm64,
  double* __restrict__ fcov64, uint32_t* __restrict__ counts, uint32_t* __restrict__ lru, int* __restrict__ coords, unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hvals, uint32_t hmask) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= nseg) return;
  const uint32_t v = seg_vid[s];
  const uint32_t first = seg_start[s];
  const unsigned long long key = keys[first];
  const bool is_new = v >= n_old;
  uint32_t cnt = is_new ? 0u : counts[v];
  double* P = fpts64 + static_cast<size_t>(v) * kFlatCap * 3;
  for (uint32_t i = first; i < n_valid && keys[i] == key; ++i) {
    if (cnt >= max_points) break;  // every further point of this batch would be rejected as well
    const uint32_t src = order[i];
    const float4 p = pts[src];
    double x, y, z;
    posed_point(T, p, x, y, z);
    bool reject = false;
    for (uint32_t j = 0; j < cnt && !reject; j++) {
      const double dx = P[3 * j] - x, dy = P[3 * j + 1] - y, dz = P[3 * j + 2] - z;
      reject = dx * dx + dy * dy + dz * dz < min_sq;
    }
    if (reject) continue;
    P[3 * cnt] = x;
    P[3 * cnt + 1] = y;
    P[3 * cnt + 2] = z;
    if constexpr (NRM) {  // T.matrix() * (nx, ny, nz, 0): the translation column meets the zero w
      const float4 q = nrm[src];
      double* N = fnrm64 + (static_cast<size_t>(v) * kFlatCap + cnt) * 3;
      for (int a = 0; a < 3; a++) N[a] = T.r[3 * a] * q.x + T.r[3 * a + 1] * q.y + T.r[3 * a + 2] * q.z;
    }
    if constexpr (COV) {
      const Cov8 q = cov[src];
      posed_cov(T, q, fcov64 + (static_cast<size_t>(v) * kFlatCap + cnt) * 6);
    }
    cnt++;
  }
  counts[v] = cnt;
  lru[v] = lru_counter;
  if (is_new) {
    voxel_key_coords(key, coords + 3 * v);
    voxel_hash_insert(hkeys, hvals, hmask, key, v);
  }
}

template <bool NRM, bool COV>
__global__ void fvm_compact_kernel(
  uint32_t n, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ pos, const double* __restrict__ p_in, const double* __restrict__ n_in, const double* __restrict__ c_in, const uint32_t* __restrict__ cnt_in,
  const uint32_t* __restrict__ lru_in, const int* __restrict__ co_in, double* __restrict__ p_out, double* __restrict__ n_out, double* __restrict__ c_out, uint32_t* __restrict__ cnt_out, uint32_t* __restrict__ lru_out,
  int* __restrict__ co_out) {
  const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n || !keep[v]) return;
  const uint32_t w = pos[v];
  for (int k = 0; k < 3; k++) co_out[3 * w + k] = co_in[3 * v + k];
  const uint32_t cnt = cnt_in[v];
  for (uint32_t j = 0; j < cnt; j++) {
    const size_t so = static_cast<size_t>(w) * kFlatCap + j, si = static_cast<size_t>(v) * kFlatCap + j;
    for (int k = 0; k < 3; k++) p_out[so * 3 + k] = p_in[si * 3 + k];
    if constexpr (NRM)
      for (int k = 0; k < 3; k++) n_out[so * 3 + k] = n_in[si * 3 + k];
    if constexpr (COV)
      for (int k = 0; k < 6; k++) c_out[so * 6 + k] = c_in[si * 6 + k];
  }
  cnt_out[w] = cnt;
  lru_out[w] = lru_in[v];
}

// fp32 records read by the factor kernels: slot = voxel * kFlatCap + i, w = slot; normals {nx, ny, nz, 0} under the same slot numbering
template <bool NRM, bool COV>
__global__ void fvm_export_kernel(uint32_t n, const uint32_t* __restrict__ counts, const double* __restrict__ fpts64, const double* __restrict__ fnrm64, const double* __restrict__ fcov64, double ox, double oy, double oz,
                                  float4* __restrict__ pts, float4* __restrict__ nrm, Cov8* __restrict__ cov) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t v = t / kFlatCap, j = t % kFlatCap;
  if (v >= n) return;
  if (j >= counts[v]) {
    pts[t] = make_float4(INFINITY, INFINITY, INFINITY, __uint_as_float(t));
    return;
  }
  pts[t] = make_float4(static_cast<float>(fpts64[3 * static_cast<size_t>(t)] - ox), static_cast<float>(fpts64[3 * static_cast<size_t>(t) + 1] - oy), static_cast<float>(fpts64[3 * static_cast<size_t>(t) + 2] - oz), __uint_as_float(t));
  if constexpr (NRM) {
    const double* q = fnrm64 + 3 * static_cast<size_t>(t);
    nrm[t] = make_float4(static_cast<float>(q[0]), static_cast<float>(q[1]), static_cast<float>(q[2]), 0.f);
  }
  if constexpr (COV) {
    const double* c = fcov64 + 6 * static_cast<size_t>(t);
    cov[t] = cov8_of(c[0], c[1], c[2], c[3], c[4], c[5]);
  }
}

// the instantiation for a map's contents
#define SGA_FLAT_DISPATCH(idx, KERNEL, ...)                                                                         \
  do {                                                                                                              \
    if ((idx)->has_normals && (idx)->has_covs) hipLaunchKernelGGL((KERNEL<true, true>), __VA_ARGS__);              \
    else if ((idx)->has_normals) hipLaunchKernelGGL((KERNEL<true, false>), __VA_ARGS__);                           \
    else if ((idx)->has_covs) hipLaunchKernelGGL((KERNEL<false, true>), __VA_ARGS__);                              \
    else hipLaunchKernelGGL((KERNEL<false, false>), __VA_ARGS__);                                                  \
  } while (0)

// origin of a device frame centred on n host points (3 doubles each)
static void host_origin(const double* xyz, size_t n, double origin[3]) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) {
      const double x = xyz[3 * i + k];
      if (x - x == 0.0) lo[k] = x < lo[k] ? x : lo[k], hi[k] = x > hi[k] ? x : hi[k];
    }
  choose_origin(lo, hi, origin);
}

template <typename T>
static int grow(sga_context* ctx, DevBuf<T>& buf, size_t used, size_t want) {
  if (buf.n >= want) return SGA_OK;
  DevBuf<T> bigger;
  SGA_TRY(bigger.alloc(want));
  if (used > 0) SGA_HIP(hipMemcpyAsync(bigger.p, buf.p, used * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the old block goes back to the allocator
  buf.swap(bigger);
  return SGA_OK;
}

static int rebuild_hash(sga_context* ctx, sga_index* idx, size_t n_target) {
  uint32_t hsize = 1024;
  while (hsize < 4 * n_target) hsize <<= 1;  // at most 1/4 full right after a rebuild, rebuilt again at 1/2
  if (idx->hkeys.n != hsize) {
    SGA_TRY(idx->hkeys.alloc(hsize));
    SGA_TRY(idx->hvals.alloc(hsize));
  }
  idx->hmask = hsize - 1;
  SGA_HIP(hipMemsetAsync(idx->hkeys.p, 0xff, hsize * sizeof(unsigned long long), ctx->stream));
  SGA_HIP(hipMemsetAsync(idx->hvals.p, 0, hsize * sizeof(uint32_t), ctx->stream));
  if (idx->n > 0) hipLaunchKernelGGL(ivm_rehash_kernel, dim3((idx->n + 255) / 256), dim3(256), 0, ctx->stream, static_cast<uint32_t>(idx->n), idx->vcoords.p, idx->hkeys.p, idx->hvals.p, idx->hmask);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// capacity of the per-voxel arrays and of the table for n_total voxels (the map holds idx->n): sga_voxelmap_insert's conditions
int ivm_reserve(sga_context* ctx, sga_index* idx, size_t n_total) {
  const size_t n_old = idx->n;
  if (n_total > idx->vcap) {
    const size_t cap = std::max<size_t>(2 * n_total, 1024);
    const bool flat = idx->kind == SGA_INDEX_FLATMAP;
    if (flat) {
      SGA_TRY(grow(ctx, idx->fpts64, 3 * kFlatCap * n_old, 3 * kFlatCap * cap));
      if (idx->has_normals) SGA_TRY(grow(ctx, idx->fnrm64, 3 * kFlatCap * n_old, 3 * kFlatCap * cap));
      if (idx->has_covs) SGA_TRY(grow(ctx, idx->fcov64, 6 * kFlatCap * n_old, 6 * kFlatCap * cap));
    } else {
      SGA_TRY(grow(ctx, idx->vmean64, 3 * n_old, 3 * cap));
      SGA_TRY(grow(ctx, idx->vcov64, 6 * n_old, 6 * cap));
    }
    SGA_TRY(grow(ctx, idx->vcounts, n_old, cap));
    SGA_TRY(grow(ctx, idx->vlru, n_old, cap));
    SGA_TRY(grow(ctx, idx->vcoords, 3 * n_old, 3 * cap));
    SGA_TRY(grow(ctx, idx->pts, 0, flat ? kFlatCap * cap : cap));
    if (flat && idx->has_normals) SGA_TRY(grow(ctx, idx->nrm, 0, kFlatCap * cap));
    if (!flat || idx->has_covs) SGA_TRY(grow(ctx, idx->cov, 0, flat ? kFlatCap * cap : cap));
    idx->vcap = cap;
  }
  if (idx->hkeys.n == 0 || 2 * n_total > idx->hkeys.n) SGA_TRY(rebuild_hash(ctx, idx, n_total));
  return SGA_OK;
}

// LRU sweep (incremental_voxelmap.hpp:76-88), when the counter (already incremented for this insert) says it is due
int ivm_lru_sweep(sga_context* ctx, sga_index* idx) {
  if (idx->lru_counter % idx->lru_clear_cycle == 0 && idx->n > 0) {
    const uint32_t nv = static_cast<uint32_t>(idx->n);
    DevBuf<uint32_t> keep, pos;
    SGA_TRY(keep.alloc(nv));
    SGA_TRY(pos.alloc(nv));
    hipLaunchKernelGGL(ivm_keep_kernel, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, nv, idx->vlru.p, idx->lru_horizon, idx->lru_counter, keep.p);
    SGA_TRY(exclusive_scan(ctx, keep.p, pos.p, nv));
    uint32_t last_keep = 0, last_pos = 0;
    SGA_HIP(hipMemcpyAsync(&last_keep, keep.p + (nv - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipMemcpyAsync(&last_pos, pos.p + (nv - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipStreamSynchronize(ctx->stream));
    const uint32_t kept = last_pos + last_keep;
    if (kept < nv) {
      DevBuf<double> m2, n2, c2;
      DevBuf<uint32_t> cnt2, lru2;
      DevBuf<int> co2;
      const bool flat = idx->kind == SGA_INDEX_FLATMAP;
      SGA_TRY(m2.alloc((flat ? 3 * kFlatCap : 3) * idx->vcap));
      if (flat && idx->has_normals) SGA_TRY(n2.alloc(3 * kFlatCap * idx->vcap));
      if (!flat || idx->has_covs) SGA_TRY(c2.alloc((flat ? 6 * kFlatCap : 6) * idx->vcap));
      SGA_TRY(cnt2.alloc(idx->vcap));
      SGA_TRY(lru2.alloc(idx->vcap));
      SGA_TRY(co2.alloc(3 * idx->vcap));
      if (flat)
        SGA_FLAT_DISPATCH(idx, fvm_compact_kernel, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, nv, keep.p, pos.p, idx->fpts64.p, idx->fnrm64.p, idx->fcov64.p, idx->vcounts.p, idx->vlru.p, idx->vcoords.p, m2.p, n2.p, c2.p,
                          cnt2.p, lru2.p, co2.p);
      else
        hipLaunchKernelGGL(ivm_compact_kernel, dim3((nv + 255) / 256), dim3(256), 0, ctx->stream, nv, keep.p, pos.p, idx->vmean64.p, idx->vcov64.p, idx->vcounts.p, idx->vlru.p, idx->vcoords.p, m2.p, c2.p, cnt2.p, lru2.p, co2.p);
      SGA_HIP(hipGetLastError());
      SGA_HIP(hipStreamSynchronize(ctx->stream));
      if (flat) {
        idx->fpts64.swap(m2);
        idx->fnrm64.swap(n2);
        idx->fcov64.swap(c2);
      } else {
        idx->vmean64.swap(m2);
        idx->vcov64.swap(c2);
      }
      idx->vcounts.swap(cnt2);
      idx->vlru.swap(lru2);
      idx->vcoords.swap(co2);
      idx->n = kept;
      SGA_TRY(rebuild_hash(ctx, idx, kept));
    }
  }
  return SGA_OK;
}

// `table1`: [members][ranges: 6 ints per member][counters: 2 per member][ticket][prefix of the key grid: count + 1]
int ivm_forest_enqueue_runs(sga_context* ctx, sga_index* const* maps, const sga_cloud* const* clouds, const double* T, const IvmForestPlan& plan, unsigned long long seq, VoxelForestChain& ch) {
  const size_t count = plan.forest.size();
  if (count == 0) return SGA_OK;
  TableLayout L;
  const auto s_members = L.add<IvmMember>(count);
  const auto s_range = L.add<int>(6 * count);
  const auto s_counters = L.add<unsigned>(2 * count);
  const auto s_ticket = L.add<unsigned>(1);
  const auto s_prefix = L.add_prefixes(1, count);
  const uint32_t n32 = static_cast<uint32_t>(plan.points);
  const IvmMember* d_members = nullptr;
  SGA_TRY(voxel_forest_runs(ctx, ch, plan.points, plan.member_bits, plan.end_bit, Chain::IvmInsert, [&]() -> int {
    SGA_TRY(ch.seg_vid.alloc(plan.points));
    std::vector<IvmMember> members(count);
    std::vector<uint32_t> prefix(count + 1, 0u);
    SGA_TRY(ch.table1.alloc(L.words()));
    uint32_t off = 0;
    for (size_t j = 0; j < count; j++) {
      const size_t k = plan.forest[j];
      const sga_cloud* c = clouds[k];
      const sga_index* idx = maps[k];
      IvmMember& g = members[j];
      std::memset(&g, 0, sizeof(g));
      g.pts = c->pts.p;
      g.T = insert_pose(T ? T + 16 * k : nullptr, c->origin);
      g.inv_leaf = 1.0 / idx->leaf;
      g.hkeys = idx->hkeys.p;
      g.hvals = idx->hvals.p;
      g.range = L.at(s_range, ch.table1.p) + 6 * j;
      g.counters = L.at(s_counters, ch.table1.p) + 2 * j;
      g.count_slot = forest_slot_dev(ctx, j);
      g.hmask = idx->n > 0 ? idx->hmask : 0u;
      g.n = static_cast<uint32_t>(c->n);
      g.off = off;
      off += g.n;
      prefix[j + 1] = prefix[j] + (g.n + 255u) / 256u;
    }
    count_launch(Chain::IvmInsert);
    SGA_TRY(upload_table(ctx, ch.table1.p, L.words(), [&](unsigned long long* host) {
      L.put(s_members, host, members.data());
      L.put(s_prefix, host, prefix.data());
      voxel_range_identity(L.at(s_range, host), count);
    }));
    d_members = L.at(s_members, ch.table1.p);
    count_launch(Chain::IvmInsert);
    hipLaunchKernelGGL(ivm_keys_forest_kernel, dim3(prefix[count]), dim3(256), 0, ctx->stream, d_members, L.at(s_prefix, ch.table1.p), static_cast<int>(count), ch.keys.p, ch.vals.p);
    SGA_HIP(hipGetLastError());
    return SGA_OK;
  }));
  const ForestBoxes hand{L.at(s_ticket, ch.table1.p), static_cast<unsigned>(count), ctx->h_forest_dev, seq};
  count_launch(Chain::IvmInsert);
  hipLaunchKernelGGL(ivm_starts_forest_kernel, dim3((n32 + 255u) / 256u), dim3(256), 0, ctx->stream, d_members, ch.keys_sorted.p, ch.flags.p, ch.seg_id.p, ch.order.p, n32, ch.seg_start.p, ch.seg_vid.p, ch.rank_keys.p, ch.seg_ids.p, hand);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// `table2`.  One sort of all runs of the chain under the rank key — the members' new voxels in creation order, member after member, then
// every existing voxel's run in run order — and the assign + update launch
int ivm_forest_enqueue_update(sga_context* ctx, const std::vector<IvmUpdate>& members, size_t runs, uint32_t total_new, size_t members_in_chain, VoxelForestChain& ch) {
  const size_t count = members.size();
  if (count == 0 || runs == 0) return SGA_OK;
  std::vector<uint32_t> prefix(count + 1, 0u);
  for (size_t j = 0; j < count; j++) prefix[j + 1] = prefix[j] + (members[j].nseg + 127u) / 128u;
  if (prefix[count] == 0) return SGA_OK;
  SGA_TRY(ch.rank_keys_sorted.alloc(runs));
  SGA_TRY(ch.seg_by_rank.alloc(runs));
  const uint32_t* d_prefix = nullptr;
  count_launch(Chain::IvmInsert);
  SGA_TRY(upload_entries(ctx, ch.table2, members, prefix, &d_prefix));
  int rank_member_bits = 0;  // member numbers 0 .. members_in_chain (the last one: the runs of existing voxels)
  while ((1ull << rank_member_bits) < members_in_chain + 1) rank_member_bits++;
  count_launch(Chain::IvmInsert);
  SGA_TRY(sort_pairs(ctx, ch.rank_keys.p, ch.rank_keys_sorted.p, ch.seg_ids.p, ch.seg_by_rank.p, runs, 0, static_cast<unsigned>(kVoxRankMemberShift + rank_member_bits)));
  count_launch(Chain::IvmInsert);
  hipLaunchKernelGGL(ivm_update_forest_kernel, dim3(prefix[count]), dim3(128), 0, ctx->stream, reinterpret_cast<const IvmUpdate*>(ch.table2.p), d_prefix, static_cast<int>(count),
                     total_new, ch.seg_by_rank.p, ch.seg_start.p, ch.seg_vid.p, ch.keys_sorted.p, ch.order.p);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// `table3`: the fp32 records of every map of the call in one launch
int ivm_forest_enqueue_export(sga_context* ctx, const std::vector<IvmExport>& maps, VoxelForestChain& ch) {
  const size_t count = maps.size();
  if (count == 0) return SGA_OK;
  std::vector<uint32_t> prefix(count + 1, 0u);
  for (size_t j = 0; j < count; j++) prefix[j + 1] = prefix[j] + (maps[j].n + 255u) / 256u;
  const uint32_t* d_prefix = nullptr;
  count_launch(Chain::IvmInsert);
  SGA_TRY(upload_entries(ctx, ch.table3, maps, prefix, &d_prefix));
  count_launch(Chain::IvmInsert);
  hipLaunchKernelGGL(ivm_export_forest_kernel, dim3(prefix[count]), dim3(256), 0, ctx->stream, reinterpret_cast<const IvmExport*>(ch.table3.p), d_prefix, static_cast<int>(count));
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}
}  // namespace sga

using namespace sga;

extern "C" {

int sga_voxelmap_create(sga_context* ctx, double leaf, sga_index** out) {
  if (!ctx || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (!(leaf > 0)) return fail(SGA_ERR_INVALID, "leaf size must be positive");
  *out = nullptr;
  std::unique_ptr<sga_index> idx(new sga_index);
  idx->kind = SGA_INDEX_VOXELMAP;
  idx->device = ctx->device;
  idx->leaf = leaf;
  idx->has_covs = true;
  idx->incremental = true;
  *out = idx.release();
  return SGA_OK;
}

// A Gaussian voxel map from voxels that already exist on the host: the reference's GaussianVoxelMap object itself (its flat_voxels in
// flat order: coord, mean, cov; ann/incremental_voxelmap.hpp:39-92, gaussian_voxelmap.hpp:15-60) handed over as it is, so that
// Registration<GICPFactor, ParallelReductionHIP>::align(voxelmap, source, voxelmap) (registration_helper.cpp:125-137) searches exactly the
// voxels the caller built, with the caller's voxel ids.
int sga_index_create_voxelmap_from_voxels(sga_context* ctx, double leaf, const int32_t* coords, const double* means3, const double* cov6, size_t n, sga_index** out) {
  if (!ctx || !out || (n > 0 && (!coords || !means3 || !cov6))) return fail(SGA_ERR_INVALID, "null argument");
  if (!(leaf > 0)) return fail(SGA_ERR_INVALID, "leaf size must be positive");
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many voxels");
  *out = nullptr;
  SGA_ENTER(ctx);
  std::unique_ptr<sga_index> idx(new sga_index);
  idx->kind = SGA_INDEX_VOXELMAP;
  idx->device = ctx->device;
  idx->leaf = leaf;
  idx->has_covs = true;
  idx->n = n;
  if (n > 0) {
    DevBuf<double> d_mean, d_cov;
    SGA_TRY(d_mean.alloc(3 * n));
    SGA_TRY(d_cov.alloc(6 * n));
    SGA_TRY(idx->vcoords.alloc(3 * n));
    SGA_TRY(idx->vcounts.alloc(n));
    SGA_TRY(idx->pts.alloc(n));
    SGA_TRY(idx->cov.alloc(n));
    SGA_HIP(hipMemcpyAsync(d_mean.p, means3, 3 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SGA_HIP(hipMemcpyAsync(d_cov.p, cov6, 6 * n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    SGA_HIP(hipMemcpyAsync(idx->vcoords.p, coords, 3 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SGA_HIP(hipMemsetAsync(idx->vcounts.p, 0, n * sizeof(uint32_t), ctx->stream));  // (the number of points behind a voxel is not part of what the registration reads)
    host_origin(means3, n, idx->origin);
    hipLaunchKernelGGL(ivm_export_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, static_cast<uint32_t>(n), d_mean.p, d_cov.p, idx->origin[0], idx->origin[1], idx->origin[2], idx->pts.p, idx->cov.p);
    SGA_HIP(hipGetLastError());
    SGA_TRY(rebuild_hash(ctx, idx.get(), n));
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the host buffers are the caller's
  } else {
    SGA_TRY(rebuild_hash(ctx, idx.get(), 0));
  }
  *out = idx.release();
  return SGA_OK;
}

// A flat voxel map from voxels that already exist on the host: the reference's IncrementalVoxelMap<FlatContainer*> object as it is
// (flat order; per voxel its points and, where the container keeps them, their normals and covariances: flat_container.hpp:21-58), 16 slots
// per voxel like sga_flatmap_download.  The scan-to-model target of Registration<GICPFactor | PointToPlaneICPFactor, ParallelReductionHIP>
// (odometry_benchmark_small_gicp_model_omp.cpp).  The contents follow the arrays given.
int sga_index_create_flatmap_from_voxels_contents(sga_context* ctx, double leaf, const int32_t* coords, const uint32_t* counts, const double* points3, const double* normals3, const double* cov6, int search_offsets, size_t n,
                                                   sga_index** out) {
  if (!ctx || !out || (n > 0 && (!coords || !counts || !points3))) return fail(SGA_ERR_INVALID, "null argument");
  if (!(leaf > 0)) return fail(SGA_ERR_INVALID, "leaf size must be positive");
  if (search_offsets != 1 && search_offsets != 7 && search_offsets != 27) return fail(SGA_ERR_INVALID, "search offsets must be 1, 7 or 27 (incremental_voxelmap.hpp:157-186)");
  if (n >= (1ull << 27)) return fail(SGA_ERR_INVALID, "too many voxels");
  for (size_t v = 0; v < n; v++)
    if (counts[v] > static_cast<uint32_t>(kFlatCap)) return fail(SGA_ERR_UNSUPPORTED, "voxel %zu holds %u points: at most %d per voxel (max_num_points_in_cell)", v, counts[v], kFlatCap);
  *out = nullptr;
  SGA_ENTER(ctx);
  std::unique_ptr<sga_index> idx(new sga_index);
  idx->kind = SGA_INDEX_FLATMAP;
  idx->device = ctx->device;
  idx->leaf = leaf;
  idx->has_normals = normals3 != nullptr;
  idx->has_covs = cov6 != nullptr;
  idx->search_offsets = search_offsets;
  idx->n = n;
  if (n > 0) {
    const size_t slots = n * kFlatCap;
    DevBuf<double> d_pts, d_nrm, d_cov;
    SGA_TRY(d_pts.alloc(3 * slots));
    SGA_TRY(idx->vcoords.alloc(3 * n));
    SGA_TRY(idx->vcounts.alloc(n));
    SGA_TRY(idx->pts.alloc(slots));
    SGA_HIP(hipMemcpyAsync(d_pts.p, points3, 3 * slots * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (normals3) {
      SGA_TRY(d_nrm.alloc(3 * slots));
      SGA_TRY(idx->nrm.alloc(slots));
      SGA_HIP(hipMemcpyAsync(d_nrm.p, normals3, 3 * slots * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    if (cov6) {
      SGA_TRY(d_cov.alloc(6 * slots));
      SGA_TRY(idx->cov.alloc(slots));
      SGA_HIP(hipMemcpyAsync(d_cov.p, cov6, 6 * slots * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    }
    SGA_HIP(hipMemcpyAsync(idx->vcoords.p, coords, 3 * n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    SGA_HIP(hipMemcpyAsync(idx->vcounts.p, counts, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    {  // the device frame: centred on the valid points
      double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (size_t v = 0; v < n; v++)
        for (uint32_t j = 0; j < counts[v]; j++)
          for (int k = 0; k < 3; k++) {
            const double x = points3[3 * (v * kFlatCap + j) + k];
            if (x - x == 0.0) lo[k] = x < lo[k] ? x : lo[k], hi[k] = x > hi[k] ? x : hi[k];
          }
      choose_origin(lo, hi, idx->origin);
    }
    SGA_FLAT_DISPATCH(idx, fvm_export_kernel, dim3((slots + 255) / 256), dim3(256), 0, ctx->stream, static_cast<uint32_t>(n), idx->vcounts.p, d_pts.p, d_nrm.p, d_cov.p, idx->origin[0], idx->origin[1], idx->origin[2], idx->pts.p,
                      idx->nrm.p, idx->cov.p);
    SGA_HIP(hipGetLastError());
    SGA_TRY(rebuild_hash(ctx, idx.get(), n));
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the host buffers are the caller's
  } else {
    SGA_TRY(rebuild_hash(ctx, idx.get(), 0));
  }
  *out = idx.release();
  return SGA_OK;
}

int sga_index_create_flatmap_from_voxels(sga_context* ctx, double leaf, const int32_t* coords, const uint32_t* counts, const double* points3, const double* cov6, int search_offsets, size_t n, sga_index** out) {
  return sga_index_create_flatmap_from_voxels_contents(ctx, leaf, coords, counts, points3, nullptr, cov6, search_offsets, n, out);
}

int sga_flatmap_create_contents(sga_context* ctx, double leaf, int contents, sga_index** out) {
  if (contents < 0 || contents > (SGA_FLAT_NORMALS | SGA_FLAT_COVS)) return fail(SGA_ERR_INVALID, "flat map contents must be a combination of SGA_FLAT_NORMALS and SGA_FLAT_COVS");
  SGA_TRY(sga_voxelmap_create(ctx, leaf, out));
  (*out)->kind = SGA_INDEX_FLATMAP;
  (*out)->has_normals = (contents & SGA_FLAT_NORMALS) != 0;
  (*out)->has_covs = (contents & SGA_FLAT_COVS) != 0;
  return SGA_OK;
}

int sga_flatmap_create(sga_context* ctx, double leaf, sga_index** out) { return sga_flatmap_create_contents(ctx, leaf, SGA_FLAT_COVS, out); }

int sga_flatmap_get_contents(const sga_index* index, int* contents) {
  if (!index || !contents) return fail(SGA_ERR_INVALID, "null argument");
  if (index->kind != SGA_INDEX_FLATMAP) return fail(SGA_ERR_INVALID, "not a flat voxel map");
  *contents = (index->has_normals ? SGA_FLAT_NORMALS : 0) | (index->has_covs ? SGA_FLAT_COVS : 0);
  return SGA_OK;
}

int sga_flatmap_set_setting(sga_index* index, double min_sq_dist_in_cell, uint32_t max_num_points_in_cell) {
  if (!index || index->kind != SGA_INDEX_FLATMAP) return fail(SGA_ERR_INVALID, "not a flat voxel map");
  if (max_num_points_in_cell == 0 || max_num_points_in_cell > static_cast<uint32_t>(kFlatCap)) return fail(SGA_ERR_INVALID, "max_num_points_in_cell must be in [1, %d]", kFlatCap);
  if (index->n > 0) return fail(SGA_ERR_INVALID, "the cell setting must be chosen before the first insert");
  index->flat_min_sq = min_sq_dist_in_cell;
  index->flat_max = max_num_points_in_cell;
  return SGA_OK;
}

int sga_voxelmap_set_search_offsets(sga_index* index, int num_offsets) {
  if (!index || (index->kind != SGA_INDEX_VOXELMAP && index->kind != SGA_INDEX_FLATMAP)) return fail(SGA_ERR_INVALID, "not a voxel map");
  if (num_offsets != 1 && num_offsets != 7 && num_offsets != 27) return fail(SGA_ERR_INVALID, "search offsets must be 1, 7 or 27");
  index->search_offsets = num_offsets;
  return SGA_OK;
}

// per voxel: coords (3 ints) and number of points; points (3 floats), normals (3 floats) and cov6 (6 floats) for kFlatCap slots per voxel.
// strict: a requested attribute the map does not keep is an error; otherwise (sga_flatmap_download, cov6 only) it comes back as zeros.
static int flatmap_download(sga_context* ctx, const sga_index* index, int32_t* coords, uint32_t* counts, float* points, float* normals, float* cov6, bool strict) {
  if (!ctx || !index) return fail(SGA_ERR_INVALID, "null argument");
  if (index->kind != SGA_INDEX_FLATMAP) return fail(SGA_ERR_INVALID, "not a flat voxel map");
  if (strict && normals && !index->has_normals) return fail(SGA_ERR_INVALID, "the flat map keeps no normals");
  if (strict && cov6 && !index->has_covs) return fail(SGA_ERR_INVALID, "the flat map keeps no covariances");
  const size_t n = index->n;
  if (n == 0) return SGA_OK;
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, index->ready));
  std::vector<float4> hp, hn;
  std::vector<Cov8> hc;
  if (points) {
    hp.resize(n * kFlatCap);
    SGA_HIP(hipMemcpyAsync(hp.data(), index->pts.p, hp.size() * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (normals) {
    hn.resize(n * kFlatCap);
    SGA_HIP(hipMemcpyAsync(hn.data(), index->nrm.p, hn.size() * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  }
  if (cov6 && index->has_covs) {
    hc.resize(n * kFlatCap);
    SGA_HIP(hipMemcpyAsync(hc.data(), index->cov.p, hc.size() * sizeof(Cov8), hipMemcpyDeviceToHost, ctx->stream));
  } else if (cov6) {
    hc.assign(n * kFlatCap, Cov8{});
  }
  if (coords) SGA_HIP(hipMemcpyAsync(coords, index->vcoords.p, n * 3 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  if (counts) SGA_HIP(hipMemcpyAsync(counts, index->vcounts.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < n * kFlatCap; i++) {
    if (points) {  // device frame -> the caller's (empty slots hold +inf and stay +inf)
      points[3 * i] = static_cast<float>(static_cast<double>(hp[i].x) + index->origin[0]);
      points[3 * i + 1] = static_cast<float>(static_cast<double>(hp[i].y) + index->origin[1]);
      points[3 * i + 2] = static_cast<float>(static_cast<double>(hp[i].z) + index->origin[2]);
    }
    if (normals) {  // (directions: no frame; the records of empty slots are undefined)
      normals[3 * i] = hn[i].x;
      normals[3 * i + 1] = hn[i].y;
      normals[3 * i + 2] = hn[i].z;
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

int sga_flatmap_download(sga_context* ctx, const sga_index* index, int32_t* coords, uint32_t* counts, float* points, float* cov6) { return flatmap_download(ctx, index, coords, counts, points, nullptr, cov6, false); }

int sga_flatmap_download_contents(sga_context* ctx, const sga_index* index, int32_t* coords, uint32_t* counts, float* points, float* normals, float* cov6) {
  return flatmap_download(ctx, index, coords, counts, points, normals, cov6, true);
}

int sga_voxelmap_set_lru(sga_index* index, uint32_t horizon, uint32_t clear_cycle) {
  if (!index || !index->incremental) return fail(SGA_ERR_INVALID, "not an incremental voxel map");
  if (clear_cycle == 0) return fail(SGA_ERR_INVALID, "clear_cycle must be positive");
  index->lru_horizon = horizon;
  index->lru_clear_cycle = clear_cycle;
  return SGA_OK;
}

int sga_voxelmap_insert(sga_context* ctx, sga_index* idx, const sga_cloud* cloud, const double T16[16]) {
  if (!ctx || !idx || !cloud) return fail(SGA_ERR_INVALID, "null argument");
  if (!idx->incremental) return fail(SGA_ERR_INVALID, "not an incremental voxel map (create it with sga_voxelmap_create)");
  if (idx->kind != SGA_INDEX_FLATMAP || idx->has_covs) {
    if (cloud->n > 0 && !cloud->has_covs) return fail(SGA_ERR_INVALID, "GaussianVoxelMap needs point covariances");
  }
  if (idx->kind == SGA_INDEX_FLATMAP && idx->has_normals && cloud->n > 0 && !cloud->has_normals) return fail(SGA_ERR_INVALID, "a flat voxel map with normals needs point normals");
  if (cloud->device != ctx->device || idx->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud / map live on another device");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, cloud->ready));
  SGA_TRY(wait_ready(ctx, idx->ready));
  // The cloud's records live in its device frame (p' = p - o_c, common.hpp); the map's fp64 state, voxel coordinates and hash keys are the
  // CALLER's frame, exactly the reference's doubles: the kernels move a record by R p' + (R o_c + t).
  const Pose12 T = insert_pose(T16, cloud->origin);
  // The fp32 records the factor kernels read are re-exported after every insert anyway: their device frame follows the inserted scan (the
  // moved origin of the cloud's frame, quantised), so a map that walks kilometres (scan-to-model odometry) keeps sub-millimetre records.
  // (the new origin is committed only where the records are exported below — an insert that fails on the way leaves the map's
  // fp32 records AND the origin they are relative to as they were)
  double new_origin[3];
  map_origin_after_insert(T, cloud->n, 1.0 / idx->leaf, idx->origin, new_origin);
  const size_t n = cloud->n;
  const uint32_t n_old = static_cast<uint32_t>(idx->n);
  if (n > 0) {
    DevBuf<unsigned long long> keys, keys_sorted;
    DevBuf<uint32_t> vals, order, flags, seg_id;
    DevBuf<unsigned int> d_new;
    SGA_TRY(keys.alloc(n));
    SGA_TRY(keys_sorted.alloc(n));
    SGA_TRY(vals.alloc(n));
    SGA_TRY(order.alloc(n));
    SGA_TRY(flags.alloc(n));
    SGA_TRY(seg_id.alloc(n));
    SGA_TRY(d_new.alloc(1));
    const dim3 grid((n + 255) / 256), block(256);
    hipLaunchKernelGGL(ivm_keys_kernel, grid, block, 0, ctx->stream, cloud->pts.p, n, T, 1.0 / idx->leaf, keys.p, vals.p);
    size_t tb = 0;
    SGA_HIP(rocprim::radix_sort_pairs(nullptr, tb, keys.p, keys_sorted.p, vals.p, order.p, n, 0, 64, ctx->stream));
    SGA_TRY(ensure_temp(ctx, tb));
    SGA_HIP(rocprim::radix_sort_pairs(ctx->d_temp.p, tb, keys.p, keys_sorted.p, vals.p, order.p, n, 0, 64, ctx->stream));
    segment_heads(ctx, keys_sorted.p, n, flags.p);
    SGA_TRY(exclusive_scan(ctx, flags.p, seg_id.p, n));
    uint32_t last_flag = 0, last_seg = 0;
    SGA_HIP(hipMemcpyAsync(&last_flag, flags.p + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipMemcpyAsync(&last_seg, seg_id.p + (n - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
    SGA_HIP(hipStreamSynchronize(ctx->stream));
    const uint32_t nseg = last_seg + last_flag;
    if (nseg > 0) {
      DevBuf<uint32_t> seg_start, seg_first, seg_vid, rank_key, rank_sorted, seg_ids, seg_by_rank;
      SGA_TRY(seg_start.alloc(nseg));
      SGA_TRY(seg_first.alloc(nseg));
      SGA_TRY(seg_vid.alloc(nseg));
      SGA_TRY(rank_key.alloc(nseg));
      SGA_TRY(rank_sorted.alloc(nseg));
      SGA_TRY(seg_ids.alloc(nseg));
      SGA_TRY(seg_by_rank.alloc(nseg));
      const dim3 sgrid((nseg + 255) / 256);
      hipLaunchKernelGGL(ivm_segments_kernel, grid, block, 0, ctx->stream, flags.p, seg_id.p, order.p, n, seg_start.p, seg_first.p);
      SGA_HIP(hipMemsetAsync(d_new.p, 0, sizeof(unsigned int), ctx->stream));
      hipLaunchKernelGGL(ivm_lookup_kernel, sgrid, block, 0, ctx->stream, nseg, seg_start.p, seg_first.p, keys_sorted.p, idx->hkeys.p, idx->hvals.p, n_old > 0 ? idx->hmask : 0u, seg_vid.p, rank_key.p, seg_ids.p, d_new.p);
      size_t tb3 = 0;
      SGA_HIP(rocprim::radix_sort_pairs(nullptr, tb3, rank_key.p, rank_sorted.p, seg_ids.p, seg_by_rank.p, nseg, 0, 32, ctx->stream));
      SGA_TRY(ensure_temp(ctx, tb3));
      SGA_HIP(rocprim::radix_sort_pairs(ctx->d_temp.p, tb3, rank_key.p, rank_sorted.p, seg_ids.p, seg_by_rank.p, nseg, 0, 32, ctx->stream));
      unsigned int n_new = 0;
      SGA_HIP(hipMemcpyAsync(&n_new, d_new.p, sizeof(n_new), hipMemcpyDeviceToHost, ctx->stream));
      SGA_HIP(hipStreamSynchronize(ctx->stream));
      const size_t n_total = static_cast<size_t>(n_old) + n_new;
      if (n_total >= (1ull << 31)) return fail(SGA_ERR_INVALID, "voxel map too large");
      SGA_TRY(ivm_reserve(ctx, idx, n_total));
      if (n_new > 0) hipLaunchKernelGGL(ivm_assign_kernel, dim3((n_new + 255) / 256), block, 0, ctx->stream, n_new, seg_by_rank.p, n_old, seg_vid.p);
      if (idx->kind == SGA_INDEX_FLATMAP)
        SGA_FLAT_DISPATCH(idx, fvm_update_kernel, sgrid, block, 0, ctx->stream, nseg, seg_start.p, seg_vid.p, static_cast<uint32_t>(n), keys_sorted.p, order.p, cloud->pts.p, cloud->nrm.p, cloud->cov.p, T, n_old,
                          idx->lru_counter, idx->flat_max, idx->flat_min_sq, idx->fpts64.p, idx->fnrm64.p, idx->fcov64.p, idx->vcounts.p, idx->vlru.p, idx->vcoords.p, idx->hkeys.p, idx->hvals.p, idx->hmask);
      else
        hipLaunchKernelGGL(
          ivm_update_kernel, sgrid, block, 0, ctx->stream, nseg, seg_start.p, seg_vid.p, static_cast<uint32_t>(n), keys_sorted.p, order.p, cloud->pts.p, cloud->cov.p, T, n_old, idx->lru_counter, idx->vmean64.p, idx->vcov64.p,
          idx->vcounts.p, idx->vlru.p, idx->vcoords.p, idx->hkeys.p, idx->hvals.p, idx->hmask);
      SGA_HIP(hipGetLastError());
      idx->n = n_total;
    }
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the scratch buffers of this insert are released below
  }
  // LRU sweep (incremental_voxelmap.hpp:76-88)
  idx->lru_counter++;
  SGA_TRY(ivm_lru_sweep(ctx, idx));
  for (int k = 0; k < 3; k++) idx->origin[k] = new_origin[k];  // every fallible step is behind us: the records exported now are relative to it
  if (idx->n > 0) {
    if (idx->kind == SGA_INDEX_FLATMAP)
      SGA_FLAT_DISPATCH(idx, fvm_export_kernel, dim3((idx->n * kFlatCap + 255) / 256), dim3(256), 0, ctx->stream, static_cast<uint32_t>(idx->n), idx->vcounts.p, idx->fpts64.p, idx->fnrm64.p, idx->fcov64.p, idx->origin[0],
                        idx->origin[1], idx->origin[2], idx->pts.p, idx->nrm.p, idx->cov.p);
    else
      hipLaunchKernelGGL(ivm_export_kernel, dim3((idx->n + 255) / 256), dim3(256), 0, ctx->stream, static_cast<uint32_t>(idx->n), idx->vmean64.p, idx->vcov64.p, idx->origin[0], idx->origin[1], idx->origin[2], idx->pts.p, idx->cov.p);
  }
  SGA_HIP(hipGetLastError());
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

}  // extern "C"

// Clustering on the device: sga_cloud_cluster — DBSCAN with a deterministic border rule over the fixed-radius
// walk of kd_radius.hpp.  Core flags, a lock-free union of the core points in a 32-bit parent array, the roots, the border points'
// nearest core point, sizes and boxes by integer atomics at the root's slot, the selection and numbering by one workgroup, the labels,
// and the crop's stable compaction (cloud_crop.hip: cloud_crop_stat) when a cloud is asked for.  Everything is in cloud indices.  One
// host wait; no floating-point atomic, no spin, no grid barrier.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "kd_radius.hpp"
#include "notes.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kCluBlock = 64;       // walk kernels: points of a workgroup, one lane each, one wave
constexpr int kCluFlatBlock = 256;  // the kernels that do not walk
constexpr uint32_t kCluNone = 0xffffffffu;

// What the kernels receive (kernel arguments: read with scalar loads)
struct ClusterArgs {
  KdView g;             // the tree over the cloud
  const float4* pts;    // the cloud's records, its order
  double radius;
  double ox, oy, oz;    // the cloud's origin
  uint32_t n;
  uint32_t min_points;
  uint32_t min_size, max_size;  // max_size: 0xffffffff = no limit
  uint32_t* core;       // n: 1 = core point
  uint32_t* parent;     // n: the union's forest, parent[v] <= v
  uint32_t* root;       // n: the root of the point's cluster, kCluNone for noise
  uint32_t* size;       // n: members, at the root's slot
  int* box;             // 6 n: min x y z, max x y z of the members' records (box_enc), at the root's slot
  int* number;          // n: at a root's slot the cluster's number, -1 for a dropped one
  unsigned long long* counts_host;  // {clusters kept, noise points, points of dropped clusters, rows written}: a slot of the staging ring
  sga_cluster_row* rows_host;       // table_capacity rows behind them
  int* labels_host;                 // n labels behind those; or null
  double* flag;         // n, or null: 0.0 where the compaction keeps the point, 1.0 where it does not (held against 0.5)
  uint32_t table_capacity;
  int keep;
};

// ---- the union ------------------------------------------------------------------------------------------------------------------------------
// parent[] is a forest over the core points with parent[v] <= v; a root has parent[v] == v.  Links are only ever made by
// atomicCAS(&parent[hi], hi, lo) with lo < hi, so a slot changes at most ONCE in the hook kernel, from v to something smaller, and every
// link joins two points the graph connects.  No path is compressed there.
//
// The per-XCD L2s are not coherent, so a load of parent[v] may return an OLDER value of the slot — which can only be v itself (the slot's
// one earlier value).  The argument does not need fresh loads:
//   * cluster_find follows parent[] with relaxed agent-scope loads until it meets p == v.  Every step strictly descends, so it ends; what
//     it returns is an ancestor-or-self of its argument: the true root, or, after a stale read, a point that has been linked further.
//   * cluster_unite finds both ends, returns when they meet, and otherwise tries the CAS on the larger.  The CAS at agent scope is the
//     only decider: it succeeds iff hi is a root at that instant, and then the two trees are one.  When it fails it returns the slot's
//     current value — an ancestor of hi, smaller than hi — and the loop CONTINUES FROM THAT VALUE, never from a re-read.  (a, b) is
//     replaced by a pair in the same two trees whose larger member has strictly decreased; indices are bounded below, so the loop ends.
//   * No step waits for another lane's write: a lane that loses a CAS has been handed the winner's link and moves on.
// The flatten runs in a later kernel and reads settled values.  Returns the smaller end, a point of the merged tree: the caller's next
// unite may start from it.
__device__ __forceinline__ uint32_t cluster_find(uint32_t* parent, uint32_t v) {
  for (;;) {
    const uint32_t p = __hip_atomic_load(&parent[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == v) return v;
    v = p;
  }
}
__device__ __forceinline__ uint32_t cluster_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cluster_find(parent, a);
    b = cluster_find(parent, b);
    if (a == b) return a;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = atomicCAS(&parent[hi], hi, lo);
    if (old == hi) return lo;
    a = old;  // parent[hi] as the CAS saw it: < hi
    b = lo;
  }
}

}  // namespace

// parent = identity, sizes zero, boxes empty, and, without a count pass, every point core
__global__ __launch_bounds__(kCluFlatBlock) void cluster_init_kernel(const ClusterArgs a) {
  const uint32_t v = blockIdx.x * static_cast<uint32_t>(kCluFlatBlock) + threadIdx.x;
  if (v >= a.n) return;
  a.parent[v] = v;
  a.size[v] = 0u;
  if (a.min_points <= 1u) a.core[v] = 1u;
#pragma unroll
  for (int k = 0; k < 6; k++) a.box[6ull * v + k] = k < 3 ? 0x7fffffff : static_cast<int>(0x80000000u);
}

// The three passes that walk; lane i of the grid owns the record at kd position i (neighbouring lanes walk neighbouring paths) and acts
// for the cloud index in its w.
//   PASS 0 count:  core[i] = at least min_points records within the radius, the point included
//   PASS 1 hook:   a core point i is united with every core neighbour j < i
//   PASS 2 border: a non-core point takes the root of its nearest core neighbour — (d2 in double, then the lower index) — or none
template <int PASS>
__global__ __launch_bounds__(kCluBlock) void cluster_walk_kernel(const ClusterArgs a) {
  extern __shared__ uint32_t clu_stack[];  // [kKdMaxDepth][kCluBlock] words
  const int lane = threadIdx.x;
  const uint32_t pos = blockIdx.x * static_cast<uint32_t>(kCluBlock) + lane;
  if (pos >= a.n) return;  // (the walk has no wave-level step)
  const float4 p = a.g.pts[pos];
  const uint32_t i = __float_as_uint(p.w);
  const double qx = p.x, qy = p.y, qz = p.z;
  if constexpr (PASS == 0) {
    uint32_t c = 0;
    auto add = [&](uint32_t, double) { c++; };
    kd_radius_walk<kCluBlock>(a.g, qx, qy, qz, a.radius, clu_stack, lane, add);
    a.core[i] = c >= a.min_points ? 1u : 0u;
  } else if constexpr (PASS == 1) {
    if (a.core[i] == 0u) return;
    uint32_t mine = i;  // a point of i's tree: where the next find starts
    auto hook = [&](uint32_t j, double) {
      if (j < i && a.core[j] != 0u) mine = cluster_unite(a.parent, mine, j);
    };
    kd_radius_walk<kCluBlock>(a.g, qx, qy, qz, a.radius, clu_stack, lane, hook);
  } else {
    if (a.core[i] != 0u) return;
    double best = static_cast<double>(INFINITY);
    uint32_t who = kCluNone;
    auto nearest = [&](uint32_t j, double d2) {
      if (a.core[j] != 0u && (d2 < best || (d2 == best && j < who))) best = d2, who = j;
    };
    kd_radius_walk<kCluBlock>(a.g, qx, qy, qz, a.radius, clu_stack, lane, nearest);
    a.root[i] = who != kCluNone ? a.root[who] : kCluNone;  // (root[] of a core point: the flatten kernel's, never written here)
  }
}

// the root of every core point; none for the others (the border pass fills in its own)
__global__ __launch_bounds__(kCluFlatBlock) void cluster_flatten_kernel(const ClusterArgs a) {
  const uint32_t v = blockIdx.x * static_cast<uint32_t>(kCluFlatBlock) + threadIdx.x;
  if (v >= a.n) return;
  a.root[v] = a.core[v] != 0u ? cluster_find(a.parent, v) : kCluNone;
}

// every member adds itself to its root's size and box: integer atomics only (the box on the order-preserving image of the coordinates)
__global__ __launch_bounds__(kCluFlatBlock) void cluster_sizes_kernel(const ClusterArgs a) {
  const uint32_t v = blockIdx.x * static_cast<uint32_t>(kCluFlatBlock) + threadIdx.x;
  if (v >= a.n) return;
  const uint32_t r = a.root[v];
  if (r == kCluNone) return;
  const float4 p = a.pts[v];
  atomicAdd(&a.size[r], 1u);
  int* b = a.box + 6ull * r;
  atomicMin(&b[0], box_enc(p.x)), atomicMin(&b[1], box_enc(p.y)), atomicMin(&b[2], box_enc(p.z));
  atomicMax(&b[3], box_enc(p.x)), atomicMax(&b[4], box_enc(p.y)), atomicMax(&b[5], box_enc(p.z));
}

// The roots whose size passes are numbered in index order — a root is its cluster's lowest core index, its seed — by ONE workgroup
// (kd_radius.hpp: one_block_prefix); their rows and the call's counts go to the slot.  noise = n - members of all clusters.
__global__ __launch_bounds__(kRadScanThreads) void cluster_select_kernel(const ClusterArgs a) {
  __shared__ unsigned long long sh[kRadScanThreads];
  uint32_t first, end;
  auto is_root = [&](uint32_t v) { return a.root[v] == v; };  // (only core points are roots; a border point's root is another point)
  auto passes = [&](uint32_t v) { return a.size[v] >= a.min_size && a.size[v] <= a.max_size; };
  unsigned long long clusters, members, dropped;
  (void)one_block_prefix(a.n, first, end, sh, members, [&](uint32_t v) { return is_root(v) ? static_cast<unsigned long long>(a.size[v]) : 0ull; });
  (void)one_block_prefix(a.n, first, end, sh, dropped, [&](uint32_t v) { return is_root(v) && !passes(v) ? static_cast<unsigned long long>(a.size[v]) : 0ull; });
  unsigned long long at = one_block_prefix(a.n, first, end, sh, clusters, [&](uint32_t v) { return is_root(v) && passes(v) ? 1ull : 0ull; });
  for (uint32_t v = first; v < end; v++) {
    if (!is_root(v)) continue;
    if (!passes(v)) {
      a.number[v] = -1;
      continue;
    }
    a.number[v] = static_cast<int>(at);
    if (at < a.table_capacity) {
      sga_cluster_row row;
      row.seed = v;
      row.size = a.size[v];
      const int* b = a.box + 6ull * v;
      row.lo[0] = static_cast<double>(box_dec(b[0])) + a.ox, row.lo[1] = static_cast<double>(box_dec(b[1])) + a.oy, row.lo[2] = static_cast<double>(box_dec(b[2])) + a.oz;
      row.hi[0] = static_cast<double>(box_dec(b[3])) + a.ox, row.hi[1] = static_cast<double>(box_dec(b[4])) + a.oy, row.hi[2] = static_cast<double>(box_dec(b[5])) + a.oz;
      a.rows_host[at] = row;
    }
    at++;
  }
  if (threadIdx.x == 0) {
    a.counts_host[0] = clusters;
    a.counts_host[1] = a.n - members;
    a.counts_host[2] = dropped;
    a.counts_host[3] = clusters < a.table_capacity ? clusters : a.table_capacity;
  }
  __threadfence_system();
}

// the label of every point, and what the compaction reads
__global__ __launch_bounds__(kCluFlatBlock) void cluster_labels_kernel(const ClusterArgs a) {
  const uint32_t v = blockIdx.x * static_cast<uint32_t>(kCluFlatBlock) + threadIdx.x;
  if (v >= a.n) return;
  const uint32_t r = a.root[v];
  const int label = r != kCluNone ? a.number[r] : -1;
  if (a.flag != nullptr) a.flag[v] = (label >= 0) == (a.keep == 1) ? 0.0 : 1.0;
  if (a.labels_host != nullptr) {
    a.labels_host[v] = label;
    __threadfence_system();
  }
}

namespace {

// what sga_cloud_cluster refuses of its arguments (no handle is read)
int cluster_check(const sga_cluster_params& p, const sga_cluster_row* table, size_t table_capacity, const int64_t* kept, sga_cloud* const* out) {
  if (p.keep < 0 || p.keep > 2) return fail(SGA_ERR_INVALID, "cluster: keep %d is not 0 (no cloud), 1 (the clustered) or 2 (the rest)", p.keep);
  if (p.keep == 0 && out != nullptr) return fail(SGA_ERR_INVALID, "cluster: keep is 0 but an output cloud is asked for");
  if (p.keep != 0 && out == nullptr) return fail(SGA_ERR_INVALID, "cluster: keep is %d but there is no place for the output cloud", p.keep);
  if (p.keep == 0 && kept != nullptr) return fail(SGA_ERR_INVALID, "cluster: kept is given but keep is 0");
  if ((table == nullptr) != (table_capacity == 0)) return fail(SGA_ERR_INVALID, "cluster: a table needs a capacity and a capacity a table");
  if (table_capacity >= (1ull << 31)) return fail(SGA_ERR_INVALID, "cluster: table capacity %zu is beyond 2^31-1", table_capacity);
  if (!(p.radius - p.radius == 0.0 && p.radius > 0.0)) return fail(SGA_ERR_INVALID, "cluster: radius must be finite and > 0");
  if (p.min_points < 1) return fail(SGA_ERR_INVALID, "cluster: min_points %d is below 1", p.min_points);
  if (p.min_size < 1) return fail(SGA_ERR_INVALID, "cluster: min_size %lld is below 1", static_cast<long long>(p.min_size));
  if (p.max_size < 0) return fail(SGA_ERR_INVALID, "cluster: max_size %lld is negative (0: no limit)", static_cast<long long>(p.max_size));
  if (p.max_size > 0 && p.min_size > p.max_size) return fail(SGA_ERR_INVALID, "cluster: min_size %lld is above max_size %lld", static_cast<long long>(p.min_size), static_cast<long long>(p.max_size));
  return SGA_OK;
}

struct IndexDestroy {
  void operator()(sga_index* i) const { (void)sga_index_destroy(i); }
};

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_cluster_params_default(sga_cluster_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->radius = 0.5;
  p->min_points = 1;
  p->min_size = 1;
}

int sga_cloud_cluster(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree, const sga_cluster_params* params, int32_t* labels, sga_cluster_row* table, size_t table_capacity, int64_t* kept, sga_cluster_result* result,
                      sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !cloud || !params) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(cluster_check(*params, table, table_capacity, kept, out));
  // ---- (from here on the handles are read)
  if (result) std::memset(result, 0, sizeof(*result));
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (kdtree) {  // checked as sga_cloud_remove_outliers checks it
    if (kdtree->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "clustering needs a kd-tree index, not a projective search");
    if (kdtree->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_INVALID, "a kd-tree index is required");
    if (kdtree->device != ctx->device) return fail(SGA_ERR_INVALID, "index lives on another device");
    if (kdtree->n != n) return fail(SGA_ERR_INVALID, "index was built over a cloud of %zu points, got %zu", kdtree->n, n);
    for (int a = 0; a < 3; a++)
      if (kdtree->origin[a] != cloud->origin[a]) return fail(SGA_ERR_INVALID, "the index was not built over this cloud (their device frames differ)");
  }
  CropStat cs{nullptr, nullptr, 0.5, Chain::Cluster};
  if (n == 0) return out ? cloud_crop_stat(ctx, cloud, cs, kept, out) : SGA_OK;  // an empty cloud, zero clusters; nothing is launched
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
    SGA_TRY(wait_ready(ctx, index->ready));
  }
  SGA_TRY(wait_ready(ctx, cloud->ready));
  // core, parent, root, size, number (n words each) and the boxes (6 n) in one block; the compaction's flags beside it
  DevBuf<uint32_t> words;
  DevBuf<double> flag;
  SGA_TRY(words.alloc(11 * n));
  if (out) SGA_TRY(flag.alloc(n));
  // the counts, the rows and the labels leave through ONE slot of the staging ring, which the kernels write by its device address
  const size_t rows_bytes = table_capacity * sizeof(sga_cluster_row);
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, 32 + rows_bytes + (labels != nullptr ? n * sizeof(int32_t) : 0), &slot));
  char* slot_dev = static_cast<char*>(slot->dev);
  ClusterArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = make_kd_view(index);
  a.pts = cloud->pts.p;
  a.radius = params->radius;
  a.ox = cloud->origin[0], a.oy = cloud->origin[1], a.oz = cloud->origin[2];
  a.n = static_cast<uint32_t>(n);
  a.min_points = static_cast<uint32_t>(params->min_points);
  a.min_size = static_cast<uint32_t>(params->min_size < (1ll << 32) ? params->min_size : 0xffffffffll);
  a.max_size = params->max_size > 0 && params->max_size < 0xffffffffll ? static_cast<uint32_t>(params->max_size) : 0xffffffffu;
  a.core = words.p;
  a.parent = words.p + n;
  a.root = words.p + 2 * n;
  a.size = words.p + 3 * n;
  a.number = reinterpret_cast<int*>(words.p + 4 * n);
  a.box = reinterpret_cast<int*>(words.p + 5 * n);
  a.counts_host = reinterpret_cast<unsigned long long*>(slot_dev);
  a.rows_host = reinterpret_cast<sga_cluster_row*>(slot_dev + 32);
  a.labels_host = labels != nullptr ? reinterpret_cast<int*>(slot_dev + 32 + rows_bytes) : nullptr;
  a.flag = flag.p;
  a.table_capacity = static_cast<uint32_t>(table_capacity);
  a.keep = params->keep;
  const dim3 flat(static_cast<unsigned>((n + kCluFlatBlock - 1) / kCluFlatBlock)), walk(static_cast<unsigned>((n + kCluBlock - 1) / kCluBlock));
  const size_t stack_bytes = static_cast<size_t>(kKdMaxDepth) * 4 * kCluBlock;
  const bool density = a.min_points > 1u;  // else every point is core: no count pass, no border pass
  count_launch(Chain::Cluster);
  hipLaunchKernelGGL(cluster_init_kernel, flat, dim3(kCluFlatBlock), 0, ctx->stream, a);
  if (density) {
    count_launch(Chain::Cluster);
    hipLaunchKernelGGL((cluster_walk_kernel<0>), walk, dim3(kCluBlock), stack_bytes, ctx->stream, a);
  }
  count_launch(Chain::Cluster);
  hipLaunchKernelGGL((cluster_walk_kernel<1>), walk, dim3(kCluBlock), stack_bytes, ctx->stream, a);
  count_launch(Chain::Cluster);
  hipLaunchKernelGGL(cluster_flatten_kernel, flat, dim3(kCluFlatBlock), 0, ctx->stream, a);
  if (density) {
    count_launch(Chain::Cluster);
    hipLaunchKernelGGL((cluster_walk_kernel<2>), walk, dim3(kCluBlock), stack_bytes, ctx->stream, a);
  }
  count_launch(Chain::Cluster);
  hipLaunchKernelGGL(cluster_sizes_kernel, flat, dim3(kCluFlatBlock), 0, ctx->stream, a);
  count_launch(Chain::Cluster);
  hipLaunchKernelGGL(cluster_select_kernel, dim3(1), dim3(kRadScanThreads), 0, ctx->stream, a);
  count_launch(Chain::Cluster);
  hipLaunchKernelGGL(cluster_labels_kernel, flat, dim3(kCluFlatBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  sga_cloud* made = nullptr;
  count_launch(Chain::RadiusWait);
  if (out) {
    cs.d = a.flag;
    SGA_TRY(cloud_crop_stat(ctx, cloud, cs, kept, &made));  // (its wait shows that everything above has run)
  } else {
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait
  }
  const char* host = static_cast<const char*>(slot->host);
  const unsigned long long* counts = reinterpret_cast<const unsigned long long*>(host);
  if (result) {
    result->clusters = counts[0];
    result->noise = counts[1];
    result->dropped = counts[2];
    result->rows = counts[3];
  }
  if (table) std::memcpy(table, host + 32, static_cast<size_t>(counts[3]) * sizeof(sga_cluster_row));
  if (labels) std::memcpy(labels, host + 32 + rows_bytes, n * sizeof(int32_t));
  if (out) *out = made;
  return SGA_OK;
}

int sga_debug_cloud_cluster_launches(unsigned long long* launches) { return report_launches(Chain::Cluster, launches); }

}  // extern "C"

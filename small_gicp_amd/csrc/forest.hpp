// The batched chains: one call serves B members through one chain of launches and one host wait.  Shared here:
//   * the table: laid out once (forest_table.hpp), filled in a zeroed slot of the pinned staging ring and copied to the device with one
//     command (upload_table: the only way a table reaches the device); the batched kernels — beside the lone kernels whose bodies they
//     share — read what the lone kernel receives as its arguments from their member's entry, with scalar loads (uniform_const);
//   * the box block: pinned, device-mapped words of the context; word 0 receives the call's sequence number once every member has
//     written its slot (forest_slot_dev / forest_slot_host, the kSlot constants);
//   * the call (forest_call_begin, the chain's enqueue, forest_call_wait: the ONE host wait) and the launch counters (Chain).
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"
#include "device_math.hpp"
#include "forest_table.hpp"
#include "kd_search.hpp"
#include "uniform.hpp"

namespace sga {

// One tree of a forest build: the arguments of kd_split_level_kernel / kd_finish_kernel / kd_tail_kernel / kd_boxes_kernel for it.
// Level d of the build reads perm[(d + 1) & 1] (level 0: the identity) and writes perm[d & 1]; the finish kernel is level dA.
struct ForestTree {
  const float4* pts;   // the cloud
  const float4* nrm;   // its attributes, or null
  const Cov8* cov;
  uint32_t* perm[2];
  float2* nodes;
  float4* opts;        // the index's arrays (kd_tail_kernel)
  float4* onrm;
  Cov8* ocov;
  float4* boxes;
  float4* groups;
  float* blocks;
  float4* pairs;
  unsigned long long* spacing_acc;  // {sum, leaves counted, arrival counter, 0} of this tree's tail launch; zero between launches
  unsigned long long* late_slot;    // the late note that carries the tree's length scale (notes.hpp), or null
  unsigned long long late_seq;
  unsigned long long* box_slot;     // words 1..3 receive the cloud's bounding box (pinned, device-mapped: the call's box block)
  uint32_t n;
  int D, dA;  // depth; first level finished in LDS (index_build.hip: build_kdtree)
};

// The hand-off of the boxes: every tree's root level writes its box, the last to arrive publishes the call's sequence number
struct ForestBoxes {
  unsigned* ticket;               // arrivals of the trees' root levels (device memory, zero when the call starts)
  unsigned total;                 // trees of the forest
  unsigned long long* seq_word;   // in the box block
  unsigned long long seq;
};

// by ONE thread of a member (a tree's root level, a grid's last tile), after it wrote the member's words of the box block: the last member
// to arrive publishes the call's sequence number (agent-scope ticket, system-scope release: batch_reduce_rows_kernel's hand-off, reduce_rows.hpp)
__device__ __forceinline__ void forest_box_arrive(const ForestBoxes& h) {
  __threadfence_system();
  if (__hip_atomic_fetch_add(h.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == h.total - 1u) {
    __threadfence_system();
    __hip_atomic_store(h.seq_word, h.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// One member of a batched covariance / normal estimation: the arguments of knn_wave_kernel / features_from_list_kernel for it
struct ForestFeat {
  KdView g;
  int* nbr;
  float4* idx_nrm;
  Cov8* idx_cov;
  float4* cloud_nrm;
  Cov8* cloud_cov;
  double ox, oy, oz;
};

// the member that owns workgroup b: prefix[k] <= b < prefix[k + 1] (wave-uniform binary search, as batch_search_linearize_kernel's)
__device__ __forceinline__ int forest_member_of(const uint32_t* prefix, int count, uint32_t b) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// A call's table on its way to the device: a slot of the staging ring is acquired and zeroed, `fill` writes what is not zero of the
// table's `words` 8-byte words, ONE copy command carries them to `dst`, the slot is released behind it.  (Counts nothing: Chain.)
template <typename Fill>
int upload_table(sga_context* ctx, unsigned long long* dst, size_t words, Fill&& fill) {
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, words * 8, &slot));
  unsigned long long* host = static_cast<unsigned long long*>(slot->host);
  std::memset(host, 0, words * 8);
  fill(host);
  SGA_HIP(hipMemcpyAsync(dst, host, words * 8, hipMemcpyHostToDevice, ctx->stream));
  return stage_release(ctx, slot);
}
// The table of a launch that needs no more than [entries][prefix of its grids: count + 1 each]; *d_prefix: the prefixes on the device
template <typename Entry>
int upload_entries(sga_context* ctx, DevBuf<unsigned long long>& table, const std::vector<Entry>& entries, const std::vector<uint32_t>& prefix, const uint32_t** d_prefix) {
  TableLayout L;
  const auto members = L.add<Entry>(entries.size());
  const auto grids = L.add_prefixes(prefix.size() / (entries.size() + 1), entries.size());
  SGA_TRY(table.alloc(L.words()));
  *d_prefix = L.at(grids, table.p);
  return upload_table(ctx, table.p, L.words(), [&](unsigned long long* host) {
    L.put(members, host, entries.data());
    L.put(grids, host, prefix.data());
  });
}

// ---- the box block and the call ---------------------------------------------------------------------------------------------------------
// Member j's slot: `stride` words from word 4 + stride * j of the block, as the device addresses it and as the host reads it
constexpr size_t kSlotWords = 4;  // (deskew and crop: kBoxSlotWords, cloud_ops.hpp)
inline unsigned long long* forest_slot_dev(const sga_context* ctx, size_t j, size_t stride = kSlotWords) { return ctx->h_forest_dev + 4 + stride * j; }
inline const unsigned long long* forest_slot_host(const sga_context* ctx, size_t j, size_t stride = kSlotWords) { return ctx->h_forest + 4 + stride * j; }
// what the words of a slot hold
constexpr int kSlotBox = 1;                                          // kd forest, problem creation: words 1..3, the box (box_note_decode)
constexpr int kSlotRuns = 1, kSlotOverflow = 2, kSlotNewVoxels = 3;  // grid forest: runs; map build: runs, overflow; insert: all three
// batch_preprocess.hip.  A call begins: the box block has room for `members` slots of `stride` words, *seq is the call's sequence number
int forest_call_begin(sga_context* ctx, size_t members, size_t stride, unsigned long long* seq);
// ... and, its chain enqueued with status `enqueued`, waits until the block shows `seq`.  A failed enqueue and a failed wait (`what`
// did not arrive) drain the stream: kernels already enqueued write into the block and the members' arrays, nothing stays in flight.
int forest_call_wait(sga_context* ctx, int enqueued, unsigned long long seq, const char* what);

// An entry point that makes one object per member: a failure leaves every out[k] NULL and destroys what was made inside the entry point
template <typename T>
void null_out(T** out, size_t count) {
  for (size_t k = 0; out != nullptr && k < count; k++) out[k] = nullptr;
}
template <typename T, typename Build>
int build_into(T** out, Build&& build) {
  std::vector<std::unique_ptr<T>> made;
  SGA_TRY(build(made));
  for (size_t k = 0; k < made.size(); k++) out[k] = made[k].release();
  return SGA_OK;
}

// ---- the launch counters (diagnostics: the sga_debug_*_launches entry points) --------------------------------------------------------------
// What a chain counts is its own rule: Forest (kd, features) and Grid count kernels and sorts, the others their table copies as well
enum class Chain { Forest, Grid, VoxBuild, IvmInsert, Problem, Merge, Deskew, Crop, Outliers, Overlap, Visibility, Fpfh, FeatureMatch, Ransac, PlacesAdd, PlacesQuery, PlacesWait, RadiusSearch, Cluster, RadiusWait, Plane, PlaneWait, Keypoints, KeypointsWait, Occupancy, OccupancyWait, Sweep, GridFields, kCount };
void count_launch(Chain chain);                                  // batch_preprocess.hip
int report_launches(Chain chain, unsigned long long* launches);  // the body of an sga_debug_*_launches entry point

// index_build.hip: the build of all `trees` (every field but spacing_acc filled in by the caller) enqueued on the context's stream;
// `table` (device memory: the trees, the launches' member lists, the accumulators) must live until the kernels have run
int forest_build(sga_context* ctx, std::vector<ForestTree>& trees, unsigned long long* box_seq_word, unsigned long long box_seq, DevBuf<unsigned long long>& table);
// preprocess.hip: knn_wave_kernel + features_from_list_kernel for all members
int forest_features(sga_context* ctx, const std::vector<ForestFeat>& members, int k, int flags, DevBuf<unsigned long long>& table);
void forest_tree_shape(size_t n, int* D, int* dA);  // index_build.hip: depth and first LDS level of a cloud of 1 <= n <= kForestMaxPoints points
int features_check_k(int k);     // preprocess.hip: SGA_OK, or the lone estimation's error for a num_neighbors outside its range
long long knn_wave_max_points();  // preprocess.hip: g_knn_wave_max
// index_build.hip, for the lone build and the forest: the header of a kd index over `cloud`; the six arrays behind its nodes (kd_pts .. kd_leaf)
std::unique_ptr<sga_index> kd_index_new(const sga_context* ctx, const sga_cloud* cloud);
int kd_index_alloc(sga_index* idx, const sga_cloud* cloud, int D);

// ---- the grid forest: sga_voxelgrid_sampling for B clouds in one chain of launches --------------------------
// What the host decides about a batched voxel-grid call before it launches anything (preprocess.hip: grid_forest_plan);
// sga_voxelgrid_sampling_batch acts on it, sga_debug_voxelgrid_batch_plan reports it.  A member joins the shared chain when it has a box
// (a short-key layout of its own), 1 .. 262144 points, and — members taken in the call's order — the composite key
// (member << W) | short key still fits 64 bits and the concatenation kGridForestMaxPoints points with it; every other non-empty member
// goes through the lone routine.
constexpr size_t kGridForestMaxPoints = 1ull << 24;  // cap of the concatenation (28 bytes of scratch per point: 448 MB)
struct GridForestPlan {
  int key_bytes = 0;    // 4: the composite key fits 32 bits, 8 otherwise; 0: no member in the chain
  int W = 0;            // bits below the member number: the widest short key of a member (its `total`) + 1, for the dropped points' key
  int member_bits = 0;  // bits_for(members of the chain)
  uint32_t tiles = 0;   // workgroups of the runs kernel: tiles of 2048 keys counted from every member's own start
  size_t points = 0;    // the concatenation
  std::vector<size_t> forest, lone;  // positions of the members in the chain / through the lone routine (empty members are in neither)
};
GridForestPlan grid_forest_plan(const sga_cloud* const* clouds, size_t count, double leaf);
// preprocess.hip: keys, sort, runs, centroids of the plan's forest members enqueued on the context's stream; out[j]: the records of forest
// member j (room for the member's point count); member j's run count arrives in word kSlotRuns of its slot of the box block, then `seq` in word 0
int grid_forest_enqueue(sga_context* ctx, const sga_cloud* const* clouds, double leaf, const GridForestPlan& plan, float4* const* out, unsigned long long seq);
// ---- the voxel forests (DESIGN.md sections 3.14 and 3.15): sga_index_build_gaussian_voxelmap for B clouds, sga_voxelmap_insert for B
// (Gaussian map, cloud, pose) triples, each in one chain of launches.  The sort key, the tables and the stages: voxel_steps.hpp.
constexpr size_t kVoxForestMaxMember = 262144;    // points of a member of the chain (2^18: a run's first point takes 18 bits of the rank key)
constexpr size_t kVoxForestMaxMembers = 1u << 15;  // the member number's bits above bit 49
constexpr int kVoxKeyMemberShift = 49, kVoxRankMemberShift = 18;
constexpr uint32_t kForestMaxPoints = 1024 * 32;  // = kSplitMaxPoints (index_build.hip): the clouds the split kernel holds whole
// What the host decides about a batched call before it launches anything.
struct VoxForestPlan {
  int member_bits = 0;  // bits_for(members of the chain)
  int end_bit = 0;      // the sort's: 49 + member_bits; 0: no member in the chain
  size_t points = 0;    // the concatenation
  std::vector<size_t> forest, lone, empty;  // positions of the members in the chain / through the lone routine / without points
  // member k with n >= 1 points joins the chain — members taken in the call's order — while the chain has room: at most kVoxForestMaxMember
  // points, the concatenation within kGridForestMaxPoints and the chain within kVoxForestMaxMembers members
  bool join(size_t k, size_t n) {
    if (n > kVoxForestMaxMember || points + n > kGridForestMaxPoints || forest.size() >= kVoxForestMaxMembers) return false;
    forest.push_back(k), points += n;
    return true;
  }
  void close() {
    if (forest.empty()) return;
    while ((1ull << member_bits) < forest.size()) member_bits++;
    end_bit = kVoxKeyMemberShift + member_bits;
  }
};
using IvmForestPlan = VoxForestPlan;
// the build: every non-empty member that finds no room goes through the lone routine
inline VoxForestPlan vox_forest_plan(const sga_cloud* const* clouds, size_t count) {
  VoxForestPlan P;
  for (size_t k = 0; k < count; k++) {
    const size_t n = clouds[k]->n;
    if (n == 0)
      P.empty.push_back(k);
    else if (!P.join(k, n))
      P.lone.push_back(k);
  }
  P.close();
  return P;
}
// the insert: a member joins when its map is a Gaussian incremental map.  A Gaussian map with an empty cloud takes no part in the chain's
// kernels (its counter, its sweep and its export are the call's).  Flat maps and the clouds that find no room go through the lone routine.
inline IvmForestPlan ivm_forest_plan(const sga_index* const* maps, const sga_cloud* const* clouds, size_t count) {
  IvmForestPlan P;
  for (size_t k = 0; k < count; k++) {
    const size_t n = clouds[k]->n;
    if (maps[k]->kind == SGA_INDEX_FLATMAP)
      P.lone.push_back(k);
    else if (n == 0)
      P.empty.push_back(k);
    else if (!P.join(k, n))
      P.lone.push_back(k);
  }
  P.close();
  return P;
}

// ---- the problem forest: sga_problem_create for B (target, source, pose) triples in one chain of launches ------
// What the host decides about a batched problem creation before it launches anything (problem.hip: sga_problem_create_batch acts on it,
// sga_debug_problem_batch_plan reports it).  A member joins the chain — members taken in the call's order — when its target is a kd-tree,
// a Gaussian or a flat map and its source has 1 .. kVoxForestMaxMember points, while the concatenation stays within kGridForestMaxPoints
// (48 bytes of scratch per point: two buffers of sort records and the sort's own).  Projective targets (their key is projective.hip's) and
// larger clouds go through the lone routine; an empty source gets its problem as the lone call makes it.
struct ProblemForestPlan {
  size_t points = 0;  // the concatenation
  std::vector<size_t> forest, lone, empty;
};
inline ProblemForestPlan problem_forest_plan(const sga_index* const* targets, const sga_cloud* const* sources, size_t count) {
  ProblemForestPlan P;
  for (size_t k = 0; k < count; k++) {
    const size_t n = sources[k]->n;
    if (n == 0)
      P.empty.push_back(k);
    else if (targets[k]->kind != SGA_INDEX_PROJECTIVE && n <= kVoxForestMaxMember && P.points + n <= kGridForestMaxPoints)
      P.forest.push_back(k), P.points += n;
    else
      P.lone.push_back(k);
  }
  return P;
}
// The sort record of the chain: the lone key (63 bits of Morton code against a map: it does not fit under a member number in 64 bits)
// behind the member, compared lexicographically by ONE stable merge sort; `index` — the point's position in its own cloud — rides along
// and takes no part in the comparison, so points of equal key keep the input order, as the lone call's stable sort leaves them.
struct alignas(16) ProblemKey {
  unsigned long long key;
  uint32_t member, index;
};
struct ProblemKeyLess {
  __host__ __device__ __forceinline__ bool operator()(const ProblemKey& a, const ProblemKey& b) const { return a.member < b.member || (a.member == b.member && a.key < b.key); }
};
// One member of the chain (read with scalar loads): what source_keys_kernel / source_kd_keys_kernel, gather_source_kernel and
// problem_state_init_kernel receive as arguments for it, and where its bounding box is reduced and handed over
struct ProblemMember {
  const float4* pts;  // the source
  const Cov8* cov;    // or null
  float4* opts;       // the problem's own arrays
  Cov8* ocov;
  int* corr;
  int* hint;
  int* hint2;
  uint32_t* walked;
  KdView kd;          // the target's tree (use_kd)
  Rigid<float> T;     // the pose between the two device frames (pose_to_device)
  float ox, oy, oz, inv;  // the key cells: origin and reciprocal size
  int* box;                      // {min x, y, z, max x, y, z} (box_enc) in the call's table, identity values at the start
  unsigned* done;                // positions of the member the last launch has finished: in the call's table, zero at the start
  unsigned long long* box_slot;  // words 1..3 receive the box (pinned, device-mapped: the context's box block)
  uint32_t n, off;               // the member's stretch of the concatenation
  int use_kd, pad;               // 1: source_kd_keys_kernel's key, 0: source_keys_kernel's
};

}  // namespace sga

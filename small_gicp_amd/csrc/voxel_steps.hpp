// The steps that the voxel-map routines share — the one-shot Gaussian map (voxelmap_build.hip), the incremental Gaussian and flat maps
// (voxelmap.hip), lone and batched ("forest", DESIGN.md sections 3.14 and 3.15) — each stated ONCE: what a map holds is decided by the
// expressions of this header and by nothing else.  The functions are inlined into every kernel that uses them; operand order, casts and
// the places where a value is rounded to a variable are part of their definition (-ffp-contract=fast fuses what it finds after inlining).
// Below them: the tables, the scratch and the host stages of the two voxel forests.
#pragma once
#include <climits>
#include <functional>
#include <vector>

#include "common.hpp"
#include "device_math.hpp"
#include "forest.hpp"
#include "voxel_hash.hpp"

namespace sga {

// ---- the posed point ---------------------------------------------------------------------------------------------------------------------
struct Pose12 {
  double r[9];  // row-major rotation
  double t[3];
};
// the pose sga_voxelmap_insert hands its kernels: T16 column-major (null: the identity), the cloud's device-frame origin folded in (R o_c + t)
inline Pose12 insert_pose(const double* T16, const double origin[3]) {
  Pose12 T;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T.r[3 * r + c] = T16 ? T16[4 * c + r] : (r == c ? 1.0 : 0.0);
    T.t[r] = T16 ? T16[12 + r] : 0.0;
  }
  for (int r = 0; r < 3; r++) T.t[r] += T.r[3 * r] * origin[0] + T.r[3 * r + 1] * origin[1] + T.r[3 * r + 2] * origin[2];
  return T;
}
// R p + t in double
__device__ __forceinline__ void posed_point(const Pose12& T, const float4 p, double& x, double& y, double& z) {
  x = T.r[0] * p.x + T.r[1] * p.y + T.r[2] * p.z + T.t[0];
  y = T.r[3] * p.x + T.r[4] * p.y + T.r[5] * p.z + T.t[1];
  z = T.r[6] * p.x + T.r[7] * p.y + T.r[8] * p.z + T.t[2];
}
// R C R^T as {xx, xy, xz, yy, yz, zz} (T.matrix() * cov * T.matrix().transpose(): the translation column meets the zero row of the 4x4 covariance)
__device__ __forceinline__ void posed_cov(const Pose12& T, const Cov8 q, double out[6]) {
  const double C[3][3] = {{q.xx, q.xy, q.xz}, {q.xy, q.yy, q.yz}, {q.xz, q.yz, q.zz}};
  double RC[3][3];
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) RC[a][b] = T.r[3 * a] * C[0][b] + T.r[3 * a + 1] * C[1][b] + T.r[3 * a + 2] * C[2][b];
  int k = 0;
  for (int a = 0; a < 3; a++)
    for (int b = a; b < 3; b++) out[k++] = RC[a][0] * T.r[3 * b] + RC[a][1] * T.r[3 * b + 1] + RC[a][2] * T.r[3 * b + 2];
}

// ---- voxel coordinates: true = the point is dropped -----------------------------------------------------------------------------------------
// (ux, uy, uz) = x / leaf: a point with a coordinate that voxel_key cannot hold, a NaN or an infinity among them, is dropped — decided on
// the doubles (voxel_coord_in_range, voxel_hash.hpp); the ints of a dropped point mean nothing
__device__ __forceinline__ bool voxel_coords(double ux, double uy, double uz, int& cx, int& cy, int& cz) {
  cx = fast_floor_d(ux), cy = fast_floor_d(uy), cz = fast_floor_d(uz);
  return !(voxel_coord_in_range(ux) && voxel_coord_in_range(uy) && voxel_coord_in_range(uz));
}
// incremental maps: fast_floor(T p / leaf) in double
__device__ __forceinline__ bool insert_coords(const Pose12& T, const float4 p, double inv_leaf, int& cx, int& cy, int& cz) {
  double x, y, z;
  posed_point(T, p, x, y, z);
  return voxel_coords(x * inv_leaf, y * inv_leaf, z * inv_leaf, cx, cy, cz);
}
// one-shot maps; (ox, oy, oz): origin of the cloud's device frame — voxel coordinates are those of the CALLER's frame
// (incremental_voxelmap.hpp:60)
__device__ __forceinline__ bool build_coords(const float4 p, double ox, double oy, double oz, double inv_leaf, int& cx, int& cy, int& cz) {
  return voxel_coords((static_cast<double>(p.x) + ox) * inv_leaf, (static_cast<double>(p.y) + oy) * inv_leaf, (static_cast<double>(p.z) + oz) * inv_leaf, cx, cy, cz);
}
// The device frame of an incremental map's fp32 records follows the inserted scan: its origin becomes the quantised position of the posed
// cloud frame (T.t = R o_c + t) — unless the cloud is empty, or that position is one the map holds no voxel at (beyond the key's range:
// every point near it is dropped; records relative to it would lose the map's precision for nothing), where the map keeps its frame.
inline void map_origin_after_insert(const Pose12& T, size_t n, double inv_leaf, const double old_origin[3], double origin[3]) {
  for (int k = 0; k < 3; k++) origin[k] = old_origin[k];
  if (n == 0) return;
  for (int k = 0; k < 3; k++)
    if (!voxel_coord_in_range(T.t[k] * inv_leaf)) return;
  choose_origin(T.t, T.t, origin);
}
// the coordinates a voxel_key was made of
__device__ __forceinline__ void voxel_key_coords(unsigned long long key, int* __restrict__ xyz) {
  xyz[0] = static_cast<int>(key & 0x1fffffu) - (1 << 20);
  xyz[1] = static_cast<int>((key >> 21) & 0x1fffffu) - (1 << 20);
  xyz[2] = static_cast<int>((key >> 42) & 0x1fffffu) - (1 << 20);
}

// ---- the forests' sort key ---------------------------------------------------------------------------------------------------------------
// The members' points are concatenated (member m at [off, off + n)) and sorted ONCE, stably, under
//   (m << 49) | (cz & 0xffff) << 32 | (cy & 0xffff) << 16 | (cx & 0xffff);   a dropped point: (m << 49) | (2^49 - 1), last of its member.
// The key separates the voxels of a member exactly when every axis of the member spans fewer than 65536 voxels; the keys launch reduces
// the range, the runs stage raises the member's overflow word beside its run count, and the host sends such a member through the lone routine.
constexpr unsigned long long kVoxDropped = (1ull << kVoxKeyMemberShift) - 1;  // bit 48 and everything below: behind every voxel of the member
__device__ __forceinline__ unsigned long long forest_voxel_key(int m, int cx, int cy, int cz, bool dropped) {
  const unsigned long long key = static_cast<unsigned long long>(static_cast<uint32_t>(cx) & 0xffffu) | (static_cast<unsigned long long>(static_cast<uint32_t>(cy) & 0xffffu) << 16) |
                                 (static_cast<unsigned long long>(static_cast<uint32_t>(cz) & 0xffffu) << 32);
  return (static_cast<unsigned long long>(m) << kVoxKeyMemberShift) | (dropped ? kVoxDropped : key);
}
// by every lane of a keys workgroup (lo > hi: the lane has no voxel to report): the range of the member's voxel coordinates, reduced over
// the wave, then one atomic per wave, axis and end into range = {min x, y, z, max x, y, z}
__device__ __forceinline__ void forest_range_reduce(int lo[3], int hi[3], int* range) {
  for (int a = 0; a < 3; a++)
    for (int off = 32; off > 0; off >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], off));
      hi[a] = max(hi[a], __shfl_xor(hi[a], off));
    }
  if ((threadIdx.x & 63u) == 0u && lo[0] <= hi[0])  // (a wave of dropped points only: nothing to report)
    for (int a = 0; a < 3; a++) {
      atomicMin(range + a, lo[a]);
      atomicMax(range + 3 + a, hi[a]);
    }
}
// the member's overflow word: two voxels of the member may share a key
__device__ __forceinline__ bool forest_range_overflows(const int* range) {
  bool overflow = false;
  for (int a = 0; a < 3; a++) {
    const long long lo = range[a], hi = range[3 + a];
    overflow = overflow || (hi >= lo && hi - lo >= 65536);
  }
  return overflow;
}

// ---- a voxel's record ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Cov8 cov8_of(double xx, double xy, double xz, double yy, double yz, double zz) {
  Cov8 o;
  o.xx = static_cast<float>(xx);
  o.xy = static_cast<float>(xy);
  o.xz = static_cast<float>(xz);
  o.yy = static_cast<float>(yy);
  o.yz = static_cast<float>(yz);
  o.zz = static_cast<float>(zz);
  o.pad0 = o.pad1 = 0.f;
  return o;
}
// voxel v into a table that has a free slot (the hosts keep it at most half full)
__device__ __forceinline__ void voxel_hash_insert(unsigned long long* __restrict__ hkeys, uint32_t* __restrict__ hvals, uint32_t hmask, unsigned long long key, uint32_t v) {
  uint32_t slot = voxel_hash(key) & hmask;
  for (;;) {
    const unsigned long long prev = atomicCAS(&hkeys[slot], SGA_HASH_EMPTY, key);
    if (prev == SGA_HASH_EMPTY) {
      hvals[slot] = v;
      return;
    }
    slot = (slot + 1) & hmask;
  }
}
// One-shot map, voxel v: mean of points and mean of covariances over the entries [first, end) of the sorted order that carry `key`, summed
// in insertion order in fp64.  Returns the number of points.
__device__ __forceinline__ uint32_t voxel_mean_of_run(uint32_t v, uint32_t first, uint32_t end, unsigned long long key, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order, const float4* __restrict__ pts,
                                                      const Cov8* __restrict__ cov, float4* __restrict__ means, Cov8* __restrict__ mcov) {
  double m[3] = {0, 0, 0}, c[6] = {0, 0, 0, 0, 0, 0};
  uint32_t cnt = 0;
  for (uint32_t i = first; i < end && keys[i] == key; ++i) {
    const uint32_t src = order[i];
    const float4 p = pts[src];
    const Cov8 q = cov[src];
    m[0] += p.x;
    m[1] += p.y;
    m[2] += p.z;
    c[0] += q.xx;
    c[1] += q.xy;
    c[2] += q.xz;
    c[3] += q.yy;
    c[4] += q.yz;
    c[5] += q.zz;
    cnt++;
  }
  const double inv = 1.0 / cnt;
  means[v] = make_float4(static_cast<float>(m[0] * inv), static_cast<float>(m[1] * inv), static_cast<float>(m[2] * inv), __uint_as_float(v));
  mcov[v] = cov8_of(c[0] * inv, c[1] * inv, c[2] * inv, c[3] * inv, c[4] * inv, c[5] * inv);
  return cnt;
}
// Incremental Gaussian map, voxel v: GaussianVoxel::add for the entries [first, end) that carry `key`, in insertion order, then finalize
// (gaussian_voxelmap.hpp:32-53) — un-finalize (mean *= N, cov *= N), per point N++, mean += T p, cov += R C R^T, then divide by N.
__device__ __forceinline__ void gaussian_voxel_add(uint32_t v, bool is_new, uint32_t first, uint32_t end, unsigned long long key, const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ order,
                                                   const float4* __restrict__ pts, const Cov8* __restrict__ cov, const Pose12& T, double* __restrict__ mean64, double* __restrict__ cov64, uint32_t* __restrict__ counts) {
  uint32_t N = is_new ? 0u : counts[v];
  double m[3] = {0, 0, 0}, c[6] = {0, 0, 0, 0, 0, 0};
  if (!is_new) {  // un-finalize: mean *= num_points, cov *= num_points
    for (int k = 0; k < 3; k++) m[k] = mean64[3 * v + k] * static_cast<double>(N);
    for (int k = 0; k < 6; k++) c[k] = cov64[6 * v + k] * static_cast<double>(N);
  }
  for (uint32_t i = first; i < end && keys[i] == key; ++i) {
    const uint32_t src = order[i];
    const float4 p = pts[src];
    const Cov8 q = cov[src];
    double x, y, z, rcr[6];
    posed_point(T, p, x, y, z);
    m[0] += x;
    m[1] += y;
    m[2] += z;
    posed_cov(T, q, rcr);
    for (int k = 0; k < 6; k++) c[k] += rcr[k];
    N++;
  }
  for (int k = 0; k < 3; k++) mean64[3 * v + k] = m[k] / static_cast<double>(N);
  for (int k = 0; k < 6; k++) cov64[6 * v + k] = c[k] / static_cast<double>(N);
  counts[v] = N;
}
// the fp32 records of voxel v that the factor kernels read; (ox, oy, oz): origin of the map's device frame (common.hpp) — the fp64 state is
// the caller's frame, the records are not
__device__ __forceinline__ void gaussian_voxel_export(uint32_t v, const double* __restrict__ mean64, const double* __restrict__ cov64, double ox, double oy, double oz, float4* __restrict__ means, Cov8* __restrict__ mcov) {
  means[v] = make_float4(static_cast<float>(mean64[3 * v] - ox), static_cast<float>(mean64[3 * v + 1] - oy), static_cast<float>(mean64[3 * v + 2] - oz), __uint_as_float(v));
  mcov[v] = cov8_of(cov64[6 * v], cov64[6 * v + 1], cov64[6 * v + 2], cov64[6 * v + 3], cov64[6 * v + 4], cov64[6 * v + 5]);
}

// ---- run heads: one definition for the one-shot build and the insert (voxelmap_build.hip) ---------------------------------------------------
// flags[i] = 1 where sorted position i starts a run of equal keys that is not the dropped points'
void segment_heads(sga_context* ctx, const unsigned long long* keys_sorted, size_t n, uint32_t* flags);           // lone: the dropped key is SGA_HASH_EMPTY
void segment_heads_forest(sga_context* ctx, const unsigned long long* keys_sorted, uint32_t n, uint32_t* flags);  // forest key: dropped = bit 48 set

// ---- the two voxel forests (plans: forest.hpp): tables, scratch, host stages ------------------------------------------------------------------------------
// the chain's scratch, of either forest: lives from the first stage to the end of the call (then: the stream's free list)
struct VoxelForestChain {
  DevBuf<unsigned long long> keys, keys_sorted, rank_keys, rank_keys_sorted, table1, table2, table3;
  DevBuf<uint32_t> vals, order, flags, seg_id, seg_start, seg_vid, seg_ids, seg_by_rank;  // (seg_vid, table3: the insert forest's)
  int member_bits = 0;
};
// The part of the runs stage that the two forests share, on the context's stream: the scratch of `points` points, then `keys_stage` —
// the forest's own table and keys launch, which fills ch.keys / ch.vals — then the sort under `end_bit` bits, the heads and the scan
// (ch.keys_sorted, ch.order, ch.flags, ch.seg_id).  Every command counts for `chain`.
int voxel_forest_runs(sga_context* ctx, VoxelForestChain& ch, size_t points, int member_bits, int end_bit, Chain chain, const std::function<int()>& keys_stage);
// the ranges section of a table as the host writes it: the identity of min / max, {min x, y, z, max x, y, z} per member
inline void voxel_range_identity(int* range, size_t count) {
  for (size_t j = 0; j < count; j++)
    for (int a = 0; a < 3; a++) range[6 * j + a] = INT_MAX, range[6 * j + 3 + a] = INT_MIN;
}

// One member of the build chain (read with scalar loads).  The first block is what voxel_keys_kernel receives, used by the stage before the
// host's wait; the second is what voxel_finalize_kernel receives, known once the host has the voxel counts and filled in for the stage
// behind the wait (a second table: the members that did not overflow, and the empty members, whose tables are cleared with the others').
struct VoxMember {
  const float4* pts;
  const Cov8* cov;
  double ox, oy, oz;
  int* range;                      // {min x, y, z, max x, y, z} of the voxel coordinates: in the call's table, set up with it
  unsigned long long* count_slot;  // word 1 receives the member's voxel count, word 2 its overflow word (pinned, device-mapped: the box block)
  uint32_t n, off;                 // the member's stretch of the concatenation
  float4* means;
  Cov8* mcov;
  int* coords;
  uint32_t* counts;
  unsigned long long* hkeys;
  uint32_t* hvals;
  uint32_t hmask, nvox;
  uint32_t run0, pad;              // the member's first run among the runs of the whole chain
};
// voxelmap_build.hip: keys, sort, runs of the plan's chain enqueued on the context's stream; member j's voxel count arrives in word kSlotRuns
// of its slot of the context's box block, its overflow word in word kSlotOverflow, then `seq` in word 0
int vox_forest_enqueue_runs(sga_context* ctx, const sga_cloud* const* clouds, double leaf, const VoxForestPlan& plan, unsigned long long seq, VoxelForestChain& ch);
// the ranks' sort over `runs` runs, the clearing of every member's hash table and the finalize launch (members: second block filled in)
int vox_forest_enqueue_finalize(sga_context* ctx, const std::vector<VoxMember>& members, size_t runs, double leaf, VoxelForestChain& ch);
// the header and the hash table of a Gaussian map of `nvox` voxels over `cloud`, then its per-voxel arrays: what the lone build and the
// chain make of (cloud, leaf, nvox), each at the point where it allocates
int gaussian_map_new(sga_context* ctx, const sga_cloud* cloud, double leaf, uint32_t nvox, std::unique_ptr<sga_index>& idx);
int gaussian_map_alloc_voxels(sga_index* idx);

// One member of the insert chain before the host's wait (table 1, read with scalar loads): what ivm_keys_kernel and ivm_lookup_kernel receive
struct IvmMember {
  const float4* pts;
  Pose12 T;
  double inv_leaf;
  const unsigned long long* hkeys;  // the map's table as it is before the insert
  const uint32_t* hvals;
  int* range;                       // {min x, y, z, max x, y, z} of the voxel coordinates: in the call's table, set up with it
  unsigned* counters;               // {new voxels, positions of the member the starts launch has finished}: in the call's table, zero at the start
  unsigned long long* count_slot;   // word 1: runs, word 2: overflow word, word 3: new voxels (pinned, device-mapped: the box block)
  uint32_t hmask;                   // 0: the map holds no voxel
  uint32_t n, off, pad;             // the member's stretch of the concatenation
};
// One member behind the wait (table 2): what ivm_assign_kernel and ivm_update_kernel receive, the map's arrays after growth
struct IvmUpdate {
  const float4* pts;
  const Cov8* cov;
  Pose12 T;
  double inv_leaf;
  double* mean64;
  double* cov64;
  uint32_t* counts;
  uint32_t* lru;
  int* coords;
  unsigned long long* hkeys;
  uint32_t* hvals;
  uint32_t hmask, n_old, lru_counter;
  uint32_t nseg, n_new;    // the member's runs; the new voxels among them
  uint32_t new0, old0;     // position of the member's first new / first existing run in the ranks' order
  uint32_t end;            // end of the member's stretch of the concatenation
};
// One map of the export launch (table 3): ivm_export_kernel's arguments
struct IvmExport {
  const double* mean64;
  const double* cov64;
  float4* means;
  Cov8* mcov;
  double ox, oy, oz;
  uint32_t n, pad;
};
// voxelmap.hip.  Keys, sort, heads, scan, starts + lookup of the plan's chain: member j's run count, overflow word and new-voxel count
// arrive in words kSlotRuns, kSlotOverflow, kSlotNewVoxels of its slot of the context's box block, then `seq` in word 0
int ivm_forest_enqueue_runs(sga_context* ctx, sga_index* const* maps, const sga_cloud* const* clouds, const double* T, const IvmForestPlan& plan, unsigned long long seq, VoxelForestChain& ch);
// the ranks' sort over `runs` runs (`total_new` of them new voxels) of `members_in_chain` members and the assign + update launch (members: the
// ones that did not overflow)
int ivm_forest_enqueue_update(sga_context* ctx, const std::vector<IvmUpdate>& members, size_t runs, uint32_t total_new, size_t members_in_chain, VoxelForestChain& ch);
int ivm_forest_enqueue_export(sga_context* ctx, const std::vector<IvmExport>& maps, VoxelForestChain& ch);
int ivm_reserve(sga_context* ctx, sga_index* idx, size_t n_total);  // the per-voxel arrays and the table for n_total voxels, under sga_voxelmap_insert's conditions
int ivm_lru_sweep(sga_context* ctx, sga_index* idx);                // the sweep of sga_voxelmap_insert (incremental_voxelmap.hpp:76-88) when the map's counter says it is due

}  // namespace sga

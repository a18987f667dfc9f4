// Clouds cropped and gathered on the device: sga_cloud_crop / _batch / _device — range and box filters with a
// stable compaction, one table and ONE launch for B members — and the gather behind sga_cloud_select (indices) and sga_cloud_slice (a range).
#include "cloud_box.hpp"
#include "device_io.hpp"
#include "forest.hpp"
#include "lookback.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kCropThreads = 256, kCropItems = 8, kCropTile = kCropThreads * kCropItems;
static_assert(kCropThreads == kIoBlock, "box64_reduce_block reduces the waves of a 256-thread workgroup");
constexpr unsigned kCropSpinLimit = 1u << 22;  // polls of one look-back window before a workgroup gives up (seconds: the call then fails)

// One member of a crop (read with scalar loads): its records and where the kept ones go, the predicate's constants — formed on the host
// in double —, its words of the call's table and its slot of the box block.
struct CropMember {
  const float4* pts;
  const float4* nrm;  // or null
  const Cov8* cov;
  float4* opts;
  float4* onrm;
  Cov8* ocov;
  uint32_t* kept32;          // the indices kept: a stretch of a slot of the staging ring, by its device address; or null
  long long* kept64;         // ... or device memory of the caller's; or null
  unsigned long long* acc;   // {min x y z, max x y z (encoded), ticket, finished} in the call's table (cloud_box.hpp: MemberBoxes)
  unsigned long long* slot;  // its slot of the context's box block (pinned, device-mapped): the count, the box
  const double* stat;        // the statistic predicate (sga_cloud_remove_outliers, cloud_outliers.hip): one value per point, in the cloud's
  const double* limit;       // order, and the limit they are held against — device memory written by earlier launches; or both null
  double d[3];               // o - center
  double o[3];
  double r2min, r2max;
  double blo[3], bhi[3];
  uint32_t n, tiles;
  int box_mode;
  int every_record;          // 1: the crop's own predicate is not applied (CropStat::every_record, cloud_ops.hpp)
};
static_assert(sizeof(CropMember) % 8 == 0, "the table is copied in 8-byte words");

// The predicate, stated once (small_gicp_amd.h: sga_crop).
__device__ __forceinline__ bool crop_keeps(const CropMember& g, const float4 p) {
  const bool finite = fabsf(p.x) <= 3.4028234e38f && fabsf(p.y) <= 3.4028234e38f && fabsf(p.z) <= 3.4028234e38f;
  const double x = static_cast<double>(p.x) + g.d[0], y = static_cast<double>(p.y) + g.d[1], z = static_cast<double>(p.z) + g.d[2];
  const double d2 = x * x + y * y + z * z;
  bool keep = finite && g.r2min <= d2 && d2 <= g.r2max;
  if (g.box_mode != 0) {  // (uniform)
    const double bx = static_cast<double>(p.x) + g.o[0], by = static_cast<double>(p.y) + g.o[1], bz = static_cast<double>(p.z) + g.o[2];
    const bool inside = g.blo[0] <= bx && bx <= g.bhi[0] && g.blo[1] <= by && by <= g.bhi[1] && g.blo[2] <= bz && bz <= g.bhi[2];
    keep = keep && (inside == (g.box_mode == 1));
  }
  return keep;
}

// Record i, whose point is p, becomes record r: the point with the index word r, then normal and covariance (two float4) where the output keeps them.
__device__ __forceinline__ void copy_record(const float4 p, const float4* __restrict__ nrm, const Cov8* __restrict__ cov, uint32_t i, float4* __restrict__ opts, float4* __restrict__ onrm, Cov8* __restrict__ ocov, uint32_t r) {
  opts[r] = make_float4(p.x, p.y, p.z, __uint_as_float(r));
  if (onrm != nullptr) onrm[r] = nrm[i];
  if (ocov != nullptr) {
    const float4* cin = reinterpret_cast<const float4*>(cov + i);
    float4* cout = reinterpret_cast<float4*>(ocov + r);
    const float4 c0 = cin[0], c1 = cin[1];
    cout[0] = c0;
    cout[1] = c1;
  }
}

}  // namespace

// Clouds -> the records that pass their member's predicate, in the input's order.  Workgroup b belongs to the member m with prefix[m] <= b
// < prefix[m + 1] and takes the member's NEXT tile of 2048 points from the member's own ticket word.
//   Forward progress (ds_segments_kernel's argument, preprocess.hip, per member): arrival order equals tile order, so the workgroup
//   that holds tile t has taken its ticket after the holders of the tiles 0 .. t - 1 took theirs — every one of them is already RUNNING.
//   A running workgroup publishes its aggregate after its own loads and one barrier, before it waits for anybody, and the look-back
//   waits for nothing but "published, aggregate or prefix": it only ever waits for workgroups that are running and that reach their
//   publication without waiting.  No workgroup waits for one that has not been dispatched, whatever the grid's size and the order of
//   dispatch.  (A poll count bounds every wait all the same: a workgroup that gives up publishes what it has, marks the member, and the
//   host reports the call as failed — a shared machine gets its kernel back.)
// The tile is wave-striped: load j of wave w reads the 64 consecutive records (w * 8 + j) * 64 + lane of the tile, so a kept lane's rank
// within its load is a __ballot and an mbcnt, a wave's total eight popcounts.  Wave totals meet in LDS; the tile's aggregate and inclusive
// prefix go through the member's status words [prefix[m], prefix[m + 1]) of the context's array under the call's epoch, the look-back
// 64 predecessors at a time.  Kept records go to exclusive prefix + rank: points (w = the new index), then normals and covariances for
// kept lanes only, and the index kept.  The box of the kept records is joined in the member's accumulator; the member's last workgroup
// to FINISH writes the count and the box into the member's slot of the box block and arrives (forest_box_arrive).
__global__ __launch_bounds__(kCropThreads) void crop_cloud_kernel(const CropMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, unsigned long long* __restrict__ status_g, unsigned epoch, const ForestBoxes hand) {
  __shared__ uint32_t sh_tile, sh_wave[kCropThreads / 64], sh_excl;
  __shared__ bool sh_last, sh_failed;
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const CropMember& g = *uniform_const(members + m);
  unsigned long long* __restrict__ status = status_g + prefix[m];
  if (threadIdx.x == 0) sh_tile = static_cast<uint32_t>(__hip_atomic_fetch_add(&g.acc[6], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  __syncthreads();
  const uint32_t tile = sh_tile;  // < g.tiles: the member has g.tiles workgroups and the word starts at zero
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t first = tile * static_cast<uint32_t>(kCropTile) + static_cast<uint32_t>(wave * kCropItems * 64 + lane);
  float4 p[kCropItems];
#pragma unroll
  for (int j = 0; j < kCropItems; j++) {
    const uint32_t i = first + 64u * j;
    p[j] = i < g.n ? g.pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  unsigned long long kept[kCropItems];  // (wave-uniform)
  uint32_t wave_total = 0;
#pragma unroll
  for (int j = 0; j < kCropItems; j++) {
    bool keep = first + 64u * j < g.n && (g.every_record != 0 || crop_keeps(g, p[j]));  // (uniform)
    if (g.stat != nullptr) keep = keep && g.stat[first + 64u * j] <= *g.limit;  // (uniform; read only where the point exists and passes)
    kept[j] = __ballot(keep);
    wave_total += static_cast<uint32_t>(__popcll(kept[j]));
  }
  if (lane == 0) sh_wave[wave] = wave_total;
  __syncthreads();
  uint32_t wave_base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kCropThreads / 64; w++) {
    if (w < wave) wave_base += sh_wave[w];
    total += sh_wave[w];
  }
  const unsigned long long tag = static_cast<unsigned long long>(epoch) << kLookEpochShift;
  bool gave_up = false;  // (wave 0, uniform)
  if (wave == 0) {
    uint32_t excl = 0;
    if (tile > 0) {
      if (lane == 0) __hip_atomic_store(&status[tile], tag | kLookAgg | total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      int look = static_cast<int>(tile) - 1;
      for (;;) {
        const int j = look - lane;
        unsigned long long w;
        unsigned polls = 0;
        for (;;) {
          w = j >= 0 ? __hip_atomic_load(&status[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) : (tag | kLookPrefix);
          if (__ballot((w >> kLookEpochShift) != (tag >> kLookEpochShift)) == 0ull) break;  // every predecessor of this window has published
          if (++polls >= kCropSpinLimit) {
            gave_up = true;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        if (gave_up) break;
        const unsigned long long prefixes = __ballot((w & kLookPrefix) != 0ull);
        const int stop = prefixes != 0ull ? __ffsll(static_cast<long long>(prefixes)) - 1 : 63;  // nearest predecessor holding an inclusive prefix
        uint32_t v = lane <= stop ? static_cast<uint32_t>(w) : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        excl += v;
        if (prefixes != 0ull) break;
        look -= 64;
      }
    }
    if (lane == 0) {
      __hip_atomic_store(&status[tile], tag | kLookPrefix | (excl + total), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      sh_excl = excl;  // (after a give-up: below the true prefix — every write stays inside the member's arrays)
    }
  }
  __syncthreads();
  uint32_t dst = sh_excl + wave_base;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
  for (int j = 0; j < kCropItems; j++) {
    const unsigned long long mask = kept[j];
    if ((mask >> lane) & 1ull) {
      const uint32_t i = first + 64u * j;
      const uint32_t r = dst + __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
      copy_record(p[j], g.nrm, g.cov, i, g.opts, g.onrm, g.ocov, r);
      if (g.kept32 != nullptr) g.kept32[r] = i;
      if (g.kept64 != nullptr) g.kept64[r] = static_cast<long long>(i);
      const double x = p[j].x, y = p[j].y, z = p[j].z;
      lo[0] = fmin(lo[0], x), lo[1] = fmin(lo[1], y), lo[2] = fmin(lo[2], z);
      hi[0] = fmax(hi[0], x), hi[1] = fmax(hi[1], y), hi[2] = fmax(hi[2], z);
    }
    dst += static_cast<uint32_t>(__popcll(mask));
  }
  if (g.kept32 != nullptr) __threadfence_system();  // (uniform) the indices live in host memory: on their way before this workgroup counts as finished
  box64_reduce_block(lo, hi, g.acc);
  if (threadIdx.x == 0) {
    const unsigned long long mine = 1ull | (gave_up ? 1ull << 32 : 0ull);  // low word: workgroups finished; high word: workgroups that gave up
    const unsigned long long before = __hip_atomic_fetch_add(&g.acc[7], mine, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    sh_last = static_cast<uint32_t>(before) == g.tiles - 1u;
    sh_failed = ((before + mine) >> 32) != 0ull;
  }
  __syncthreads();
  if (!sh_last) return;  // workgroup-uniform
  if (threadIdx.x < 6) g.slot[kBoxSlotLo + threadIdx.x] = __hip_atomic_load(&g.acc[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (threadIdx.x == 0) {
    // every tile has finished: the last tile's word holds its inclusive prefix, the member's count
    const unsigned long long w = __hip_atomic_load(&status[g.tiles - 1u], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
    g.slot[kBoxSlotCount] = sh_failed ? ~0ull : (w & 0xffffffffull);
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) forest_box_arrive(hand);
}

// out record j = in record idx[j] (select), or first + j when idx is null (slice); the index word j
__global__ __launch_bounds__(256) void gather_cloud_kernel(const float4* __restrict__ pts, const float4* __restrict__ nrm, const Cov8* __restrict__ cov, const uint32_t* __restrict__ idx, uint32_t first, uint32_t m, float4* __restrict__ opts,
                                                           float4* __restrict__ onrm, Cov8* __restrict__ ocov) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= m) return;
  const uint32_t i = idx != nullptr ? idx[j] : first + j;
  copy_record(pts[i], nrm, cov, i, opts, onrm, ocov, j);
}

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

// what sga_cloud_crop refuses of crops[k] (nothing but the struct is read)
int crop_check(const sga_crop& c, size_t k) {
  if (!(c.min_range >= 0.0)) return fail(SGA_ERR_INVALID, "crops[%zu]: min_range is negative or NaN", k);
  if (c.max_range != c.max_range) return fail(SGA_ERR_INVALID, "crops[%zu]: max_range is NaN", k);
  if (c.min_range > c.max_range) return fail(SGA_ERR_INVALID, "crops[%zu]: min_range > max_range", k);
  for (int a = 0; a < 3; a++)
    if (!is_finite(c.center[a])) return fail(SGA_ERR_INVALID, "crops[%zu]: center has a non-finite entry", k);
  if (c.box_mode < 0 || c.box_mode > 2) return fail(SGA_ERR_INVALID, "crops[%zu]: box_mode %d is not 0, 1 or 2", k, c.box_mode);
  for (int a = 0; c.box_mode != 0 && a < 3; a++) {
    if (c.box_lo[a] != c.box_lo[a] || c.box_hi[a] != c.box_hi[a]) return fail(SGA_ERR_INVALID, "crops[%zu]: box_lo / box_hi has a NaN entry", k);
    if (c.box_lo[a] > c.box_hi[a]) return fail(SGA_ERR_INVALID, "crops[%zu]: box_lo > box_hi on axis %d", k, a);
  }
  return SGA_OK;
}

// What the records of `in` and the crop `cr` alone decide of a member's entry: the inputs, the predicate's constants, the tiles.
CropMember crop_member(const sga_cloud* in, const sga_crop& cr) {
  CropMember g;
  std::memset(&g, 0, sizeof(g));
  g.pts = in->pts.p, g.nrm = in->has_normals ? in->nrm.p : nullptr, g.cov = in->has_covs ? in->cov.p : nullptr;
  for (int a = 0; a < 3; a++) {
    g.d[a] = in->origin[a] - cr.center[a];
    g.o[a] = in->origin[a];
    g.blo[a] = cr.box_lo[a], g.bhi[a] = cr.box_hi[a];
  }
  g.r2min = cr.min_range * cr.min_range;
  g.r2max = cr.max_range * cr.max_range;
  g.n = static_cast<uint32_t>(in->n);
  g.tiles = (g.n + kCropTile - 1u) / kCropTile;
  g.box_mode = cr.box_mode;
  return g;
}

// `count` clouds, each cropped by its own predicate: one table — [members][prefix of the grid][accumulators: 8 words per member][ticket] —
// and ONE launch over the members' tiles.  The indices kept leave as uint32 through ONE slot of the staging ring, which the kernel writes
// by its device address and the host widens after the wait (kept), or as int64 into device memory of the caller's (d_kept, one member).
// The call waits for the members' counts and boxes (the context's box block: its one wait), on a stream-ordered context too.
// stat (one member only): the statistic predicate on top of the crop's, its launches counted under the chain it names.
int cloud_crop(sga_context* ctx, const sga_cloud* const* clouds, const sga_crop* crops, int64_t* const* kept, int64_t* d_kept, bool device_form, size_t count, void* user_stream, int flags, sga_cloud** out,
               const CropStat* stat = nullptr) {
  const Chain chain = stat != nullptr ? stat->chain : Chain::Crop;
  if (count == 0) return SGA_OK;
  null_out(out, count);
  if (!ctx || !out || !clouds || !crops) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(cloud_members_args(clouds, count));
  for (size_t k = 0; k < count; k++) SGA_TRY(crop_check(crops[k], k));
  // ---- (from here on the handles are read)
  CloudMembers mem;
  SGA_TRY(cloud_members(ctx, clouds, count, kCropTile, &mem));
  const std::vector<size_t>& live = mem.live;
  size_t kept_words = 0;
  for (size_t k : live)
    if (kept != nullptr && kept[k] != nullptr) kept_words += clouds[k]->n;
  if (mem.blocks >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points in all (%zu tiles of %d; limit 2^31-1)", mem.blocks, kCropTile);
  if (!live.empty()) SGA_HIP(hipSetDevice(ctx->device));
  if (d_kept != nullptr && !live.empty()) SGA_TRY(check_device_range(ctx, d_kept, clouds[0]->n * sizeof(int64_t), sizeof(int64_t), "d_kept", "sga_cloud_crop"));
  StreamScope stream_scope(ctx->stream);
  std::vector<std::unique_ptr<sga_cloud>> made(count);  // with room for the input: the count is known only once the kernel has run
  for (size_t k = 0; k < count; k++) SGA_TRY(cloud_make_like(ctx, clouds[k], clouds[k]->n, &made[k]));
  if (live.empty()) return hand_over(made, out);
  const size_t L = live.size();
  for (size_t k : live) SGA_TRY(wait_ready(ctx, clouds[k]->ready));  // made by another context in stream-ordered mode (common.hpp: Ready)
  sga_context::StageSlot* kslot = nullptr;
  if (kept_words > 0) SGA_TRY(stage_acquire(ctx, kept_words * sizeof(uint32_t), &kslot));
  unsigned epoch = 0;
  SGA_TRY(voxelgrid_status(ctx, static_cast<uint32_t>(mem.blocks), &epoch));
  // ---- the table
  TableLayout lay;
  const auto s_members = lay.add<CropMember>(L);
  const auto s_prefix = lay.add_prefixes(1, L);
  MemberBoxes boxes;
  boxes.add(lay, L);
  const auto s_limit = lay.add<double>(stat != nullptr ? 1 : 0);  // the limit of a statistic predicate that no launch computes
  DevBuf<unsigned long long> table;
  ForestBoxes hand;
  SGA_TRY(boxes.begin(ctx, lay, table, &hand));
  std::vector<CropMember> members(L);
  std::vector<uint32_t> prefix(L + 1, 0u);
  size_t kat = 0;
  for (size_t j = 0; j < L; j++) {
    const size_t k = live[j];
    CropMember& g = members[j] = crop_member(clouds[k], crops[k]);
    g.opts = made[k]->pts.p, g.onrm = made[k]->nrm.p, g.ocov = made[k]->cov.p;
    if (kept != nullptr && kept[k] != nullptr) g.kept32 = static_cast<uint32_t*>(kslot->dev) + kat, kat += g.n;
    g.kept64 = reinterpret_cast<long long*>(d_kept);
    g.acc = lay.at(boxes.acc, table.p) + 8 * j, g.slot = forest_slot_dev(ctx, j, kBoxSlotWords);
    if (stat != nullptr) g.stat = stat->d, g.limit = stat->limit != nullptr ? stat->limit : lay.at(s_limit, table.p), g.every_record = stat->every_record ? 1 : 0;
    prefix[j + 1] = prefix[j] + g.tiles;
  }
  IoOrder ord;
  if (device_form) SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  auto enqueue = [&]() -> int {
    count_launch(chain);
    SGA_TRY(upload_table(ctx, table.p, lay.words(), [&](unsigned long long* host) {
      lay.put(s_members, host, members.data());
      lay.put(s_prefix, host, prefix.data());
      boxes.init(host);
      if (stat != nullptr) *lay.at(s_limit, host) = stat->limit_value;
    }));
    count_launch(chain);
    hipLaunchKernelGGL(crop_cloud_kernel, dim3(prefix[L]), dim3(kCropThreads), 0, ctx->stream, lay.at(s_members, table.p), lay.at(s_prefix, table.p), static_cast<int>(L), ctx->vg_status.p, epoch, hand);
    SGA_HIP(hipGetLastError());
    return SGA_OK;
  };
  SGA_TRY(forest_call_wait(ctx, enqueue(), hand.seq, "counts of a crop"));  // (the wait shows that every workgroup has written what it writes)
  if (device_form) SGA_TRY(io_end(ctx, ord));
  kat = 0;
  for (size_t j = 0; j < L; j++) {
    const size_t k = live[j];
    const uint32_t* src = kept != nullptr && kept[k] != nullptr ? static_cast<const uint32_t*>(kslot->host) + kat : nullptr;  // as the kernel was told
    if (src != nullptr) kat += clouds[k]->n;
    const unsigned long long m = forest_slot_host(ctx, j, kBoxSlotWords)[kBoxSlotCount];
    if (m == ~0ull) return fail(SGA_ERR_HIP, "the crop of cloud %zu gave up waiting for a predecessor tile", k);
    if (m > clouds[k]->n) return fail(SGA_ERR_HIP, "the device reported %llu points kept of the %zu of cloud %zu", m, clouds[k]->n, k);
    if (m == 0) {
      SGA_TRY(cloud_make_like(ctx, clouds[k], 0, &made[k]));  // nothing kept: an empty cloud without attributes
      continue;
    }
    made[k]->n = static_cast<size_t>(m);
    boxes.read(ctx, j, made[k].get());
    for (size_t i = 0; src != nullptr && i < m; i++) kept[k][i] = static_cast<int64_t>(src[i]);
  }
  for (size_t k : live) SGA_TRY(mark_ready(ctx, made[k]->ready));
  return hand_over(made, out);
}

// The m records indices[j] of `cloud` (select), or first .. first + m - 1 when indices is null (slice), as a cloud in its cloud's device frame:
// ONE launch, none for m == 0, no host wait (the indices' slot of the staging ring is reused only behind the kernel), no box.  m == 0: an
// empty cloud without attributes, unless keep_flags (a slice keeps its cloud's).  The caller has checked the arguments and entered the context.
int cloud_gather(sga_context* ctx, const sga_cloud* cloud, const int64_t* indices, size_t first, size_t m, bool keep_flags, sga_cloud** out) {
  std::unique_ptr<sga_cloud> c;
  SGA_TRY(cloud_make(ctx, cloud->origin, m, (m > 0 || keep_flags) && cloud->has_normals, (m > 0 || keep_flags) && cloud->has_covs, &c));
  if (m > 0) {
    SGA_TRY(wait_ready(ctx, cloud->ready));
    sga_context::StageSlot* slot = nullptr;
    if (indices != nullptr) {
      SGA_TRY(stage_acquire(ctx, m * sizeof(uint32_t), &slot));
      uint32_t* host = static_cast<uint32_t*>(slot->host);
      for (size_t j = 0; j < m; j++) host[j] = static_cast<uint32_t>(indices[j]);
    }
    hipLaunchKernelGGL(gather_cloud_kernel, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, cloud->pts.p, cloud->nrm.p, cloud->cov.p, slot != nullptr ? static_cast<const uint32_t*>(slot->dev) : nullptr, static_cast<uint32_t>(first),
                       static_cast<uint32_t>(m), c->pts.p, c->nrm.p, c->cov.p);
    SGA_HIP(hipGetLastError());
    if (slot != nullptr) SGA_TRY(stage_release(ctx, slot));
    SGA_TRY(mark_ready(ctx, c->ready));
  }
  *out = c.release();
  return SGA_OK;
}

}  // namespace

int cloud_crop_stat(sga_context* ctx, const sga_cloud* cloud, const CropStat& stat, int64_t* kept, sga_cloud** out) {
  sga_crop all;  // every finite point passes the crop's own predicate
  sga_crop_default(&all);
  return cloud_crop(ctx, &cloud, &all, &kept, nullptr, false, 1, nullptr, 0, out, &stat);
}

}  // namespace sga

using namespace sga;

extern "C" {

void sga_crop_default(sga_crop* crop) {
  if (!crop) return;
  std::memset(crop, 0, sizeof(*crop));
  crop->max_range = INFINITY;
}

int sga_cloud_crop_batch(sga_context* ctx, const sga_cloud* const* clouds, const sga_crop* crops, int64_t* const* kept, size_t count, sga_cloud** out) {
  return cloud_crop(ctx, clouds, crops, kept, nullptr, false, count, nullptr, 0, out);
}

int sga_cloud_crop(sga_context* ctx, const sga_cloud* cloud, const sga_crop* crop, int64_t* kept, sga_cloud** out) {
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  return cloud_crop(ctx, &cloud, crop, &kept, nullptr, false, 1, nullptr, 0, out);
}

int sga_cloud_crop_device(sga_context* ctx, const sga_cloud* cloud, const sga_crop* crop, int64_t* d_kept, void* user_stream, int flags, sga_cloud** out) {
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  return cloud_crop(ctx, &cloud, crop, nullptr, d_kept, true, 1, user_stream, flags, out);
}

int sga_cloud_select(sga_context* ctx, const sga_cloud* cloud, const int64_t* indices, size_t m, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !cloud || !out || (m > 0 && !indices)) return fail(SGA_ERR_INVALID, "null argument");
  if (m >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many indices (%zu; limit 2^31-1)", m);
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  for (size_t j = 0; j < m; j++)
    if (indices[j] < 0 || static_cast<unsigned long long>(indices[j]) >= cloud->n) return fail(SGA_ERR_INVALID, "indices[%zu] = %lld is outside a cloud of %zu points", j, static_cast<long long>(indices[j]), cloud->n);
  SGA_ENTER(ctx);
  return cloud_gather(ctx, cloud, indices, 0, m, false, out);
}

int sga_cloud_slice(sga_context* ctx, const sga_cloud* cloud, size_t first, size_t count, sga_cloud** out) {
  if (!ctx || !cloud || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (first > cloud->n || count > cloud->n - first) return fail(SGA_ERR_INVALID, "slice [%zu, %zu) outside a cloud of %zu points", first, first + count, cloud->n);
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  *out = nullptr;
  SGA_ENTER(ctx);
  return cloud_gather(ctx, cloud, nullptr, first, count, true, out);  // (shards of one registration share their cloud's device frame)
}

int sga_debug_cloud_crop_launches(unsigned long long* launches) { return report_launches(Chain::Crop, launches); }

}  // extern "C"

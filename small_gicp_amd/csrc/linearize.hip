// K1 (linearize) and K2 (error): the per-iteration hot loop of Registration<>::align on gfx950.
//
// Replaces ParallelReductionOMP::linearize / ::error (registration/reduction_omp.hpp:24-70) fused with
// {GICP,PointToPlaneICP,ICP}Factor::linearize / ::error (factors/*.hpp), RobustFactor (robust_kernel.hpp:70-98),
// DistanceRejector (rejector.hpp:19-28) and the nearest-neighbour search (ann/kdtree.hpp:193-233 or
// ann/incremental_voxelmap.hpp:99-119).  The 6x6 solve stays on the host (optimizer.hip).
//
// One linearization pass = ONE search + factor launch and reduce_rows_kernel:
//   search_linearize_kernel   one query per lane, one wave per workgroup; cold passes (full walk) and warm passes after larger
//                             motions (certificate check first); the wave then evaluates the factors of its own 64 points
//   nn_search_queue_kernel    warm passes after small motions: certificate check per tile, the few walks fed from a queue, the
//                             factors of the chunk (4 tiles) at the end
//   nn_search_kernel + linearize_kernel   the same in two launches: host-rejector callback, fp64 per-pair arithmetic;
//                             linearize_kernel alone for voxel-map targets (the lookup happens inside it)
// Factor stage in MOMENT form (accumulate_moments / derived_entry): 74 sums per pass that are both the normal equations and the
// coefficients of the quadratic error model sga_error answers from without a pass over the cloud; error_kernel (K2) only for robust
// factors, the async API and tests.  Sums: DPP inside a wave (fp32), fp64 across waves, one row of 96 doubles per tile / chunk /
// workgroup, added in fixed order by reduce_rows_kernel (no floating-point atomics: bit-reproducible).
//
// Where things live.  THIS translation unit compiles every kernel of the pass — the device code of the four headers exists here only,
// and so does every compile-time knob (SGA_SL_WAVES, SGA_SL_WAVES_WARM, SGA_CERT_WAVES, SGA_MAX_BLOCKS, SGA_SPACING_REF):
//   pass_layout.hpp    the partial row (constants, the comment that documents its columns) and the parameter structs LinParams, NNParams,
//                      ErrParams, FusedTail, BatchPair
//   search_stage.hpp   device functions of the search: tile_schedule, certify, walk_lane, search_lane, search_tile_of_block
//   factor_stage.hpp   device functions of the factors: pair_factor, pair_moments, accumulate_moments, kernarg_lin_params, linearize_group
//   reduce_rows.hpp    derived_entry, fused_tail, reduce_rows_kernel, batch_reduce_rows_kernel, launch_reduce
//   linearize.hip      the __global__ pass kernels, the tuning table, the routing (Route, PassPlan, plan_pass, linearize_dispatch,
//                      error_dispatch), the two halves of the entry points (enqueue / collect), batch_round, the C entry points that launch
//                      a kernel of this file, preload_hot_kernels
// and beside it, in translation units of their own (they launch no template of this file):
//   frames.hip         device frames at the C-ABI boundary (problem_pose, problem_system_to_caller, frame_accumulator_kernel) and the shard frame check
//   error_model.hip    the quadratic error model on the host (error_model_value, sga_error_model_eval) and sga_unpack_accumulator
//   context.hip        wait_published (notes.hpp): the one host wait for a sequence word the device publishes
#include <algorithm>
#include <type_traits>

#include "batch.hpp"
#include "common.hpp"
#include "device_math.hpp"
#include "uniform.hpp"
#include "cell_grid.hpp"
#include "kd_search.hpp"
#include "projective.hpp"
#include "voxel_hash.hpp"
#include "notes.hpp"
#include "pass_layout.hpp"
#include "search_stage.hpp"
#include "factor_stage.hpp"
#include "reduce_rows.hpp"

void sga_profile_collect_pending(sga_context* ctx);

namespace sga {

int comm_allreduce_sum(sga_context* ctx, double* d_buf, size_t count);
// cell_grid.hip: one exact search pass over the target's cell grid (nn / nn2 / rex of every source point), and the rings a reach needs
template <typename Real>
int grid_search_pass(sga_context* ctx, const sga_index* idx, const float4* src_pts, int n, const Rigid<Real>& T, float reach2, int* nn, int* nn2, float* rex, uint32_t* stats);
int grid_rings_for(const sga_index* idx, double reach);

#ifndef SGA_SPACING_REF
#define SGA_SPACING_REF 0.5486  // length scale (geometric mean leaf diagonal) of the C3 target (scripts/spacing_probe.py), the scene the routing thresholds were tuned on
#endif

template <typename Real, int BLOCK, bool CHECK>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(8, 8))) void nn_search_kernel(const NNParams<Real> p) {
  extern __shared__ uint32_t kd_stack[];  // tree depth x BLOCK traversal stack slots
#ifdef SGA_KD_TRIPS
  const unsigned long long wave_t0 = wall_clock64();
#endif
  const int tile = search_tile_of_block();
  const int i = tile * BLOCK + threadIdx.x;
  if (i >= p.n) return;
  const float4 ps = p.src_pts[i];
  Real x, y, z;
  transform_point<Real>(p.T, ps.x, ps.y, ps.z, x, y, z);
  search_lane<Real, BLOCK, CHECK>(p, tile, i, ps, static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), kd_stack);
#ifdef SGA_KD_TRIPS
  if (blockIdx.x < 32768) {
    const unsigned long long t1 = wall_clock64();
    if (threadIdx.x == __ffsll(static_cast<long long>(__ballot(true))) - 1) {
      g_kd_wave_times[2 * blockIdx.x] = wave_t0;
      g_kd_wave_times[2 * blockIdx.x + 1] = t1;
    }
  }
#endif
}

// The search, queue-fed.  The walks of neighbouring queries differ in length (one leaf for most, twenty for a few): with one query per
// lane for the lifetime of a wave, a wave runs as long as its longest walk and most lanes idle most of the time (measured: about a
// fifth of the VALU lanes active).  Here a wave owns a CHUNK of consecutive tiles and a small queue in LDS:
//   stage:  a tile of 64 queries is prepared by all 64 lanes at once (coalesced loads; in a warm pass the certificate check — lanes
//           whose certificate holds are done right there) and the queries that need a walk are appended to the queue, each with the
//           group (kd_search.hpp: the leaves under a node of depth D - 2) to start from: the one of its previous neighbour (or, for a
//           point without one, the group of its own cell:
//           remembered in nn2[] as -2 - rank, or located by a plain descent).
//   walk:   a lane without a query takes the next one from the queue.  Its first round visits the start group and fetches the records
//           of all ancestors of that leaf at once (kd_push_path: independent loads, one latency); later rounds are the usual
//           descend -> scan -> pop.  A lane whose walk is over writes its result and is refilled in the next round.
// The result is the canonical nearest neighbour (kd_search.hpp) whatever the order; only the exclusion radii may differ from the
// one-query-per-lane kernel's (both are valid bounds).
constexpr int kQueueCap = 128;        // entries; a tile is staged while at most kQueueCap - 64 are waiting
constexpr int kPathRecords = 10;      // pair records fetched at once by kd_push_path: covers depth 20 (8 M points); deeper trees take a second batch

// FACTOR >= 0: when the chunk's searches are done the wave also evaluates the factors of its chunk (four tiles at a time, like
// linearize_kernel) and writes ONE partial row per chunk — in the warm passes this kernel runs, the memory system and the VALUs are
// mostly idle, so the factor kernel's work all but disappears inside it (and its launch, start-up and tail with it).
template <typename Real, bool CHECK, int FACTOR = -1>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 6))) void nn_search_queue_kernel(const NNParams<Real> p, const LinParams<Real> lp) {
  extern __shared__ uint32_t kd_stack[];  // tree depth x 64 traversal stack slots
  __shared__ float4 q_pt[kQueueCap];      // query (x, y, z), w = exploration slack
  __shared__ int q_idx[kQueueCap];        // source point
  __shared__ uint32_t q_leaf[kQueueCap];  // start group (heap node of depth gdepth)
  const int lane = threadIdx.x;
  const int D = p.kd.gdepth;  // the walk's unit is the group (kd_search.hpp)
  const int num_tiles = (p.n + 63) >> 6;
  // XCD-aware chunk order (workgroup b runs on XCD b % 8): each XCD gets one contiguous eighth of the chunks
  const int nblk = static_cast<int>(gridDim.x), per_xcd = nblk >> 3, b = blockIdx.x;
  const int chunk = b < 8 * per_xcd ? (b & 7) * per_xcd + (b >> 3) : b;
  int tile = chunk * p.chunk_tiles;
  const int tile_end = min(tile + p.chunk_tiles, num_tiles);
  int q_head = 0, q_count = 0;  // wave-uniform
#ifdef SGA_KD_TRIPS
  const unsigned long long qt0 = wall_clock64();
  unsigned long long qt_stage = 0, qt_last = qt0;
#endif

  bool busy = false, fresh = false;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  int qi = -1;
  uint32_t node = 1;
  int depth = 0, sp = 0;
  KdState s = kd_state(p.bound2, 0.f);

  for (;;) {
    // ---- stage tiles while the queue has room
    while (tile < tile_end && q_count <= kQueueCap - 64) {
      const int i = tile * 64 + lane;
      bool need = i < p.n;
      float fx = 0.f, fy = 0.f, fz = 0.f, slack = 0.f;
      int seed = -1, cand2 = -1;
      if (need) {
        const float4 ps = p.src_pts[i];
        Real x, y, z;
        transform_point<Real>(p.T, ps.x, ps.y, ps.z, x, y, z);
        fx = static_cast<float>(x), fy = static_cast<float>(y), fz = static_cast<float>(z);
        seed = p.nn[i];
        cand2 = p.nn2[i];
        if constexpr (CHECK) {
          Real ox, oy, oz;
          transform_point<Real>(p.T_prev, ps.x, ps.y, ps.z, ox, oy, oz);
          const float moved = sqrtf(kd_dist2(static_cast<float>(ox), static_cast<float>(oy), static_cast<float>(oz), fx, fy, fz));
          float d1 = INFINITY, d2 = INFINITY;
          if (seed >= 0) {
            const float4 c = p.kd.pts[seed];
            d1 = kd_dist2(c.x, c.y, c.z, fx, fy, fz);
          }
          if (cand2 >= 0) {
            const float4 c = p.kd.pts[cand2];
            d2 = kd_dist2(c.x, c.y, c.z, fx, fy, fz);
          }
          const bool swap = cand2 >= 0 && (d2 < d1 || (d2 == d1 && cand2 < seed));  // the canonical rule: equidistant -> lower position
          const int best = swap ? cand2 : seed;
          const float r = certify(p.rex[i], moved, best >= 0, swap ? d2 : d1, p.within2, p.cert_pad);
          if (r >= 0.f) {
            p.rex[i] = r;
            if (swap) {
              p.nn[i] = cand2;
              p.nn2[i] = seed;
            }
            need = false;
          }
          seed = best;
          slack = fminf(fmaxf(moved, p.slack_min), p.slack_max);
        }
      }
      // start group: the seed's; a point without a neighbour remembers the group of its cell; else locate it
      uint32_t leaf = 0;
      const bool seeded = need && seed >= 0, remembered = need && seed < 0 && cand2 <= -2;
      if (seeded) leaf = (1u << D) + (kd_leaf_rank(static_cast<uint32_t>(seed), p.kd.n, p.kd.depth, p.inv_leaf) >> p.kd.glevels);
      if (remembered) leaf = (1u << D) + min(static_cast<uint32_t>(-2 - cand2), (1u << D) - 1u);
      if (__ballot(need && !seeded && !remembered) != 0ull) {  // wave-uniform branch
        if (need && !seeded && !remembered) leaf = kd_locate(p.kd, fx, fy, fz);
      }
      const unsigned long long mask = __ballot(need);
      if (mask != 0ull) {
        if (need) {
          const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
          const int slot = (q_head + q_count + rank) & (kQueueCap - 1);
          q_pt[slot] = make_float4(fx, fy, fz, slack);
          q_idx[slot] = i;
          q_leaf[slot] = leaf;
        }
        const int added = __popcll(mask);
        if constexpr (CHECK) {
          if (lane == 0) p.walked[tile] += static_cast<uint32_t>(added);  // the tile belongs to this wave: no atomic
        }
        q_count += added;
      }
      tile++;
    }
#ifdef SGA_KD_TRIPS
    {
      const unsigned long long now = wall_clock64();
      qt_stage += now - qt_last;  // (the first iteration: the staging of the whole chunk; later ones: refills)
      qt_last = now;
    }
#endif
    // ---- lanes without a query take the next ones
    const unsigned long long idle = __ballot(!busy);
    if (q_count > 0 && idle != 0ull) {
      const int rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(idle >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(idle), 0u));
      if (!busy && rank < q_count) {
        const int slot = (q_head + rank) & (kQueueCap - 1);
        const float4 e = q_pt[slot];
        qx = e.x, qy = e.y, qz = e.z;
        qi = q_idx[slot];
        node = q_leaf[slot];
        depth = D;
        sp = 0;
        s = kd_state(p.bound2, CHECK ? e.w : 0.f);
        busy = true;
        fresh = true;
      }
      const int taken = min(__popcll(idle), q_count);
      q_head = (q_head + taken) & (kQueueCap - 1);
      q_count -= taken;
      if constexpr (CHECK) {
        // the walkers of a warm pass sit next to a surface: ring 1 of the cell grid settles nearly all of them with two dependent loads
        // (see search_lane); a lane whose query the ring settles is free again for the next one
        if (p.grid_walk & 4) {  // wave-uniform
          const bool trying = busy && fresh;
          if (__ballot(trying) != 0ull) {
            if (trying) {
              int g_nn, g_nn2;
              float g_rex, g_seen;
              bool g_face = false;
              // (a radius that ends at the ring's face with less than the walk's slack to spare is left to the walk: see certify_linearize_kernel)
              if (grid_ring1_lane(p.grid, qx, qy, qz, p.bound2, g_nn, g_nn2, g_rex, g_seen, &g_face) && !(g_face && g_nn >= 0 && (p.grid_walk & 32) && g_rex - g_seen < s.slack)) {
                p.nn[qi] = g_nn;
                p.nn2[qi] = g_nn2;
                p.rex[qi] = g_rex;
                busy = false;
                fresh = false;
              }
            }
          }
        }
      }
    }
    if (__ballot(busy) == 0ull) {
      if (tile >= tile_end && q_count == 0) break;  // (the ring may have settled every query just taken while more are queued)
      continue;
    }
    // ---- one round of the walk
    if (busy) {
      kd_descend<64>(p.kd, qx, qy, qz, s, node, depth, sp, kd_stack, lane);  // nothing to do for a fresh lane: it stands on its start group
      kd_visit_group(p.kd, node, qx, qy, qz, s);
    }
    if (__ballot(fresh) != 0ull) {  // wave-uniform
      if (fresh) {
        kd_push_path<64, kPathRecords>(p.kd, node, 0, qx, qy, qz, s, sp, kd_stack, lane);
        if (D > 2 * kPathRecords) kd_push_path<64, kKdMaxDepth / 2 - kPathRecords>(p.kd, node, 2 * kPathRecords, qx, qy, qz, s, sp, kd_stack, lane);
        fresh = false;
      }
    }
    if (busy) {
      if (!kd_pop<64>(p.kd, qx, qy, qz, s, node, depth, sp, kd_stack, lane)) {
        const KdBest nb = kd_result(s, p.bound2);
        p.nn[qi] = nb.idx;
        // no neighbour within reach: remember the group the walk ended on instead of a runner-up (the next pass starts there)
        p.nn2[qi] = nb.idx >= 0 ? nb.idx2 : -2 - static_cast<int>(node - (1u << D));
        p.rex[qi] = rex_from_r2(nb.r2);
        busy = false;
      }
    }
  }
#ifdef SGA_KD_TRIPS
  const unsigned long long qt1 = wall_clock64();
#endif
  if constexpr (FACTOR >= 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the chunk's neighbours are written
    __syncthreads();                                   // one wave: the stacks are free
    double* row = reinterpret_cast<double*>(kd_stack);
    for (int c = lane; c < kRow; c += 64) row[c] = 0.0;
    __syncthreads();
    const int limit = min(p.n, tile_end * 64);
    if (p.chunk_tiles == 1)  // (small clouds) one point per lane: no arithmetic on three absent tiles
      linearize_group<Real, FACTOR, 0, 1, true>(lp, chunk * 64 + lane, 64, limit, row, lane);
    else
      for (int t0 = chunk * p.chunk_tiles; t0 < tile_end; t0 += 4) linearize_group<Real, FACTOR, 0, 4, true>(lp, t0 * 64 + lane, 64, limit, row, lane);
    __syncthreads();
    for (int c = lane; c < kRow; c += 64) lp.partials[static_cast<size_t>(chunk) * kRow + c] = row[c];
  }
#ifdef SGA_KD_TRIPS
  if (lane == 0) {  // [12] staging, [13] walks, [14] factor stage, [15] waves; [11] latest end - earliest start is derived from the wave times
    const unsigned long long qt2 = wall_clock64();
    atomicAdd(&g_kd_trips[12], qt_stage);
    atomicAdd(&g_kd_trips[13], (qt1 - qt0) - qt_stage);
    atomicAdd(&g_kd_trips[14], qt2 - qt1);
    atomicAdd(&g_kd_trips[15], 1ull);
    if (blockIdx.x < 32768) {
      g_kd_wave_times[2 * blockIdx.x] = qt0;
      g_kd_wave_times[2 * blockIdx.x + 1] = qt2;
    }
  }
#endif
}

template <typename Real, int FACTOR, int TARGET, int PTS>
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(4))) void linearize_kernel(const LinParams<Real> p) {
  __shared__ double sh_acc[kTile / 64][kRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = lane; c < kRow; c += 64) sh_acc[wave][c] = 0.0;  // each wave owns its row: no workgroup barrier needed until the end
  double* acc_row = sh_acc[wave];

  int tile, stride, tile_end;
  tile_schedule(p.num_tiles, tile, stride, tile_end);
  for (; tile < tile_end; tile += stride) {
    linearize_group<Real, FACTOR, TARGET, PTS>(p, tile * PTS * kTile + static_cast<int>(threadIdx.x), kTile, p.n, acc_row, lane);
  }
  __syncthreads();
  if (threadIdx.x < kRow) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTile / 64; w++) t += sh_acc[w][threadIdx.x];
    if (p.tail.enabled)
      __hip_atomic_store(&p.partials[static_cast<size_t>(blockIdx.x) * kRow + threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      p.partials[static_cast<size_t>(blockIdx.x) * kRow + threadIdx.x] = t;
  }
  if (p.tail.enabled) fused_tail(p.tail, p.partials, gridDim.x, kModelCols, kRow, true);
}

// linearize_kernel over a projective search target (TARGET 3): the index's view travels as an argument of its own, behind the LinParams.
// One query per lane (PTS = 1): the lane scans its (2 h + 1) x (2 v + 1) window, column by column
template <typename Real, int FACTOR, int PTS>
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(4))) void projective_linearize_kernel(const LinParams<Real> p, const ProjView pv) {
  __shared__ double sh_acc[kTile / 64][kRow];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = lane; c < kRow; c += 64) sh_acc[wave][c] = 0.0;
  double* acc_row = sh_acc[wave];
  int tile, stride, tile_end;
  tile_schedule(p.num_tiles, tile, stride, tile_end);
  for (; tile < tile_end; tile += stride) {
    linearize_group<Real, FACTOR, 3, PTS>(p, tile * PTS * kTile + static_cast<int>(threadIdx.x), kTile, p.n, acc_row, lane, nullptr, &pv);
  }
  __syncthreads();
  if (threadIdx.x < kRow) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTile / 64; w++) t += sh_acc[w][threadIdx.x];
    if (p.tail.enabled)
      __hip_atomic_store(&p.partials[static_cast<size_t>(blockIdx.x) * kRow + threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      p.partials[static_cast<size_t>(blockIdx.x) * kRow + threadIdx.x] = t;
  }
  if (p.tail.enabled) fused_tail(p.tail, p.partials, gridDim.x, kModelCols, kRow, true);
}

// K1 of a warm pass after a small motion (large clouds): linearize_kernel with the certificate check on the way through.
// The streaming part is the factor kernel as it is (4 points per lane, everything of a stage in flight together: the kernel that reaches
// half of the HBM peak) plus, per point, the second candidate and the 12 bytes of certificate; the few points whose certificate fails are
// left out, flagged, and collected per step of 1024 points (one ballot per wave and sub-step into LDS: a fixed order).  Wave 0 of the
// workgroup then walks them, 64 at a time (seeded top-down walk with exploration slack, walk_lane), and adds their factors to its row —
// while the other workgroups stream on.  One launch, one partial row per workgroup; the old form (nn_search_queue_kernel: certificate
// check, queue-fed walks and factors per chunk of 4 tiles in one wave) streams at half this rate and stays for small clouds.
#ifndef SGA_CERT_WAVES
#define SGA_CERT_WAVES 4
#endif
template <typename Real, int FACTOR, int PTS>
__global__ __launch_bounds__(kTile) __attribute__((amdgpu_waves_per_eu(SGA_CERT_WAVES))) void certify_linearize_kernel(const LinParams<Real> p, const NNParams<Real> q_arg) {
  extern __shared__ uint32_t kd_stack[];  // 4 x tree depth x 64 words: the traversal stacks of the waves' walks
  __shared__ double sh_acc[kTile / 64][kRow];
  __shared__ unsigned long long sh_failed[kTile / 64][PTS];
  __shared__ int sh_list[PTS * kTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = lane; c < kRow; c += 64) sh_acc[wave][c] = 0.0;
  double* acc_row = sh_acc[wave];

  int tile, stride, tile_end;
  tile_schedule(p.num_tiles, tile, stride, tile_end);
  for (; tile < tile_end; tile += stride) {
    const int base = tile * PTS * kTile;
    linearize_group<Real, FACTOR, 0, PTS, false, true, true>(p, base + static_cast<int>(threadIdx.x), kTile, p.n, acc_row, lane, sh_failed[wave]);
    __syncthreads();
    {  // the walkers of this step: point of (sub-step u, wave w, lane l) = base + u * kTile + w * 64 + l; every wave counts them, wave 0 lists them
      int total = 0;
#pragma unroll
      for (int u = 0; u < PTS; u++)
#pragma unroll
        for (int w = 0; w < kTile / 64; w++) {
          const unsigned long long m = sh_failed[w][u];
          if (wave == 0 && ((m >> lane) & 1ull)) sh_list[total + __popcll(m & ((1ull << lane) - 1ull))] = base + u * kTile + w * 64 + lane;
          total += __popcll(m);
        }
      __syncthreads();
      // What the walk phase needs of the search parameters (tree, grid, certificate arrays: ~60 scalar registers) is read from the kernel
      // argument segment HERE, through a pointer the compiler cannot see through — otherwise it loads all of it at the kernel's start,
      // keeps it live across the streaming part, runs out of scalar registers and re-reads the pose of the streaming part from spilled
      // lanes (v_readlane: 720 of its 3187 vector instructions).
      using SearchArgs = const __attribute__((address_space(4))) NNParams<Real>;
      static_assert(alignof(NNParams<Real>) <= 8 && sizeof(LinParams<Real>) % 8 == 0, "kernel argument layout");
      SearchArgs* qa = (SearchArgs*)((const __attribute__((address_space(4))) char*)__builtin_amdgcn_kernarg_segment_ptr() + sizeof(LinParams<Real>));
      asm volatile("" : "+s"(qa));
      const NNParams<Real>& q = *(const NNParams<Real>*)qa;
      // spread over the four waves (entry 4 l + w of every 256 goes to lane l of wave w: a fixed assignment): four times the walks in flight
      uint32_t* my_stack = kd_stack + static_cast<size_t>(wave) * static_cast<size_t>(max(q.kd.depth, 1)) * 64;
      // A handful of walkers (the late passes of a registration): what they cost is the LATENCY of one walk, paid by the whole pass, while
      // nearly all lanes idle.  Then every walker gets a group of Gw lanes (the largest power of two that serves all of them in one
      // round: 64 lanes each for <= 4 walkers ... 2 lanes each for <= 128) which scan ring 1 together (grid_ring1_group).
      int Gw = 1;
      if ((q.grid_walk & 8) && total > 0 && total <= kTile / 2) {
        Gw = 64;
        while (Gw * total > kTile) Gw >>= 1;
      }
      const int per_round = kTile / Gw;  // walkers per round of the workgroup
      for (int k0 = 0; k0 < total; k0 += per_round) {
        const int sub = lane / Gw, gl = lane & (Gw - 1);
        const int k = k0 + 4 * sub + wave;  // (Gw = 1: entry 4 l + w of every 256 goes to lane l of wave w)
        const bool has = k < total, mine = has && gl == 0;
        const int i = has ? sh_list[k] : 0;
        Real P[1][3] = {{Real(0), Real(0), Real(0)}}, G[1][3] = {{Real(0), Real(0), Real(0)}}, E[1] = {Real(0)};
        Sym3<Real> Mp[1] = {Sym3<Real>{}};
        Sym3<Real> Mh{};
        bool inl = false;
        bool g_settled = false;
        int g_nn = -1, g_nn2 = -1;
        float g_rex = 0.f, g_seen = INFINITY;
        bool g_face = false;
        if (Gw > 1) {  // workgroup-uniform
          float gx = 0.f, gy = 0.f, gz = 0.f;
          if (has) {
            const float4 ps = p.src_pts[i];
            Real t[3];
            transform_point<Real>(p.T, Real(ps.x), Real(ps.y), Real(ps.z), t[0], t[1], t[2]);
            gx = static_cast<float>(t[0]), gy = static_cast<float>(t[1]), gz = static_cast<float>(t[2]);
          }
          g_settled = grid_ring1_group(q.grid, Gw, gl, has, gx, gy, gz, q.bound2, g_nn, g_nn2, g_rex, g_seen, &g_face);
        }
        if (mine) {
          const float4 ps = p.src_pts[i];
          P[0][0] = ps.x, P[0][1] = ps.y, P[0][2] = ps.z;
          Real t[3];
          transform_point<Real>(p.T, P[0][0], P[0][1], P[0][2], t[0], t[1], t[2]);
          const float fx = static_cast<float>(t[0]), fy = static_cast<float>(t[1]), fz = static_cast<float>(t[2]);
          // A walker of a warm pass sits next to a surface (its certificate failed by millimetres): ring 1 of the cell grid settles it
          // with a chain of two dependent loads where the seeded kd walk has a dozen, and its 27 cells give the new certificate a radius
          // of at least a cell.  The rare walker ring 1 does not settle walks the tree.
          int j = -1;
          bool settled = g_settled;
          if (Gw == 1 && (q.grid_walk & 1)) settled = grid_ring1_lane(q.grid, fx, fy, fz, q.bound2, g_nn, g_nn2, g_rex, g_seen, &g_face);  // wave-uniform condition
          // The ring's certificate ends at the face of its 27 cells at the latest, with no exploration slack: a walker whose neighbour lies
          // just inside that face would fail again in every later pass (the lone walker the last passes of a registration keep: ~5 us of
          // tail each).  Such a walker — radius set by the face, less than the re-walk's slack beyond the neighbour — walks the tree
          // once instead: the walk's radius ends at the third target point or the slack, whichever comes first.  (A radius that ends at
          // a third point is all a walk would find too: those stay with the ring.)
          if (settled && g_face && g_nn >= 0 && (q.grid_walk & 32)) {
            const float need = -__hip_atomic_load(&q.rex[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // what the check left there: the re-walk's slack
            if (g_rex - g_seen < need) settled = false;
          }
          if (settled) {
            q.nn[i] = g_nn;
            q.nn2[i] = g_nn2;
            q.rex[i] = g_rex;
            j = g_nn;
          }
          if (!settled) {
            // seed: the nearer candidate (the check put it first); slack: what the check left in rex[] — both written by this workgroup
            const int seed = __hip_atomic_load(&q.nn[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float slack = -__hip_atomic_load(&q.rex[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            j = walk_lane<Real, 64>(q, i, fx, fy, fz, seed, slack, my_stack, lane);
          }
          if (j >= 0) {
            const float4 m = p.tgt_pts[j];
            const bool within = kd_dist2(m.x, m.y, m.z, fx, fy, fz) < p.bound2;
            inl = pair_moments<Real, FACTOR>(p, i, j, within, t[0], t[1], t[2], Real(m.x), Real(m.y), Real(m.z), Mp[0], G[0], E[0], Mh);
          }
          p.corr[i] = inl ? j : -1;
          if constexpr (FACTOR == SGA_GICP) {
            if (inl && p.store_maha) {
              Real* mm = p.maha + static_cast<size_t>(i) * 6;
              mm[0] = Mh.xx, mm[1] = Mh.xy, mm[2] = Mh.xz, mm[3] = Mh.yy, mm[4] = Mh.yz, mm[5] = Mh.zz;
            }
          }
        }
        const int inliers = __popcll(__ballot(inl));
        if (inliers > 0) accumulate_moments<Real, 1>(P, Mp, G, E, inliers, acc_row, lane);
      }
    }
    __syncthreads();  // (sh_failed / sh_list are reused by the next step)
  }
  __syncthreads();
  if (threadIdx.x < kRow) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < kTile / 64; w++) t += sh_acc[w][threadIdx.x];
    if (p.tail.enabled)
      __hip_atomic_store(&p.partials[static_cast<size_t>(blockIdx.x) * kRow + threadIdx.x], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      p.partials[static_cast<size_t>(blockIdx.x) * kRow + threadIdx.x] = t;
  }
  if (p.tail.enabled) fused_tail(p.tail, p.partials, gridDim.x, kModelCols, kRow, true);  // small grids: the last workgroup adds the rows and hands the result over
}

// K1, fused: the search wave also evaluates the factors of its own 64 source points — their neighbours are in registers, no nn[]
// round trip, no second kernel whose start waits for the slowest search wave.  The factor algebra in moment form is lean enough
// (42 VGPRs at one point per lane) to live inside the search kernel's register budget (72 VGPRs for 7 waves per SIMD, which the walks need).
// One partial row per wave (= per tile of 64 points, whatever workgroup took it: the row order, and with it the fp64 sum, does not
// depend on the placement).  The row is built in the LDS the traversal stacks occupied.
// 7 waves per SIMD (72 VGPRs): as fast as 8 (64 VGPRs; measured 179 / 190 / 200 against 182 / 185 / 198 us for the cold passes of a C3
// registration) and without the two registers the 64-VGPR build spills around the walk (20 bytes per lane through scratch memory =
// 2 x 20 MB of HBM traffic per cold pass).
// The warm form (CHECK: certificate check, ring 1 of the cell grid for the walkers, then the walk) needs 16 registers more: at 7 waves it
// spills them around the walk (68 bytes per lane through scratch = 2 x 68 MB of HBM traffic per pass of 1M points, rocprofv3 FETCH_SIZE /
// WRITE_SIZE), at 6 waves per SIMD (80 VGPRs) it does not.
#ifndef SGA_SL_WAVES
#define SGA_SL_WAVES 7
#endif
#ifndef SGA_SL_WAVES_WARM
#define SGA_SL_WAVES_WARM 6
#endif
template <typename Real, int FACTOR, bool CHECK>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(CHECK ? SGA_SL_WAVES_WARM : SGA_SL_WAVES, CHECK ? SGA_SL_WAVES_WARM : SGA_SL_WAVES))) void search_linearize_kernel(const NNParams<Real> p, const LinParams<Real> lp) {
  extern __shared__ uint32_t kd_stack[];  // max(tree depth, 3) x 64 words: the traversal stacks, then the wave's row of kRow doubles
#ifdef SGA_KD_TRIPS
  const unsigned long long wave_t0 = wall_clock64();
#endif
  const int lane = threadIdx.x;
  const int slot = search_tile_of_block();
  const int tile = p.tile_order != nullptr ? static_cast<int>(p.tile_order[slot]) : slot;  // wave-uniform
  const unsigned long long cost_t0 = p.tile_cost != nullptr ? wall_clock64() : 0ull;
  const int i = tile * 64 + lane;
  const bool active = i < p.n;
  const float4 ps = active ? p.src_pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  Real q[3] = {Real(0), Real(0), Real(0)};
  int j = -1;
  if (active) {
    transform_point<Real>(p.T, ps.x, ps.y, ps.z, q[0], q[1], q[2]);
    j = search_lane<Real, 64, CHECK>(p, tile, i, ps, static_cast<float>(q[0]), static_cast<float>(q[1]), static_cast<float>(q[2]), kd_stack);
  }
  // ---- the factors of the wave's 64 points (linearize_kernel with one point per lane)
  Real P[1][3] = {{ps.x, ps.y, ps.z}}, G[1][3] = {{Real(0), Real(0), Real(0)}}, E[1] = {Real(0)};
  Sym3<Real> Mp[1] = {Sym3<Real>{}};
  Sym3<Real> Mh{};
  bool inl = false;
  if (j >= 0) {
    const float4 m = lp.tgt_pts[j];
    // the search reaches a little beyond the rejector (kSearchMargin) and a certified neighbour may have drifted out of reach: a
    // neighbour counts only inside the reach of a plain search, whichever way it was found
    const bool within = kd_dist2(m.x, m.y, m.z, static_cast<float>(q[0]), static_cast<float>(q[1]), static_cast<float>(q[2])) < lp.bound2;
    inl = pair_moments<Real, FACTOR>(lp, i, j, within, q[0], q[1], q[2], Real(m.x), Real(m.y), Real(m.z), Mp[0], G[0], E[0], Mh);
  }
  if (active) {
    lp.corr[i] = inl ? j : -1;
    if constexpr (FACTOR == SGA_GICP) {
      if (inl && lp.store_maha) {
        Real* mm = lp.maha + static_cast<size_t>(i) * 6;
        mm[0] = Mh.xx, mm[1] = Mh.xy, mm[2] = Mh.xz, mm[3] = Mh.yy, mm[4] = Mh.yz, mm[5] = Mh.zz;
      }
    }
  }
  const int inliers = __popcll(__ballot(inl));
  __syncthreads();  // one wave: every lane is done with its stack
  double* row = reinterpret_cast<double*>(kd_stack);
  for (int c = lane; c < kRow; c += 64) row[c] = 0.0;
  __syncthreads();
  if (inliers > 0) accumulate_moments<Real, 1>(P, Mp, G, E, inliers, row, lane);
  __syncthreads();
  for (int c = lane; c < kRow; c += 64) lp.partials[static_cast<size_t>(tile) * kRow + c] = row[c];
  if (p.tile_cost != nullptr && lane == 0) p.tile_cost[tile] = static_cast<uint32_t>(wall_clock64() - cost_t0);
#ifdef SGA_KD_TRIPS
  if (blockIdx.x < 32768 && lane == 0) {
    g_kd_wave_times[2 * blockIdx.x] = wave_t0;
    g_kd_wave_times[2 * blockIdx.x + 1] = wall_clock64();
  }
#endif
}

// (uniform_const: uniform.hpp — a wave-uniform pointer into memory that nothing writes while the kernel runs, read with scalar loads)

// search_linearize_kernel (cold) for the tiles of all active pairs in one grid.  Workgroup (= wave) b belongs to the pair k with
// prefix[k] <= b < prefix[k + 1]; every pair's share of the grid is padded to a multiple of 8 so that — workgroup b runs on XCD b % 8 —
// each XCD gets one contiguous eighth of the pair's (spatially sorted) tiles, as search_tile_of_block arranges for a lone pass; the
// waves of the padding leave at once.  The row of a tile goes to the pair's own partials at the tile's LOCAL number: neither the
// placement nor the company a pair keeps enters any sum.
template <int FACTOR>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SGA_SL_WAVES, SGA_SL_WAVES))) void batch_search_linearize_kernel(const int* __restrict__ prefix_g, const BatchPair* __restrict__ pairs_g, int nactive) {
  extern __shared__ uint32_t kd_stack[];  // max(deepest tree of the batch, 3) x 64 words: the traversal stacks, then the wave's row of kRow doubles
  const int lane = threadIdx.x;
  const int* prefix = uniform_const(prefix_g);
  const int b = blockIdx.x;
  int lo = 0, hi = nactive;  // wave-uniform binary search
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b)
      lo = mid;
    else
      hi = mid;
  }
  const int first = prefix[lo], per_xcd = (prefix[lo + 1] - first) >> 3, slot = b - first;
  const int tile = (slot & 7) * per_xcd + (slot >> 3);
  const BatchPair& d = *uniform_const(pairs_g + lo);
  if (tile >= d.ntiles) return;  // wave-uniform
  const NNParams<float>& p = d.q;
  const LinParams<float>& lp = d.p;
  const int i = tile * 64 + lane;
  const bool active = i < p.n;
  const float4 ps = active ? p.src_pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  float q[3] = {0.f, 0.f, 0.f};
  int j = -1;
  if (active) {
    transform_point<float>(p.T, ps.x, ps.y, ps.z, q[0], q[1], q[2]);
    const int seed = d.seedless ? -1 : p.nn[i];  // (the cold form of search_lane)
    j = walk_lane<float, 64>(p, i, q[0], q[1], q[2], seed, 0.f, kd_stack, lane);
  }
  // ---- the factors of the wave's 64 points, exactly as in search_linearize_kernel
  float P[1][3] = {{ps.x, ps.y, ps.z}}, G[1][3] = {{0.f, 0.f, 0.f}}, E[1] = {0.f};
  Sym3<float> Mp[1] = {Sym3<float>{}};
  Sym3<float> Mh{};
  bool inl = false;
  if (j >= 0) {
    const float4 m = lp.tgt_pts[j];
    const bool within = kd_dist2(m.x, m.y, m.z, q[0], q[1], q[2]) < lp.bound2;
    inl = pair_moments<float, FACTOR>(lp, i, j, within, q[0], q[1], q[2], m.x, m.y, m.z, Mp[0], G[0], E[0], Mh);
  }
  if (active) lp.corr[i] = inl ? j : -1;  // (the mahalanobis matrices are recomputed if ever asked for: problem_ensure_maha)
  const int inliers = __popcll(__ballot(inl));
  __syncthreads();  // one wave: every lane is done with its stack
  double* row = reinterpret_cast<double*>(kd_stack);
  for (int c = lane; c < kRow; c += 64) row[c] = 0.0;
  __syncthreads();
  if (inliers > 0) accumulate_moments<float, 1>(P, Mp, G, E, inliers, row, lane);
  __syncthreads();
  for (int c = lane; c < kRow; c += 64) lp.partials[static_cast<size_t>(tile) * kRow + c] = row[c];
}

// linearize_kernel<float, FACTOR, TARGET, 1> (TARGET 1: Gaussian voxel map, 2: flat map; the lookup happens inside linearize_group) for
// the tiles of all active pairs in one grid: the round table, the padding of every pair's share to a multiple of 8, the XCD-striped tile
// numbering and the row at the tile's LOCAL number in the pair's own partials are batch_search_linearize_kernel's, so the reduction is
// shared.  (The pair lookup is a second copy on purpose: as a shared device function it would be free to move the kd kernel's registers.)
// The pair's LinParams — the map's hash, leaf size, origin and search offsets among them — are read per wave with scalar loads: maps of
// different leaf size and offsets share a launch, and `offsets` stays wave-uniform.  No walk, no traversal stack: the LDS is the row.
// Occupancy: a round of 32 C5-shaped pairs is ~5 600 waves on 1 024 SIMDs and a wave lasts a few microseconds, so more than 5 - 6 waves
// are never resident on a SIMD; 4 (the lone factor kernel's floor, <= 128 VGPRs) leaves the allocator twice the ~70 registers the
// one-point-per-lane factor stage needs, and the 768 bytes of LDS per wave limit nothing.
template <int FACTOR, int TARGET>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void batch_map_linearize_kernel(const int* __restrict__ prefix_g, const BatchPair* __restrict__ pairs_g, int nactive) {
  static_assert(TARGET == 1 || TARGET == 2, "voxel-map targets");
  __shared__ double row[kRow];
  const int lane = threadIdx.x;
  const int* prefix = uniform_const(prefix_g);
  const int b = blockIdx.x;
  int lo = 0, hi = nactive;  // wave-uniform binary search
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (prefix[mid] <= b)
      lo = mid;
    else
      hi = mid;
  }
  const int first = prefix[lo], per_xcd = (prefix[lo + 1] - first) >> 3, slot = b - first;
  const int tile = (slot & 7) * per_xcd + (slot >> 3);
  const BatchPair& d = *uniform_const(pairs_g + lo);
  if (tile >= d.ntiles) return;  // wave-uniform
  const LinParams<float>& lp = d.p;
  for (int c = lane; c < kRow; c += 64) row[c] = 0.0;
  __syncthreads();
  linearize_group<float, FACTOR, TARGET, 1>(lp, tile * 64 + lane, 64, lp.n, row, lane);
  __syncthreads();
  for (int c = lane; c < kRow; c += 64) lp.partials[static_cast<size_t>(tile) * kRow + c] = row[c];
}

// Per-point export of the same factors (the reference's Python binding exposes Factor::linearize per source point,
// src/python/factors.cpp:52-101): the 28 values of every pair instead of their sum.  Runs after a linearize pass at the same pose over
// the correspondences that pass kept in corr[] (kd position or flat-map slot, -1 = none): the pass has decided every pair — the double
// re-decision between the walk's two candidates, the rejector's distance test or the host rejector's verdicts — so the export neither
// searches nor rejects again, and the matrix pair_factor caches is the pass's own.  Not on the hot path.
//
// The residual is formed without the rounding of q = R p + t: a point that lies ON its target's plane has |n . r| of 1e-5 m where q, 50 m
// from the origin, is rounded by 1e-14 m — 1e-9 of the point-to-plane b_i and e_i.  t_j - t - sum R_ak p_k is accumulated as hi + lo with
// error-free products (fma) and sums, so r carries the rounding of its own size only.
__device__ __forceinline__ void exact_add(double& hi, double& lo, double x) {  // hi + lo + x, hi + x exactly (Knuth's two-sum)
  const double s = hi + x, b = s - hi;
  lo += (hi - (s - b)) + (x - b);
  hi = s;
}
__device__ __forceinline__ double exact_residual(double tj, double t, double r0, double r1, double r2, double x, double y, double z) {
  double hi = tj, lo = 0.0;
  exact_add(hi, lo, -t);
  const double a[3] = {-r0, -r1, -r2}, v[3] = {x, y, z};
#pragma unroll
  for (int k = 0; k < 3; k++) {
    double prod = a[k] * v[k];
    // the rounded product as a value of its own: built with -ffp-contract=fast, the compiler would otherwise fuse it into the sum that
    // follows, which then no longer adds the product whose rounding lo holds
    asm volatile("" : "+v"(prod));
    lo += fma(a[k], v[k], -prod);  // the product's own rounding
    exact_add(hi, lo, prod);
  }
  return hi + lo;
}
template <typename Real, int FACTOR>
__global__ __launch_bounds__(256) void per_point_kernel(const LinParams<Real> p, double* __restrict__ out28, unsigned char* __restrict__ ok) {
  static_assert(sizeof(Real) == 8, "the export is double");
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  const float4 ps4 = p.src_pts[i];
  const Real px = ps4.x, py = ps4.y, pz = ps4.z;
  Real vals[28];
#pragma unroll
  for (int k = 0; k < 28; k++) vals[k] = Real(0);
  const int j = p.corr[i];
  Real rx = 0, ry = 0, rz = 0;
  if (j >= 0) {
    const float4 m = p.tgt_pts[j];
    const Real* R = p.T.r;
    rx = exact_residual(m.x, p.T.t[0], R[0], R[1], R[2], px, py, pz);
    ry = exact_residual(m.y, p.T.t[1], R[3], R[4], R[5], px, py, pz);
    rz = exact_residual(m.z, p.T.t[2], R[6], R[7], R[8], px, py, pz);
  }
  const bool inlier = pair_factor<Real, FACTOR>(p, i, j, px, py, pz, rx, ry, rz, vals);
  const uint32_t orig = __float_as_uint(ps4.w);  // the caller's source order
  ok[orig] = inlier ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 28; k++) out28[static_cast<size_t>(orig) * 28 + k] = static_cast<double>(vals[k]);
}

template <typename Real, int FACTOR>
__global__ __launch_bounds__(kTile) void error_kernel(const ErrParams<Real> p) {
  __shared__ double sh_e[kTile / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  int tile, stride, tile_end;
  tile_schedule(p.num_tiles, tile, stride, tile_end);
  for (; tile < tile_end; tile += stride) {
    const int i = tile * kTile + threadIdx.x;
    Real e = Real(0);
    if (i < p.n) {
      const int j = p.corr[i];
      if (j >= 0) {
        const float4 ps4 = p.src_pts[i];
        Real qx, qy, qz;
        transform_point<Real>(p.T, ps4.x, ps4.y, ps4.z, qx, qy, qz);
        const float4 t4 = p.tgt_pts[j];
        const Real rx = Real(t4.x) - qx, ry = Real(t4.y) - qy, rz = Real(t4.z) - qz;
        if constexpr (FACTOR == SGA_GICP) {
          const Real* m = p.maha + static_cast<size_t>(i) * 6;
          const Real vx = m[0] * rx + m[1] * ry + m[2] * rz, vy = m[1] * rx + m[3] * ry + m[4] * rz, vz = m[2] * rx + m[4] * ry + m[5] * rz;
          e = Real(0.5) * (rx * vx + ry * vy + rz * vz);
        } else if constexpr (FACTOR == SGA_PLANE_ICP) {
          const float4 nn = p.tgt_nrm[j];
          // same association as pair_system's 1/2 r^T diag(n^2) r
          e = Real(0.5) * (rx * (Real(nn.x) * Real(nn.x) * rx) + ry * (Real(nn.y) * Real(nn.y) * ry) + rz * (Real(nn.z) * Real(nn.z) * rz));
        } else {
          e = Real(0.5) * (rx * rx + ry * ry + rz * rz);
        }
        if (p.robust_kind != SGA_ROBUST_NONE) e *= robust_weight<Real>(p.robust_kind, p.robust_c, e);
      }
    }
    acc += wave_sum_f64(static_cast<double>(e));
  }
  if (lane == 0) sh_e[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
    for (int w = 0; w < kTile / 64; w++) s += sh_e[w];
    if (p.tail.enabled)
      __hip_atomic_store(&p.partials[blockIdx.x], s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else
      p.partials[blockIdx.x] = s;
  }
  if (p.tail.enabled) fused_tail(p.tail, p.partials, gridDim.x, 1, 1);
}

// Longest tile first.  A pass of the one-query-per-lane kernel is 1.9 rounds of waves, and 35 - 40 % of it is the drain of the waves
// that happened to start last and run long.  Which tiles run long is only known afterwards — but after a small
// motion the next pass's costs resemble this one's (correlation 0.9 at <= 0.1 m, scripts/diag_lpt.py).  This kernel sorts the tiles of
// every XCD's share (search_tile_of_block: slot s of XCD x is its (s - x * per_xcd)-th workgroup to start) by the duration their
// wave just recorded, longest first: a counting sort over 64 duration classes of 2.56 us, one workgroup per XCD.  The order within a class is
// whatever the LDS atomics make it: nothing but speed depends on the launch order (rows are indexed by tile).
__global__ __launch_bounds__(1024) void tile_order_kernel(const uint32_t* __restrict__ cost, uint32_t* __restrict__ order, int num_tiles) {
  __shared__ uint32_t hist[64], start[64];
  const int per_xcd = num_tiles >> 3;
  const int x = blockIdx.x, first = x * per_xcd;
  if (threadIdx.x < 64) hist[threadIdx.x] = 0u;
  __syncthreads();
  for (int k = threadIdx.x; k < per_xcd; k += blockDim.x) atomicAdd(&hist[63u - min(63u, cost[first + k] >> 8)], 1u);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t acc = 0u;
    for (int b = 0; b < 64; b++) {
      start[b] = acc;
      acc += hist[b];
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < per_xcd; k += blockDim.x) {
    const uint32_t pos = atomicAdd(&start[63u - min(63u, cost[first + k] >> 8)], 1u);
    order[first + pos] = static_cast<uint32_t>(first + k);
  }
  if (x == 0)
    for (int t = 8 * per_xcd + threadIdx.x; t < num_tiles; t += blockDim.x) order[t] = static_cast<uint32_t>(t);  // the (< 8) tiles beyond the XCD shares
}

// ---- the tuning table of the pass routing ------------------------------------------------------------------------------------------
// Every threshold linearize_dispatch routes by, lengths in metres at the reference spacing (routing_unit); none changes a result, only
// which exact kernel computes it.  The switches tests or exported setters change are read when the library loads.
template <typename T>
static T env_or(const char* name, T d) {  // the environment variable `name` as a T, or d if it is not set
  const char* s = getenv(name);
  return s == nullptr ? d : std::is_floating_point_v<T> ? static_cast<T>(atof(s)) : static_cast<T>(atoll(s));
}

// Points per lane and reduction (linearize_kernel's PTS): large clouds amortise the wave reductions over 4 points; small ones (a
// 15k-point scan) keep one point per lane — they are bound by latency and want every workgroup they can get.  Four per lane from
// kLinPtsMin points on (VGICP iterations of 140k / 200k / 300k / 500k / 1M points: 32.5 / 32.7 / 36.4 / 39.0 / 45.1 us at four per lane
// against 25.5 / 27.0 / 30.4 / 37.0 / 45.4 us at one: the size sweep late in round 6; 131072 before).
constexpr int kLinPts = 4;
constexpr int kLinPtsMin = 750000;
// (fp64 per-pair arithmetic keeps four per lane from 131 072 points on: its factor kernel is arithmetic-bound and loses a quarter of its rate at one —
// 200k / 400k / 700k / 1M points 11 047 / 9 236 / 6 768 / 5 389 against 9 632 / 7 069 / 4 921 / 3 673 iterations/s)
constexpr int kLinPtsMinF64 = 131072;

// A pass runs warm (certified neighbours skip the walk) while no source point can have moved farther than this since the previous
// linearization; beyond it hardly any certificate holds and checking them is wasted work.  Environment override SGA_WARM_DELTA,
// run-time override sga_set_warm_limit; negative = never.
static double g_warm_delta = env_or("SGA_WARM_DELTA", 0.1);

// Search kernel selection.  SGA_SEARCH_QUEUE: 0 = one query per lane always (nn_search_kernel), 1 = queue-fed always, 2 (default) =
// queue-fed for warm passes after a motion of at most kQueueDelta.  Measured on C3 (1 M points): when most lanes walk (cold passes,
// the first warm pass) a wave per 64 queries and 8 waves per SIMD win — the walks are bound by the number of memory accesses in flight
// and the queue-fed kernel starts each of them with 10 record fetches; when few lanes walk (the later passes of a registration) the
// queue packs them into full waves: 124 -> 80, 87 -> 73, 68 -> 53 us.
static int g_search_queue = env_or("SGA_SEARCH_QUEUE", 2);
constexpr double kQueueDelta = 0.02;
// tiles of 64 queries per wave of the queue-fed kernel (SGA_CHUNK_COLD / SGA_CHUNK_WARM, sga_set_search_mode)
static int g_chunk_tiles_cold = env_or("SGA_CHUNK_COLD", 4);
static int g_chunk_tiles_warm = env_or("SGA_CHUNK_WARM", 4);

// Warm pass of a large cloud after a small motion: the certificates are checked inside the streaming factor kernel
// (certify_linearize_kernel), whose workgroups walk their few failed points themselves.  Measured on C3 (profiles/r04_warm_split.txt):
// it wins where few points walk (after motions of a millimetre or two: 38 - 54 us against 44 - 66) and loses where many do (the walkers
// of a pass sit where the points moved most, i.e. in a few workgroups, which then walk alone: 121 against 99 us after a 1 cm motion),
// hence a second limit, smaller than kQueueDelta.
constexpr double kSplitDelta = 0.002;
// Only from this many source points on (131072 until the size sweep late in round 6: late passes of 135k / 200k / 300k / 400k /
// 600k-point pairs 27.3 / 29.1 / 33.8 / 35.0 / 41.0 us with this kernel against 24.6 / 26.6 / 34.2 / 38.5 / 43.2 us with the queue-fed
// one: the crossover is near 300k): measured on C2 (100k points) and C5 (12k-point scans) the kernel — one point per lane there, the
// row reduction folded into it (fused_tail) when the grid is small — is no faster than the queue-fed one (C2 warm pass 39.9 against
// 40.3 us, C5 registration 0.51 against 0.48 ms/scan; with 4 points per lane 53.9 us): at those sizes a pass is a chain of launch, a
// few dependent loads and the hand-off, whichever kernel runs it.  One point per lane at every size: the size sweep late in round 6 —
// late passes of 300k / 600k / 700k-point pairs 34.0 / 40.4 / 42.3 us at four per lane against 31.2 / 38.8 / 40.6 us at one, C3's warm
// passes 83.8 -> 81.2 us on average (+1.2 % on the headline).
constexpr size_t kSplitMinPoints = 262144;

// exploration slack of a re-walk = clamp(motion, kSlackMin, kSlackMax)
constexpr float kSlackMin = 3e-4f, kSlackMax = 0.02f;
// headroom of the certificate check (certify): a point walks unless its certificate survives PAD x its own motion beyond what this pass needs
static const float g_cert_pad = env_or("SGA_CERT_PAD", 0.6f);
// longest tile first (tile_order_kernel): 0 off, 1 = warm passes of the one-query-per-lane kernel (motion <= SGA_WARM_DELTA) when the
// previous pass was such a pass too, 2 = every pass of that kernel that follows another (experiments)
static const int g_lpt = env_or("SGA_LPT", 1);
// 1 (default): the one-query-per-lane search kernels walk with the fast leaf scan (32-bit keys, packed fp32; exact repeat of the
// queries it cannot decide); 0: the exact 64-bit keys throughout.
static const int g_fast_scan = env_or("SGA_FAST_SCAN", 1);

// The cell grid (cell_grid.hpp).  SGA_GRID: 0 no grid at all; 1 (default) the WALKERS of warm passes try ring 1 of the grid before they
// walk the tree (certify_linearize_kernel) and every full search stays with the kd walk — measured on C3 whole grid passes do not beat
// it; 2 = also the cold passes of a registration but its first (whose queries lie as far from the target as the
// initial guess is off: there the kd walk's pruning pays) and the warm passes after a larger motion; 3 the first pass too; 4 every pass.
// Whole grid passes only while the reach needs at most kGridMaxRings rings; if ring 1 of the last grid pass left more than kGridMaxOpen
// of the queries open, the next cold pass walks the kd-tree instead.
int g_grid_mode = env_or("SGA_GRID", 1);  // sga_set_grid_mode
long long g_grid_min_points = env_or("SGA_GRID_MIN_POINTS", 65536ll);  // targets below this get no grid (cell_grid.hip)
constexpr int kGridMaxRings = 16;
constexpr double kGridMaxOpen = 0.5;
// which walkers try ring 1 of the grid first (SGA_GRID_WALK, bits): 1 those of certify_linearize_kernel, 2 those of the
// one-query-per-lane warm pass (search_linearize_kernel<CHECK>), 4 those of the queue-fed kernel, 8 certify_linearize_kernel scans ring 1
// with a group of lanes per walker when a workgroup has few of them (grid_ring1_group); 32: a ring certificate that ends at the ring's
// face with less than the re-walk's slack beyond the neighbour is left to the tree walk (the margin rule, certify_linearize_kernel)
static const int g_grid_walk = env_or("SGA_GRID_WALK", 47);

// trial errors from the quadratic error model of the last linearization; 0 (SGA_ERROR_MODEL, sga_set_error_model) = every error pass
// runs the error kernel (the reference's literal procedure)
static bool g_error_model = env_or("SGA_ERROR_MODEL", true);

static int grid_blocks(int num_tiles) { return num_tiles < kMaxBlocks ? (num_tiles < 1 ? 1 : num_tiles) : kMaxBlocks; }
static int factor_tiles(int n, int pts) { return (n + kTile * pts - 1) / (kTile * pts); }  // steps of kTile * pts points
static int linearize_pts(int n, bool fp64) { return n >= (fp64 ? kLinPtsMinF64 : kLinPtsMin) ? kLinPts : 1; }

// nearest neighbour (caller's target order) and squared distance of every source point in the caller's source order: the input of a
// host rejector callback
template <typename Real>
__global__ void export_neighbours_kernel(const float4* __restrict__ src_pts, const int* __restrict__ nn, int n, const float4* __restrict__ tgt_pts, Rigid<Real> T, long long* __restrict__ out_idx, float* __restrict__ out_d2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 ps = src_pts[i];
  const uint32_t orig = __float_as_uint(ps.w);
  const int j = nn[i];
  long long t = -1;
  float d2 = INFINITY;
  if (j >= 0) {
    Real x, y, z;
    transform_point<Real>(T, ps.x, ps.y, ps.z, x, y, z);
    const float4 m = tgt_pts[j];
    t = static_cast<long long>(__float_as_uint(m.w));
    d2 = kd_dist2(m.x, m.y, m.z, static_cast<float>(x), static_cast<float>(y), static_cast<float>(z));
  }
  out_idx[orig] = t;
  out_d2[orig] = d2;
}

// f(std::integral_constant<int, K>{}) for factor kind K; the caller has validated the kind
template <typename F>
static void with_factor(int kind, F&& f) {
  switch (kind) {
    case SGA_GICP: f(std::integral_constant<int, SGA_GICP>{}); break;
    case SGA_PLANE_ICP: f(std::integral_constant<int, SGA_PLANE_ICP>{}); break;
    default: f(std::integral_constant<int, SGA_ICP>{}); break;
  }
}

template <typename Real, int FACTOR, int TARGET>
static void launch_linearize(hipStream_t st, const LinParams<Real>& p, int blocks, int pts) {
  if (pts == kLinPts)
    hipLaunchKernelGGL((linearize_kernel<Real, FACTOR, TARGET, kLinPts>), dim3(blocks), dim3(kTile), 0, st, p);
  else
    hipLaunchKernelGGL((linearize_kernel<Real, FACTOR, TARGET, 1>), dim3(blocks), dim3(kTile), 0, st, p);
}

// Largest displacement |Ta p - Tb p| over the box [lo, hi] (column-major 4x4 poses): the norm of an affine map is convex, so the
// maximum sits at a corner.
static double max_displacement(const double Ta[16], const double Tb[16], const float lo[3], const float hi[3]) {
  double best = 0.0;
  for (int c = 0; c < 8; c++) {
    const double x = (c & 1) ? hi[0] : lo[0], y = (c & 2) ? hi[1] : lo[1], z = (c & 4) ? hi[2] : lo[2];
    double s = 0.0;
    for (int r = 0; r < 3; r++) {
      const double d = (Ta[r] - Tb[r]) * x + (Ta[4 + r] - Tb[4 + r]) * y + (Ta[8 + r] - Tb[8 + r]) * z + (Ta[12 + r] - Tb[12 + r]);
      s += d * d;
    }
    best = std::max(best, s);
  }
  return std::sqrt(best);
}

// The lengths the pass routing compares motions with are properties of the TARGET, not constants of nature: a certificate's exclusion
// radius is a fraction of the distance between neighbouring target points, so "how far may the source have moved before the
// certificates are gone" scales with the target's spacing.  The thresholds above were tuned in metres on the C3 scene; they are applied
// multiplied by  unit = (the target's length scale) / kSpacingRef  — index_spacing(): the geometric mean of the tree's leaf diagonals,
// computed by the build (kd_tail_kernel); kSpacingRef: that number for the C3 target — so a cloud in millimetres, or one ten times sparser,
// routes its passes exactly as its metre-scale twin does (tests/test_scale_free.py).  unit = 1 while the length scale of a
// target is not known (only ever before the first result of a problem has come back: the first pass is cold anyway).
constexpr double kSpacingRef = SGA_SPACING_REF;
double index_spacing(const sga_index* idx);  // index_build.hip
ProjView make_proj_view(const sga_index* idx);  // projective.hip
static double routing_unit(const sga_index* idx) {
  const double s = index_spacing(idx);
  return s > 0.0 ? s / kSpacingRef : 1.0;
}

// Which kernels run a pass, in the order plan_pass decides it
enum class Route {
  kFactors,     // no search: a voxel-map target (the lookup happens inside linearize_kernel) or an empty source
  kGrid,        // a whole search pass over the target's cell grid (grid_search_pass), then linearize_kernel over nn[]
  kCertify,     // certify_linearize_kernel: the certificates checked inside the streaming factor kernel, which walks the failed points
  kFusedLane,   // search_linearize_kernel: one query per lane, every wave evaluates the factors of its own tile
  kFusedQueue,  // nn_search_queue_kernel<FACTOR>: queue-fed walks, every wave evaluates the factors of its chunk
  kQueue,       // nn_search_queue_kernel, then linearize_kernel
  kLane,        // nn_search_kernel (one query per lane), then linearize_kernel
};

struct PassPlan {
  Route route = Route::kFactors;
  bool warm = false;          // the certificates of the previous pass are checked (a grid pass searches every point: cold)
  bool grid = false;          // the target's cell grid serves the pass: ring 1 for the walkers (SGA_GRID_WALK), or all of it (kGrid)
  int pts = 1;                // points per lane of the kernel that evaluates the factors by tiles: linearize_kernel, or 1 in certify
  bool tail = false;          // that kernel also sums the rows (FusedTail); otherwise reduce_rows_kernel follows
  bool order_record = false;  // kFusedLane: the waves record their durations, sorted afterwards (longest tile first, tile_order_kernel) ...
  bool order_use = false;     // ... and the tiles start in the order the previous pass recorded
  int chunk_tiles = 0;        // kQueue / kFusedQueue: tiles per wave
  bool fused() const { return route == Route::kCertify || route == Route::kFusedLane || route == Route::kFusedQueue; }
};

// The routing of one pass.  displacement: how far a source point can have moved since the previous pass (INFINITY: no previous pass
// in the same arithmetic); unit: routing_unit.  Reads the problem, the target and the tuning table: no HIP call, no write.
template <typename Real>
static PassPlan plan_pass(const sga_context* ctx, const sga_problem* pb, const NNParams<Real>& q, double displacement, double unit, bool host_rejector) {
  const sga_index* idx = pb->target;
  PassPlan pl;
  pl.warm = displacement <= g_warm_delta * unit;
  pl.pts = linearize_pts(q.n, sizeof(Real) == 8);
  if (idx->kind == SGA_INDEX_PROJECTIVE) pl.pts = 1;  // the window scan is the work: four points per lane would only spill
  if (q.n > 0 && idx->kind == SGA_INDEX_KDTREE) {
    const bool small_warm = pl.warm && displacement <= kQueueDelta * unit;
    const bool fuse = sizeof(Real) == 4 && !host_rejector;  // fp64 math: the fused kernels would spill (they exist for float only)
    const int search_tiles = (q.n + kSearchBlock - 1) / kSearchBlock;
    pl.grid = g_grid_mode != 0 && idx->grid_h > 0.f && q.bound2 < 3.0e38f && !host_rejector && q.leaves == nullptr;
    bool use_grid = false;
    if (pl.grid) {
      const int rings = grid_rings_for(idx, std::sqrt(static_cast<double>(q.bound2)));
      const bool first_pass = !pb->prev_valid;
      use_grid = g_grid_mode >= 2 && rings > 0 && rings <= kGridMaxRings &&
                 (g_grid_mode >= 4 || (!small_warm && (g_grid_mode == 3 || (!first_pass && pb->grid_open_frac <= kGridMaxOpen))));
    }
    const bool queue = g_search_queue == 1 || (g_search_queue == 2 && small_warm);
    if (use_grid) {
      pl.route = Route::kGrid;
      pl.warm = false;
    } else if (g_search_queue == 2 && small_warm && displacement <= kSplitDelta * unit && fuse && pb->n >= kSplitMinPoints && q.leaves == nullptr) {
      pl.route = Route::kCertify;
      pl.pts = 1;
    } else if (fuse && !queue) {
      pl.route = Route::kFusedLane;
      pl.order_record = g_lpt != 0 && search_tiles >= 8192;  // fewer tiles than wave slots: all waves start at once, the order means nothing
      // (the order was written behind the previous pass's hand-off on that pass's stream: a pass issued on another stream could read it half-written)
      pl.order_use = pl.order_record && pb->order_tiles == static_cast<unsigned>(search_tiles) && pb->order_stream == ctx->stream && (g_lpt == 2 || pl.warm);
    } else if (queue) {
      pl.route = fuse && pl.warm ? Route::kFusedQueue : Route::kQueue;
      pl.chunk_tiles = std::max(1, pl.warm ? g_chunk_tiles_warm : g_chunk_tiles_cold);
      // a wave works through its chunk serially (two dependent round trips per tile): small clouds get shorter chunks, down to one tile,
      // as long as that leaves no more than ~4 waves per SIMD (kWaveSlots4 = 256 CUs x 4 SIMDs x 4); C3 keeps its 4 tiles
      if (pl.warm) pl.chunk_tiles = std::min(pl.chunk_tiles, std::max(1, (search_tiles + 4095) / 4096));
    } else {
      pl.route = Route::kLane;
    }
  }
  // the search kernels that evaluate the factors leave one row per tile or chunk: reduce_rows_kernel sums them.  (certify: never at its
  // sizes since kFuseMaxBlocks is 32: 128 - 256 workgroups taking the tail's ticket one after the other cost the late passes of a
  // 250k-point source 28 us, 59 against 31: scripts/diag_shards.py, N = 4)
  pl.tail = pl.route != Route::kFusedLane && pl.route != Route::kFusedQueue && q.n > 0 && grid_blocks(factor_tiles(q.n, pl.pts)) <= kFuseMaxBlocks;
  return pl;
}

// the factor stage's view of the problem that every kind of pass shares: clouds, correspondences, pose, rejector and robust kernel
// (a host rejector sees every nearest neighbour: no distance rejection of its own)
template <typename Real>
static LinParams<Real> factor_params(const sga_problem* pb, const sga_factor_params* fp, const double T[16], bool host_rejector) {
  const sga_index* idx = pb->target;
  LinParams<Real> p{};
  p.src_pts = pb->src_pts();
  p.src_cov = pb->src_cov();
  p.n = static_cast<int>(pb->n);
  p.tgt_pts = idx->kind != SGA_INDEX_KDTREE ? idx->pts.p : idx->kd_pts.p;
  p.tgt_nrm = idx->nrm.p;
  p.tgt_cov = idx->cov.p;
  p.corr = pb->corr.p;
  p.hint = pb->hint.p;
  if constexpr (sizeof(Real) == 4)
    p.maha = pb->maha.p;
  else
    p.maha = pb->maha64.p;
  p.T = rigid_from_colmajor<Real>(T);
  const bool rejects = !(fp->max_dist_sq < 0 || host_rejector);
  p.max_sq = rejects ? static_cast<Real>(fp->max_dist_sq) : static_cast<Real>(INFINITY);
  // the walks stay fp32: d2 == max_sq must still be found (strict '>' rejector), and the nudge also reaches past a double threshold
  // that float(max_dist_sq) rounded down
  const float max_sq_f = rejects ? static_cast<float>(fp->max_dist_sq) : INFINITY;
  p.bound2 = max_sq_f < 3.0e38f ? max_sq_f * 1.0000002f : INFINITY;
  if constexpr (sizeof(Real) == 8) {
    // fp64 keeps a pair on its double distance from the double query q, but the walks and the `within` tests measure kd_dist2 from
    // fl32(q): a target within r = sqrt(max_dist_sq) of q lies within r + |q - fl32(q)| of fl32(q), and kd_dist2 rounds that by less
    // than 6 ulp (the factor 1 + 2^-20 covers it and the cast).  |q_a - fl32(q_a)| <= 2^-24 |q_a|, and every query T s of the source box
    // has |q_a| <= |t_a| + sum_b |R_ab| max(|lo_b|, |hi_b|) (device frames, column-major T).
    if (rejects && p.n > 0 && max_sq_f < 3.0e38f) {
      double m2 = 0.0;
      for (int a = 0; a < 3; a++) {
        double ma = std::fabs(T[12 + a]);
        for (int b = 0; b < 3; b++) ma += std::fabs(T[4 * b + a]) * std::max(std::fabs(static_cast<double>(pb->bbox_lo[b])), std::fabs(static_cast<double>(pb->bbox_hi[b])));
        m2 += ma * ma;
      }
      const double r = std::sqrt(fp->max_dist_sq) + 0x1p-24 * (1.0 + 1e-6) * std::sqrt(m2);
      p.bound2 = std::max(p.bound2, static_cast<float>(r * r * (1.0 + 0x1p-20)));
    }
  }
  p.robust_kind = fp->robust_kind;
  p.robust_c = static_cast<Real>(fp->robust_c);
  return p;
}

// the factor stage's view of the target's search structure: the hash of a voxel map (Gaussian or flat: the lookup happens inside the
// factor kernel), the kd-tree otherwise; a projective index travels as a kernel argument of its own (projective_linearize_kernel)
template <typename Real>
static void target_view(LinParams<Real>& p, const sga_index* idx) {
  if (idx->kind == SGA_INDEX_FLATMAP) {
    p.flat.hkeys = idx->hkeys.p;
    p.flat.hvals = idx->hvals.p;
    p.flat.hmask = idx->hmask;
    p.flat.inv_leaf = 1.0 / idx->leaf;
    p.flat.vnum = idx->vcounts.p;
    p.flat.offsets = idx->search_offsets;
    for (int k = 0; k < 3; k++) p.flat.org[k] = idx->origin[k];
  } else if (idx->kind == SGA_INDEX_VOXELMAP) {
    p.vox.hkeys = idx->hkeys.p;
    p.vox.hvals = idx->hvals.p;
    p.vox.hmask = idx->hmask;
    p.vox.inv_leaf = 1.0 / idx->leaf;
    for (int k = 0; k < 3; k++) p.vox.org[k] = idx->origin[k];
    p.vox.offsets = idx->search_offsets;
  } else if (idx->kind == SGA_INDEX_KDTREE) {
    p.kd = make_kd_view(idx);
  }
}

template <typename Real>
static int linearize_dispatch(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double* d_out30, double* host, unsigned long long seq, bool with_model = false) {
  const sga_index* idx = pb->target;
  // Gaussian, flat voxel map or projective search: the lookup happens inside the factor kernel, no certificates, no warm passes, no cell
  // grid, no fp64 re-decision of a runner-up, routing unit 1
  const bool voxel = idx->kind != SGA_INDEX_KDTREE;
  const bool flat = idx->kind == SGA_INDEX_FLATMAP;
  const bool proj = idx->kind == SGA_INDEX_PROJECTIVE;
  if (fp->factor_kind == SGA_GICP && ((pb->n > 0 && !pb->has_covs) || (idx->n > 0 && !idx->has_covs))) return fail(SGA_ERR_INVALID, "GICP needs covariances on both source and target");
  // PLANE_ICP: a kd-tree or a projective search over a target with normals, or a flat map that keeps normals (per slot, under the slot
  // numbering flat_nearest returns)
  if (fp->factor_kind == SGA_PLANE_ICP && proj && idx->n > 0 && !idx->has_normals) return fail(SGA_ERR_UNSUPPORTED, "PLANE_ICP needs a projective search over a target with normals");
  if (fp->factor_kind == SGA_PLANE_ICP && !proj && ((voxel && !flat) || ((flat || idx->n > 0) && !idx->has_normals)))
    return fail(SGA_ERR_UNSUPPORTED, "PLANE_ICP needs a kd-tree index over a target with normals");
  if (fp->factor_kind < 0 || fp->factor_kind > 2) return fail(SGA_ERR_INVALID, "invalid factor_kind %d", fp->factor_kind);

  if constexpr (sizeof(Real) == 8)
    if (pb->maha64.n < pb->n * 6) SGA_TRY(pb->maha64.alloc(pb->n * 6));
  const bool host_rejector = pb->rejector_fn != nullptr && !voxel;
  LinParams<Real> p = factor_params<Real>(pb, fp, T, host_rejector);
  target_view(p, idx);
  p.cert_nn2 = (!voxel && sizeof(Real) == 8) ? pb->hint2.p : nullptr;  // fp64 arithmetic: the factor kernel measures the walk's two candidates again, in double
  p.store_maha = fp->robust_kind != SGA_ROBUST_NONE ? 1 : 0;  // the error passes of a robust factor run the error kernel
  p.partials = pb->partials.p;
  const int ncols = kModelCols, out_n = with_model ? kRow : SGA_ACCUM_DOUBLES;  // the caller's buffer: the system, or the system + its moments

  // warm pass?  Only with certificates from a previous pass in the same arithmetic (the queries must be bit-identical), and only
  // while no source point can have moved farther than the certificates can possibly cover.
  const int math = sizeof(Real) == 4 ? SGA_MATH_FP32 : SGA_MATH_FP64;
  const double displacement = (!voxel && p.n > 0 && pb->prev_valid && pb->prev_math == math) ? max_displacement(T, pb->T_prev, pb->bbox_lo, pb->bbox_hi) : INFINITY;
  const double unit = voxel ? 1.0 : routing_unit(idx);  // the target's own length scale relative to the scene the thresholds were tuned on
  NNParams<Real> q{};
  q.src_pts = pb->src_pts();
  q.n = p.n;
  q.kd = p.kd;
  q.T = p.T;
  q.within2 = p.bound2;
  q.slack_min = static_cast<float>(kSlackMin * unit), q.slack_max = static_cast<float>(kSlackMax * unit);
  q.cert_pad = std::max(g_cert_pad, 0.f);
  q.bound2 = p.bound2 * (1.f + kSearchMargin) * (1.f + kSearchMargin);
  q.nn = pb->hint.p, q.nn2 = pb->hint2.p, q.rex = pb->rex.p, q.walked = pb->walked.p;
  q.fast = g_fast_scan;
  q.leaves = pb->dbg_leaves.n >= pb->n ? pb->dbg_leaves.p : nullptr;

  const PassPlan plan = plan_pass<Real>(ctx, pb, q, displacement, unit, host_rejector);
  p.num_tiles = factor_tiles(p.n, plan.pts);
  const int blocks = grid_blocks(p.num_tiles);
  p.tail = FusedTail{plan.tail ? 1 : 0, ctx->d_ticket.p, d_out30, out_n, host, seq};
  q.check = plan.warm ? 1 : 0;
  if (plan.warm) q.T_prev = rigid_from_colmajor<Real>(pb->T_prev);
  if (plan.grid) {
    q.grid_walk = g_grid_walk;
    q.grid = make_grid_view(idx);
  }
  q.chunk_tiles = plan.chunk_tiles;

  const bool timed = ctx->profiling && (ctx->lin_seq++ % ctx->profile_period) == 0;  // sampled: event records cost ~7 us each
  if (timed) {
    sga_profile_collect_pending(ctx);
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    ctx->pending_warm = plan.warm;
  }
  int rows = p.n > 0 ? blocks : 0;  // partial rows left for reduce_rows_kernel
  // The search kernels rewrite hint / hint2 / rex for THIS pose: until the pass has been launched completely the certificates belong
  // to no pose the host knows, so an early return below (allocation, rejector callback, launch error) must not leave them marked
  // valid for T_prev.
  const bool first_pass = !pb->prev_valid;
  if (!voxel) pb->prev_valid = false;
  pb->state_fresh = false;
  if (plan.route != Route::kFactors) {
    if (q.leaves != nullptr) SGA_HIP(hipMemsetAsync(q.leaves, 0, pb->n * sizeof(int), ctx->stream));
    if (plan.grid && (first_pass || (plan.route != Route::kGrid && !plan.warm))) pb->grid_open_frac = 0.0;  // a kd pass in between: the grid gets another chance afterwards
    pb->order_tiles = 0;  // (set again below when this pass records its tiles' durations)
    const size_t words = static_cast<size_t>(p.kd.depth);  // traversal stack rows
    const dim3 sgrid((p.n + kSearchBlock - 1) / kSearchBlock), sblock(kSearchBlock);
    switch (plan.route) {
      case Route::kGrid:  // the factors follow as linearize_kernel over nn[]
        if (pb->grid_stats.n < 4) {
          SGA_TRY(pb->grid_stats.alloc(4));
          SGA_HIP(hipMemsetAsync(pb->grid_stats.p, 0, 4 * sizeof(uint32_t), ctx->stream));
        }
        SGA_TRY(grid_search_pass<Real>(ctx, idx, pb->src_pts(), p.n, p.T, q.bound2, pb->hint.p, pb->hint2.p, pb->rex.p, pb->grid_stats.p));
        pb->grid_passes++;
        break;
      case Route::kCertify:
        if constexpr (sizeof(Real) == 4) {
          p.cert_nn = q.nn, p.cert_nn2 = q.nn2, p.cert_rex = q.rex, p.cert_walked = q.walked;
          p.T_prev = q.T_prev, p.cert_within2 = q.within2, p.cert_pad = q.cert_pad;
          p.cert_slack_min = q.slack_min, p.cert_slack_max = q.slack_max;
          const size_t lds = std::max<size_t>(words, 1) * 64 * sizeof(uint32_t) * (kTile / 64);
          with_factor(fp->factor_kind, [&](auto f) { hipLaunchKernelGGL((certify_linearize_kernel<Real, decltype(f)::value, 1>), dim3(blocks), dim3(kTile), lds, ctx->stream, p, q); });
        }
        break;
      case Route::kFusedLane:
        if constexpr (sizeof(Real) == 4) {  // one partial row per tile of 64 points
          rows = static_cast<int>(sgrid.x);
          if (plan.order_record) {
            SGA_TRY(pb->tile_cost.reserve(sgrid.x));
            SGA_TRY(pb->tile_order.reserve(sgrid.x));
            q.tile_cost = pb->tile_cost.p;
            if (plan.order_use) q.tile_order = pb->tile_order.p;
          }
          const size_t lds = std::max<size_t>(words, 3) * 64 * sizeof(uint32_t);
          with_factor(fp->factor_kind, [&](auto f) {
            if (plan.warm)
              hipLaunchKernelGGL((search_linearize_kernel<Real, decltype(f)::value, true>), sgrid, sblock, lds, ctx->stream, q, p);
            else
              hipLaunchKernelGGL((search_linearize_kernel<Real, decltype(f)::value, false>), sgrid, sblock, lds, ctx->stream, q, p);
          });
        }
        break;
      case Route::kFusedQueue:
      case Route::kQueue: {
        q.inv_leaf = p.kd.n > 0 ? std::ldexp(1.0, p.kd.depth) / static_cast<double>(p.kd.n) : 0.0;
        const dim3 qgrid((sgrid.x + q.chunk_tiles - 1) / q.chunk_tiles);
        const size_t lds = std::max<size_t>(words, 3) * 64 * sizeof(uint32_t);
        if (plan.route == Route::kFusedQueue) {
          if constexpr (sizeof(Real) == 4) {  // one partial row per chunk
            rows = static_cast<int>(qgrid.x);
            with_factor(fp->factor_kind, [&](auto f) { hipLaunchKernelGGL((nn_search_queue_kernel<Real, true, decltype(f)::value>), qgrid, sblock, lds, ctx->stream, q, p); });
          }
        } else if (plan.warm)
          hipLaunchKernelGGL((nn_search_queue_kernel<Real, true>), qgrid, sblock, lds, ctx->stream, q, p);
        else
          hipLaunchKernelGGL((nn_search_queue_kernel<Real, false>), qgrid, sblock, lds, ctx->stream, q, p);
        break;
      }
      case Route::kLane:
        if (plan.warm)
          hipLaunchKernelGGL((nn_search_kernel<Real, kSearchBlock, true>), sgrid, sblock, words * kSearchBlock * sizeof(uint32_t), ctx->stream, q);
        else
          hipLaunchKernelGGL((nn_search_kernel<Real, kSearchBlock, false>), sgrid, sblock, words * kSearchBlock * sizeof(uint32_t), ctx->stream, q);
        break;
      case Route::kFactors: break;
    }
    if (timed) {
      (void)hipEventRecord(ctx->ev_mid, ctx->stream);
      ctx->mid_recorded = true;
    }
    if (host_rejector) {  // neighbours down, verdicts up (rejector.hpp:11-28 through sga_rejector_fn)
      const size_t n = pb->n;
      DevBuf<long long> d_idx;
      DevBuf<float> d_d2;
      SGA_TRY(d_idx.alloc(n));
      SGA_TRY(d_d2.alloc(n));
      SGA_TRY(pb->reject.reserve(n));
      hipLaunchKernelGGL((export_neighbours_kernel<Real>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, pb->src_pts(), pb->hint.p, p.n, p.tgt_pts, p.T, d_idx.p, d_d2.p);
      SGA_HIP(hipGetLastError());
      std::vector<int64_t> h_idx(n);
      std::vector<float> h_d2(n);
      std::vector<unsigned char> h_rej(n, 0);
      SGA_HIP(hipMemcpyAsync(h_idx.data(), d_idx.p, n * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
      SGA_HIP(hipMemcpyAsync(h_d2.data(), d_d2.p, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
      SGA_HIP(hipStreamSynchronize(ctx->stream));
      int cb_rc;
      {
        StreamScope outside(nullptr);  // user code: objects it destroys (a Python GC run) are not stream-ordered frees of this entry point
        cb_rc = pb->rejector_fn(pb->rejector_user, pb->caller_T ? pb->caller_T : T, n, h_idx.data(), h_d2.data(), h_rej.data());  // the rejector sees the CALLER's pose
      }
      if (cb_rc != 0) return fail(SGA_ERR_CALLBACK, "rejector callback failed");
      SGA_HIP(hipMemcpyAsync(pb->reject.p, h_rej.data(), n, hipMemcpyHostToDevice, ctx->stream));
      SGA_HIP(hipStreamSynchronize(ctx->stream));  // h_rej goes out of scope
      p.reject = pb->reject.p;
    }
  }
  if (p.n > 0 && !plan.fused()) {
    with_factor(fp->factor_kind, [&](auto f) {
      constexpr int F = decltype(f)::value;
      if (flat)
        launch_linearize<Real, F, 2>(ctx->stream, p, blocks, plan.pts);
      else if (proj) {
        hipLaunchKernelGGL((projective_linearize_kernel<Real, F, 1>), dim3(blocks), dim3(kTile), 0, ctx->stream, p, make_proj_view(idx));  // (plan.pts == 1)
      } else if (voxel) {
        if constexpr (F != SGA_PLANE_ICP) launch_linearize<Real, F, 1>(ctx->stream, p, blocks, plan.pts);  // (a Gaussian map refuses PLANE_ICP above)
      } else
        launch_linearize<Real, F, 0>(ctx->stream, p, blocks, plan.pts);
    });
  }
  // the sum of the rows: inside the factor kernel (tail), or reduce_rows_kernel over the rows of the fused search or of the factor
  // kernel's workgroups (a grid pass's search statistics ride along)
  if (!plan.tail) launch_reduce(ctx, pb->partials.p, rows, ncols, kRow, pb->partials.p + partial_rows(pb->n) * kRow, d_out30, out_n, host, seq, true, plan.route == Route::kGrid ? pb->grid_stats.p : nullptr);
  pb->grid_stats_pending = plan.route == Route::kGrid && !plan.tail && out_n > kStatsCol + 1;
  {  // what sga_problem_get_last_plan reports
    const int lp[8] = {static_cast<int>(plan.route), plan.warm, plan.grid, plan.pts, plan.tail, plan.chunk_tiles, plan.tail ? 0 : rows, plan.tail ? 0 : reduce_groups(rows)};
    std::copy(lp, lp + 8, pb->last_plan);
  }
  if (timed) {  // the whole GPU side of the pass: search + factors + the sum of the rows
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    ctx->pending |= 1;
  }
  if (plan.order_record) {  // after the reduction has handed the result to the host: the tiles are sorted while the host solves
    hipLaunchKernelGGL(tile_order_kernel, dim3(8), dim3(1024), 0, ctx->stream, pb->tile_cost.p, pb->tile_order.p, rows);
    pb->order_tiles = static_cast<unsigned>(rows);
    pb->order_stream = ctx->stream;
  }
  SGA_HIP(hipGetLastError());
  pb->last_math = math;
  pb->lin_factor = fp->factor_kind;
  memcpy(pb->lin_T, T, sizeof(pb->lin_T));
  pb->maha_valid = p.store_maha != 0;
  if (!voxel) {
    memcpy(pb->T_prev, T, sizeof(pb->T_prev));
    pb->prev_valid = true;
    pb->prev_math = math;
    if (plan.warm)
      pb->warm_passes++;
    else
      pb->cold_passes++;
  }
  return SGA_OK;
}

// The mahalanobis matrices of the last linearization, (C_t + R C_s R^T)^-1 per accepted pair (gicp_factor.hpp:57-60), written on
// demand: the hot loop of a non-robust registration never reads them (the error model answers the error passes), so the factor
// kernels skip the 24-byte store per point; the error kernel and sga_problem_get_factors call this first.
template <typename Real>
__global__ void recompute_maha_kernel(const Cov8* __restrict__ src_cov, const Cov8* __restrict__ tgt_cov, const int* __restrict__ corr, int n, Rigid<Real> T, Real* __restrict__ maha) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int j = corr[i];
  if (j < 0) return;
  const Sym3<Real> Cs = load_sym<Real>(src_cov, i);
  const Sym3<Real> Ct = load_sym<Real>(tgt_cov, j);
  const Sym3<Real> RCR = rotate_sym(T.r, Cs);
  const Sym3<Real> M = inverse_sym<Real>({Ct.xx + RCR.xx, Ct.xy + RCR.xy, Ct.xz + RCR.xz, Ct.yy + RCR.yy, Ct.yz + RCR.yz, Ct.zz + RCR.zz});
  Real* m = maha + static_cast<size_t>(i) * 6;
  m[0] = M.xx, m[1] = M.xy, m[2] = M.xz, m[3] = M.yy, m[4] = M.yz, m[5] = M.zz;
}

int problem_ensure_maha(sga_context* ctx, sga_problem* pb) {
  if (pb->maha_valid || pb->n == 0 || pb->lin_factor != SGA_GICP) return SGA_OK;
  const sga_index* idx = pb->target;
  const int n = static_cast<int>(pb->n);
  if (pb->last_math == SGA_MATH_FP64) {
    if (pb->maha64.n < pb->n * 6) SGA_TRY(pb->maha64.alloc(pb->n * 6));
    hipLaunchKernelGGL((recompute_maha_kernel<double>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, pb->src_cov(), idx->cov.p, pb->corr.p, n, rigid_from_colmajor<double>(pb->lin_T), pb->maha64.p);
  } else {
    hipLaunchKernelGGL((recompute_maha_kernel<float>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, pb->src_cov(), idx->cov.p, pb->corr.p, n, rigid_from_colmajor<float>(pb->lin_T), pb->maha.p);
  }
  SGA_HIP(hipGetLastError());
  pb->maha_valid = true;
  return SGA_OK;
}

template <typename Real>
static int error_dispatch(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double* d_out1, double* host, unsigned long long seq) {
  const sga_index* idx = pb->target;
  ErrParams<Real> p{};
  p.src_pts = pb->src_pts();
  p.n = static_cast<int>(pb->n);
  p.num_tiles = (p.n + kTile - 1) / kTile;
  p.tgt_pts = idx->kind != SGA_INDEX_KDTREE ? idx->pts.p : idx->kd_pts.p;
  p.tgt_nrm = idx->nrm.p;
  p.corr = pb->corr.p;
  if (fp->factor_kind == SGA_GICP) {
    if ((sizeof(Real) == 4) != (pb->last_math == SGA_MATH_FP32)) return fail(SGA_ERR_INVALID, "sga_error in another arithmetic than the last sga_linearize");
    SGA_TRY(problem_ensure_maha(ctx, pb));
  }
  if constexpr (sizeof(Real) == 4) {
    p.maha = pb->maha.p;
  } else {
    if (fp->factor_kind == SGA_GICP && pb->maha64.n < pb->n * 6) return fail(SGA_ERR_INVALID, "sga_error(fp64) before sga_linearize(fp64)");
    p.maha = pb->maha64.p;
  }
  p.T = rigid_from_colmajor<Real>(T);
  p.robust_kind = fp->robust_kind;
  p.robust_c = static_cast<Real>(fp->robust_c);
  p.partials = pb->partials.p;
  const int blocks = grid_blocks(p.num_tiles);
  const bool fuse = p.n > 0 && blocks <= kFuseMaxBlocks;
  p.tail = FusedTail{fuse ? 1 : 0, ctx->d_ticket.p, d_out1, 1, host, seq};
  if (fp->factor_kind == SGA_PLANE_ICP && !idx->has_normals) return fail(SGA_ERR_UNSUPPORTED, "PLANE_ICP needs target normals");
  const bool timed = ctx->profiling && (ctx->err_seq++ % ctx->profile_period) == 0;
  if (timed) {
    sga_profile_collect_pending(ctx);
    (void)hipEventRecord(ctx->ev2, ctx->stream);
  }
  if (p.n > 0) {
    if (fp->factor_kind < 0 || fp->factor_kind > 2) return fail(SGA_ERR_INVALID, "invalid factor_kind %d", fp->factor_kind);
    with_factor(fp->factor_kind, [&](auto f) { hipLaunchKernelGGL((error_kernel<Real, decltype(f)::value>), dim3(blocks), dim3(kTile), 0, ctx->stream, p); });
  }
  if (timed) {
    (void)hipEventRecord(ctx->ev3, ctx->stream);
    ctx->pending |= 2;
  }
  if (!fuse) launch_reduce(ctx, pb->partials.p, p.n > 0 ? blocks : 0, 1, 1, pb->partials.p + partial_rows(pb->n) * kRow, d_out1, 1, host, seq);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

size_t problem_partials_doubles(size_t n) { return partial_rows(n) * kRow + static_cast<size_t>(kReduceGroups) * kCols; }

// Hand `count` doubles to the host after an all-reduce (see reduce_rows_kernel for the protocol).
__global__ void publish_kernel(const double* __restrict__ src, int count, double* __restrict__ host, unsigned long long seq) {
  if (static_cast<int>(threadIdx.x) < count) host[threadIdx.x] = src[threadIdx.x];
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(host + kSeqWord), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// wait until the device has published `seq` in the pinned sequence word `word` (null: the context's own, behind h_accum)
static int wait_result(sga_context* ctx, unsigned long long seq, const double* word = nullptr) {
  const int rc = wait_published(ctx, reinterpret_cast<const unsigned long long*>(word != nullptr ? word : ctx->h_accum + kSeqWord), seq);
  if (rc != kNotPublished) return rc;
  // a faulted or aborted launch may have left the arrival counter of reduce_rows_kernel non-zero: the next result on this
  // context would never be published
  (void)hipMemsetAsync(ctx->d_ticket.p, 0, ctx->d_ticket.n * sizeof(unsigned), ctx->stream);
  return fail(SGA_ERR_HIP, "result was not published by the device");
}

// single GPU: the final reduction kernel publishes; with a communicator the all-reduce comes first
static int fetch_result(sga_context* ctx, const double* d_src, int count, unsigned long long seq, bool published_by_kernel) {
  if (!published_by_kernel) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(kCols), 0, ctx->stream, d_src, count, ctx->h_accum_dev, seq);
    SGA_HIP(hipGetLastError());
  }
  return wait_result(ctx, seq);
}

static int check_args(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double* T) {
  if (!ctx || !pb || !fp || !T) return fail(SGA_ERR_INVALID, "null argument");
  if (pb->device != ctx->device) return fail(SGA_ERR_INVALID, "problem lives on device %d, context on %d", pb->device, ctx->device);
  return SGA_OK;
}

}  // namespace sga
// Fold the HIP-event pair of the previous launch into the running averages (no-op while that launch is still in flight).
void sga_profile_collect_pending(sga_context* ctx) {
  // Called before the next launch of either kind: the previous launches have long finished (their results were consumed), the
  // event synchronisation only covers the short gap between the result flag and the event's own completion signal.
  if (!ctx->profiling || ctx->pending == 0) return;
  float ms = 0.f;
  if (ctx->pending & 1) {
    if (hipEventSynchronize(ctx->ev1) == hipSuccess && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1) == hipSuccess) {
      ctx->lin_ms += ms;
      ctx->lin_calls++;
      if (ctx->pending_warm) {
        ctx->warm_ms += ms;
        ctx->warm_calls++;
      } else {
        ctx->cold_ms += ms;
        ctx->cold_calls++;
      }
      if (ctx->mid_recorded && hipEventElapsedTime(&ms, ctx->ev0, ctx->ev_mid) == hipSuccess) {
        ctx->search_ms += ms;
        ctx->search_calls++;
        if (ctx->pending_warm) ctx->warm_first_ms += ms;
      }
    }
    ctx->mid_recorded = false;
    if (ctx->comm_recorded && hipEventSynchronize(ctx->ev_comm) == hipSuccess && hipEventElapsedTime(&ms, ctx->ev1, ctx->ev_comm) == hipSuccess) {
      ctx->comm_ms += ms;
      ctx->comm_calls++;
    }
    ctx->comm_recorded = false;
  }
  if (ctx->pending & 2) {
    if (hipEventSynchronize(ctx->ev3) == hipSuccess && hipEventElapsedTime(&ms, ctx->ev2, ctx->ev3) == hipSuccess) {
      ctx->err_ms += ms;
      ctx->err_calls++;
    }
  }
  ctx->pending = 0;
}

using namespace sga;

extern "C" {

int sga_linearize_per_point(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double* values28, unsigned char* inlier) {
  SGA_TRY(check_args(ctx, pb, fp, T));
  if (!values28 || !inlier) return fail(SGA_ERR_INVALID, "null output");
  const bool flat = pb->target->kind == SGA_INDEX_FLATMAP;
  if (pb->target->kind != SGA_INDEX_KDTREE && !flat) return fail(SGA_ERR_UNSUPPORTED, "per-point factors need a kd-tree target");
  SGA_ENTER(ctx);
  double H[36], b[6], e = 0;
  uint64_t ninl = 0;
  sga_factor_params f32 = *fp;
  f32.math_mode = SGA_MATH_FP64;  // the export is a diagnostic: full precision per pair
  SGA_TRY(sga_linearize(ctx, pb, &f32, T, H, b, &e, &ninl));  // neighbours + factor state at T
  const size_t n = pb->n;
  if (n == 0) return SGA_OK;
  double Td[16];
  const LinParams<double> p = factor_params<double>(pb, fp, problem_pose(pb, T, Td), false);  // (the export reads corr[]: the verdicts of the pass above, no test of its own)
  DevBuf<double> d_vals;
  DevBuf<unsigned char> d_ok;
  SGA_TRY(d_vals.alloc(n * 28));
  SGA_TRY(d_ok.alloc(n));
  const dim3 grid((n + 255) / 256), block(256);
  with_factor(fp->factor_kind, [&](auto f) { hipLaunchKernelGGL((per_point_kernel<double, decltype(f)::value>), grid, block, 0, ctx->stream, p, d_vals.p, d_ok.p); });
  SGA_HIP(hipGetLastError());
  SGA_HIP(hipMemcpyAsync(values28, d_vals.p, n * 28 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipMemcpyAsync(inlier, d_ok.p, n, hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  if (!origin_is_zero(pb->src_origin)) {  // per-point systems of the device frame -> the caller's twist convention (common.hpp)
    for (size_t i = 0; i < n; i++) {
      double* v = values28 + 28 * i;
      double Hi[36], bi[6];
      sga_unpack_accumulator(v, Hi, bi, nullptr, nullptr);  // reads [0, 27) only
      system_to_caller(pb->src_origin, Hi, bi);
      int k = 0;
      for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) v[k++] = Hi[6 * r + c];
      for (int r = 0; r < 6; r++) v[21 + r] = bi[r];
    }
  }
  return SGA_OK;
}

int sga_problem_set_rejector(sga_problem* pb, sga_rejector_fn fn, void* user) {
  if (!pb) return fail(SGA_ERR_INVALID, "null argument");
  if (fn && pb->target->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_UNSUPPORTED, "host rejectors need a kd-tree target");
  pb->rejector_fn = fn;
  pb->rejector_user = user;
  pb->prev_valid = false;  // the search bound changes with the rejector
  return SGA_OK;
}

void sga_set_warm_limit(double warm_delta_m) { g_warm_delta = warm_delta_m; }
double sga_get_warm_limit(void) { return g_warm_delta; }

int sga_linearize_async(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double* d_out30) {
  SGA_TRY(check_args(ctx, pb, fp, T));
  if (!d_out30) return fail(SGA_ERR_INVALID, "null output");
  pb->model_valid = false;  // the cached factor state changes: the synchronous error path must not answer from an older model
  SGA_ENTER(ctx);
  double Tdev[16];
  const double* Td = problem_pose(pb, T, Tdev);
  pb->caller_T = T;
  const int rc_dispatch = fp->math_mode == SGA_MATH_FP64 ? linearize_dispatch<double>(ctx, pb, fp, Td, d_out30, nullptr, 0) : linearize_dispatch<float>(ctx, pb, fp, Td, d_out30, nullptr, 0);
  pb->caller_T = nullptr;  // (valid for this dispatch only)
  SGA_TRY(rc_dispatch);
  SGA_TRY(problem_accumulator_to_caller(ctx, pb, d_out30));  // frames.hip
  return SGA_OK;
}

int sga_error_async(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double* d_out1) {
  SGA_TRY(check_args(ctx, pb, fp, T));
  if (!d_out1) return fail(SGA_ERR_INVALID, "null output");
  SGA_ENTER(ctx);
  double Tdev[16];
  const double* Td = problem_pose(pb, T, Tdev);
  return fp->math_mode == SGA_MATH_FP64 ? error_dispatch<double>(ctx, pb, fp, Td, d_out1, nullptr, 0) : error_dispatch<float>(ctx, pb, fp, Td, d_out1, nullptr, 0);
}

}  // extern "C"

namespace sga {
// pb->caller_T points at the caller's (often stack) pose for the duration of ONE dispatch (a host rejector is shown the caller's pose):
// cleared when the entry point returns, whichever way (it used to dangle)
struct CallerPoseScope {
  sga_problem* pb;
  CallerPoseScope(sga_problem* p, const double* T) : pb(p) { pb->caller_T = T; }
  ~CallerPoseScope() { pb->caller_T = nullptr; }
  CallerPoseScope(const CallerPoseScope&) = delete;
  CallerPoseScope& operator=(const CallerPoseScope&) = delete;
};
// sga_linearize in two halves, so that one host thread can keep several devices busy (multi.hip): enqueue = the kernels of the pass, the
// sum over ranks if the context has a communicator, and the hand-off of the result to the host; collect = wait for it (ctx->h_accum
// then holds `count` doubles: the system, or the system and the error model).
int linearize_enqueue(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T_caller[16], unsigned long long* seq_out, int* count_out) {
  double Tdev[16];
  const double* T = problem_pose(pb, T_caller, Tdev);  // the kernels work between the two device frames (common.hpp)
  CallerPoseScope caller_pose(pb, T_caller);
  SGA_TRY(problem_check_shard_frames(ctx, pb));
  const unsigned long long seq = ++ctx->publish_seq;
  const bool direct = !ctx->sharded();
  double* host = direct ? ctx->h_accum_dev : nullptr;
  const bool model = fp->robust_kind == SGA_ROBUST_NONE && g_error_model;  // a robust kernel's error is not quadratic in the pose
  pb->model_valid = false;
  const int count = model ? kRow : SGA_ACCUM_DOUBLES;
  SGA_TRY(fp->math_mode == SGA_MATH_FP64 ? linearize_dispatch<double>(ctx, pb, fp, T, ctx->d_accum.p, host, seq, model) : linearize_dispatch<float>(ctx, pb, fp, T, ctx->d_accum.p, host, seq, model));
  int rc = comm_allreduce_sum(ctx, ctx->d_accum.p, count);  // source sharded over ranks: sum the shards' systems (and error models)
  if (rc == SGA_OK && !direct && (ctx->pending & 1)) {  // a timed pass: ev1 (behind the row reduction) -> ev_comm = the time inside the collective
    (void)hipEventRecord(ctx->ev_comm, ctx->stream);
    ctx->comm_recorded = true;
  }
  if (rc == SGA_OK && !direct) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(kCols), 0, ctx->stream, ctx->d_accum.p, count, ctx->h_accum_dev, seq);
    if (hipGetLastError() != hipSuccess) rc = fail(SGA_ERR_HIP, "publish_kernel launch failed");
  }
  if (rc != SGA_OK) {
    pb->prev_valid = false;  // the pass did not complete: its certificates are not to be trusted
    return rc;
  }
  *seq_out = seq;
  *count_out = count;
  return SGA_OK;
}
int linearize_collect(sga_context* ctx, sga_problem* pb, const double T[16], unsigned long long seq, int count) {
  const int rc = wait_result(ctx, seq);
  if (rc != SGA_OK) {
    pb->prev_valid = false;
    return rc;
  }
  if (pb->grid_stats_pending) {  // search statistics of a grid pass: the share of the queries its first ring left open steers the next cold pass
    pb->grid_stats_pending = false;
    if (!ctx->sharded() && pb->n > 0) {
      pb->grid_open_frac = ctx->h_accum[kStatsCol] / static_cast<double>(pb->n);
      pb->grid_open_total += static_cast<uint64_t>(ctx->h_accum[kStatsCol]);
      pb->grid_ring_total += static_cast<uint64_t>(ctx->h_accum[kStatsCol + 1]);
    }
  }
  if (count == kRow) {  // the error model: moments of the source's device frame, evaluated between device-frame poses (sga_error)
    double Tdev[16];
    memcpy(pb->model, ctx->h_accum, sizeof(pb->model));
    memcpy(pb->model_T, problem_pose(pb, T, Tdev), sizeof(pb->model_T));
    pb->model_valid = true;
  }
  return SGA_OK;
}
}  // namespace sga

namespace sga {
// ---- batched registration: one round (see BatchPair) --------------------------------------------------------------------------------
// round table: [prefix: count + 1 ints, padded to 16 bytes][BatchPair x count]
static size_t batch_pairs_offset(size_t count) { return ((count + 1) * sizeof(int) + 15) / 16 * 16; }
size_t batch_round_bytes(size_t count) { return batch_pairs_offset(count) + count * sizeof(BatchPair); }

int batch_round(sga_context* ctx, sga_batch* bt, const sga_factor_params* fp, const double* T, const unsigned char* active, bool seedless) {
  const size_t count = bt->problems.size();
  // the active pairs, largest first: the long pair's waves start first and the short pairs fill in behind them
  std::vector<int> order;
  for (size_t k = 0; k < count; k++)
    if (active == nullptr || active[k]) order.push_back(static_cast<int>(k));
  if (order.empty()) return SGA_OK;
  // a voxel map may have grown (or been filled) since the batch was created: its pairs' tiles are counted per round
  const bool map = bt->kind != SGA_INDEX_KDTREE;
  std::vector<int> tiles(bt->tiles);
  if (map)
    for (int k : order) tiles[k] = batch_pair_tiles(bt->problems[k]);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tiles[a] > tiles[b]; });
  int* prefix = static_cast<int*>(bt->h_round);
  BatchPair* pairs = reinterpret_cast<BatchPair*>(static_cast<unsigned char*>(bt->h_round) + batch_pairs_offset(count));
  std::vector<double> Tdev(16 * order.size());
  int blocks = 0;
  for (size_t a = 0; a < order.size(); a++) {
    const int k = order[a];
    sga_problem* pb = bt->problems[k];
    const sga_index* idx = pb->target;
    double* Td = &Tdev[16 * a];
    const double* Tp = problem_pose(pb, T + 16 * k, Td);  // each pair's pose between ITS two device frames (common.hpp)
    if (Tp != Td) memcpy(Td, Tp, 16 * sizeof(double));
    BatchPair d{};
    d.p = factor_params<float>(pb, fp, Td, false);
    target_view(d.p, idx);  // (as linearize_dispatch fills it: the kd-tree, or the map's hash, leaf size, origin and search offsets)
    d.p.partials = pb->partials.p;
    if (!map) {  // the search half: kd batches only
      d.q.src_pts = pb->src_pts();
      d.q.n = d.p.n;
      d.q.kd = d.p.kd;
      d.q.T = d.p.T;
      d.q.within2 = d.p.bound2;
      d.q.bound2 = d.p.bound2 * (1.f + kSearchMargin) * (1.f + kSearchMargin);
      d.q.nn = pb->hint.p, d.q.nn2 = pb->hint2.p, d.q.rex = pb->rex.p, d.q.walked = pb->walked.p;
      d.q.fast = g_fast_scan;
      d.seedless = seedless ? 1 : 0;
    }
    d.ntiles = tiles[k];
    d.pair = k;
    prefix[a] = blocks;
    blocks += (d.ntiles + 7) / 8 * 8;  // (bt->tile_prefix bounds the sum: batch.hip)
    pairs[a] = d;
  }
  prefix[order.size()] = blocks;
  const int nactive = static_cast<int>(order.size());
  const unsigned long long seq = ++bt->seq;
  SGA_HIP(hipMemcpyAsync(bt->d_round.p, bt->h_round, batch_round_bytes(count), hipMemcpyHostToDevice, ctx->stream));
  const int* d_prefix = reinterpret_cast<const int*>(bt->d_round.p);
  const BatchPair* d_pairs = reinterpret_cast<const BatchPair*>(bt->d_round.p + batch_pairs_offset(count));
  for (int k : order) {  // as in linearize_dispatch: until the round is launched completely the certificates belong to no pose the host knows
    sga_problem* pb = bt->problems[k];
    if (!map) {  // (a map pass is linearize_dispatch's Route::kFactors: it neither reads nor writes the state of the kd search)
      pb->prev_valid = false;
      pb->order_tiles = 0;
    }
    pb->model_valid = false;
    pb->state_fresh = false;
    if (tiles[k] == 0 && pb->n > 0) SGA_HIP(hipMemsetAsync(pb->corr.p, 0xff, pb->n * sizeof(int), ctx->stream));  // an empty target: no correspondences
  }
  if (blocks > 0 && !map) {
    const size_t lds = static_cast<size_t>(std::max(bt->max_depth, 3)) * 64 * sizeof(uint32_t);
    with_factor(fp->factor_kind, [&](auto f) { hipLaunchKernelGGL((batch_search_linearize_kernel<decltype(f)::value>), dim3(blocks), dim3(64), lds, ctx->stream, d_prefix, d_pairs, nactive); });
  } else if (blocks > 0) {
    with_factor(fp->factor_kind, [&](auto f) {
      constexpr int F = decltype(f)::value;
      if (bt->kind == SGA_INDEX_FLATMAP)
        hipLaunchKernelGGL((batch_map_linearize_kernel<F, 2>), dim3(blocks), dim3(64), 0, ctx->stream, d_prefix, d_pairs, nactive);
      else if constexpr (F != SGA_PLANE_ICP)  // (batch_check refuses PLANE_ICP on a Gaussian map)
        hipLaunchKernelGGL((batch_map_linearize_kernel<F, 1>), dim3(blocks), dim3(64), 0, ctx->stream, d_prefix, d_pairs, nactive);
    });
  }
  hipLaunchKernelGGL(batch_reduce_rows_kernel, dim3(nactive), dim3(kReduceSlices * kCols), 0, ctx->stream, d_pairs, bt->ticket.p, bt->h_out_dev, bt->h_out_dev + count * kRow, seq);
  SGA_HIP(hipGetLastError());
  int rc = wait_result(ctx, seq, bt->h_out + count * kRow);
  if (rc != SGA_OK) {
    (void)hipMemsetAsync(bt->ticket.p, 0, sizeof(unsigned), ctx->stream);
    return rc;
  }
  for (size_t a = 0; a < order.size(); a++) {  // what a lone pass at this pose leaves in the problem: a cold kd pass, or a map pass (Route::kFactors)
    const int k = order[a];
    sga_problem* pb = bt->problems[k];
    const double* Td = &Tdev[16 * a];
    pb->last_math = SGA_MATH_FP32;
    pb->lin_factor = fp->factor_kind;
    memcpy(pb->lin_T, Td, sizeof(pb->lin_T));
    pb->maha_valid = false;
    if (!map) {  // certificates and pass statistics belong to kd targets
      memcpy(pb->T_prev, Td, sizeof(pb->T_prev));
      pb->prev_valid = true;
      pb->prev_math = SGA_MATH_FP32;
      pb->cold_passes++;
    }
    pb->grid_stats_pending = false;
    const int lp[8] = {static_cast<int>(map ? Route::kFactors : Route::kFusedLane), 0, 0, 1, 0, 0, tiles[k], 1};
    std::copy(lp, lp + 8, pb->last_plan);
    memcpy(pb->model, bt->h_out + static_cast<size_t>(k) * kRow, sizeof(pb->model));
    memcpy(pb->model_T, Td, sizeof(pb->model_T));
    pb->model_valid = true;
  }
  return SGA_OK;
}
}  // namespace sga

extern "C" {

int sga_linearize(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double H[36], double b[6], double* e, uint64_t* num_inliers) {
  SGA_TRY(check_args(ctx, pb, fp, T));
  if (!H || !b || !e) return fail(SGA_ERR_INVALID, "null output");
  SGA_ENTER(ctx);
  unsigned long long seq = 0;
  int count = 0;
  SGA_TRY(linearize_enqueue(ctx, pb, fp, T, &seq, &count));
  SGA_TRY(linearize_collect(ctx, pb, T, seq, count));
  sga_unpack_accumulator(ctx->h_accum, H, b, e, num_inliers);
  problem_system_to_caller(pb, H, b);
  return SGA_OK;
}

}  // extern "C"

namespace sga {
bool error_model_enabled() { return g_error_model; }
// sga_error's device pass in two halves (see linearize_enqueue)
int error_enqueue(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T_caller[16], unsigned long long* seq_out) {
  double Tdev[16];
  const double* T = problem_pose(pb, T_caller, Tdev);
  const unsigned long long seq = ++ctx->publish_seq;
  const bool direct = !ctx->sharded();
  double* host = direct ? ctx->h_accum_dev : nullptr;
  SGA_TRY(fp->math_mode == SGA_MATH_FP64 ? error_dispatch<double>(ctx, pb, fp, T, ctx->d_accum.p, host, seq) : error_dispatch<float>(ctx, pb, fp, T, ctx->d_accum.p, host, seq));
  SGA_TRY(comm_allreduce_sum(ctx, ctx->d_accum.p, 1));
  if (!direct) {
    hipLaunchKernelGGL(publish_kernel, dim3(1), dim3(kCols), 0, ctx->stream, ctx->d_accum.p, 1, ctx->h_accum_dev, seq);
    SGA_HIP(hipGetLastError());
  }
  *seq_out = seq;
  return SGA_OK;
}
int error_collect(sga_context* ctx, unsigned long long seq, double* e) {
  SGA_TRY(wait_result(ctx, seq));
  *e = ctx->h_accum[0];
  return SGA_OK;
}
}  // namespace sga

extern "C" {

int sga_error(sga_context* ctx, sga_problem* pb, const sga_factor_params* fp, const double T[16], double* e) {
  SGA_TRY(check_args(ctx, pb, fp, T));
  if (!e) return fail(SGA_ERR_INVALID, "null output");
  if (pb->model_valid && fp->robust_kind == SGA_ROBUST_NONE && g_error_model) {  // no pass over the cloud: the model of the last linearization
    double Tdev[16];
    *e = error_model_value(pb->model, pb->model_T, problem_pose(pb, T, Tdev));
    return SGA_OK;
  }
  SGA_ENTER(ctx);
  unsigned long long seq = 0;
  SGA_TRY(error_enqueue(ctx, pb, fp, T, &seq));
  return error_collect(ctx, seq, e);
}

// experiments / tests: 0 = every error pass runs the error kernel (the reference's literal procedure)
void sga_set_error_model(int enabled) { g_error_model = enabled != 0; }

// diagnostics: record the leaves scanned per source point by the next passes (one-query-per-lane kernel); out = the last pass's
int sga_problem_set_search_stats(sga_context* ctx, sga_problem* pb, int enabled) {
  if (!ctx || !pb) return fail(SGA_ERR_INVALID, "null argument");
  SGA_ENTER(ctx);
  if (enabled) return pb->dbg_leaves.alloc(pb->n);
  pb->dbg_leaves.release();
  return SGA_OK;
}
// diagnostics: the source points in the engine's order (sorted by target leaf at init_T, then Morton): n x 4 floats (x, y, z, original index bits)
int sga_problem_get_sorted_points(sga_context* ctx, const sga_problem* pb, float* xyzw) {
  if (!ctx || !pb || !xyzw) return fail(SGA_ERR_INVALID, "null argument");
  if (pb->n == 0) return SGA_OK;
  SGA_ENTER(ctx);
  SGA_HIP(hipMemcpyAsync(xyzw, pb->src_pts(), pb->n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}
// diagnostics: the PassPlan of the last linearize_dispatch (route, warm, grid, points per lane, tail, chunk tiles, rows and workgroups
// of reduce_rows_kernel)
int sga_problem_get_last_plan(const sga_problem* pb, int out[8]) {
  if (!pb || !out) return fail(SGA_ERR_INVALID, "null argument");
  std::copy(pb->last_plan, pb->last_plan + 8, out);
  return SGA_OK;
}
int sga_problem_get_search_stats(sga_context* ctx, const sga_problem* pb, int* leaves_per_point) {
  if (!ctx || !pb || !leaves_per_point) return fail(SGA_ERR_INVALID, "null argument");
  if (pb->dbg_leaves.n < pb->n) return fail(SGA_ERR_INVALID, "search statistics are not enabled");
  SGA_ENTER(ctx);
  SGA_HIP(hipMemcpyAsync(leaves_per_point, pb->dbg_leaves.p, pb->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

// diagnostics / tests: the fixed-order sum of `nrows` host rows of kRow doubles, exactly as a linearization pass runs it (launch_reduce over
// kModelCols columns, stage rows behind the partial rows, result handed over through the pinned block); out = kRow doubles
int sga_debug_reduce_rows(sga_context* ctx, const double* rows, int nrows, int derive, double* out) {
  if (!ctx || !out || nrows < 0 || (nrows > 0 && !rows)) return fail(SGA_ERR_INVALID, "null argument or negative row count");
  SGA_ENTER(ctx);
  const size_t stage_off = sga::partial_rows(static_cast<size_t>(nrows) * 64) * sga::kRow;  // (one row per 64 points: where a pass over that many rows keeps its stage rows)
  sga::DevBuf<double> buf;
  SGA_TRY(buf.alloc(stage_off + static_cast<size_t>(sga::kReduceGroups) * sga::kCols));
  if (nrows > 0) SGA_HIP(hipMemcpyAsync(buf.p, rows, static_cast<size_t>(nrows) * sga::kRow * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
  const unsigned long long seq = ++ctx->publish_seq;
  sga::launch_reduce(ctx, buf.p, nrows, sga::kModelCols, sga::kRow, buf.p + stage_off, ctx->d_accum.p, sga::kRow, ctx->h_accum_dev, seq, derive != 0);
  SGA_HIP(hipGetLastError());
  SGA_TRY(sga::wait_result(ctx, seq));
  memcpy(out, ctx->h_accum, sga::kRow * sizeof(double));
  return SGA_OK;
}

#ifdef SGA_REDUCE_STAMPS
// diagnostics build (make stamps): the clock stamps of the last reduce_rows_kernel (layout: g_reduce_stamps)
int sga_debug_reduce_stamps(unsigned long long* out24) {
  if (hipDeviceSynchronize() != hipSuccess) return SGA_ERR_HIP;  // the finishing workgroup writes its stamps after it has released the result to the host
  if (hipMemcpyFromSymbol(out24, HIP_SYMBOL(sga::g_reduce_stamps), sizeof(unsigned long long) * 24) != hipSuccess) return SGA_ERR_HIP;
  return SGA_OK;
}
#else
int sga_debug_reduce_stamps(unsigned long long*) { return fail(SGA_ERR_UNSUPPORTED, "clock stamps of the row sum exist in the diagnostics build only (make stamps)"); }
#endif

#ifdef SGA_KD_TRIPS
// diagnostics build (make trips): loop-body executions of the walk since the last call, [0, 6) per lane, [8, 14) per wave
int sga_debug_kd_trips(unsigned long long* out16) {
  unsigned long long zero[16] = {0};
  if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_kd_trips), sizeof(zero)) != hipSuccess) return SGA_ERR_HIP;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_kd_trips), zero, sizeof(zero)) != hipSuccess) return SGA_ERR_HIP;
  return SGA_OK;
}
// diagnostics build: start / end (100 MHz wall clock) of the first `waves` search waves of the last fused search launch
int sga_debug_kd_wave_times(unsigned long long* out, int waves) {
  if (waves > 32768) waves = 32768;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kd_wave_times), sizeof(unsigned long long) * 2 * static_cast<size_t>(waves)) != hipSuccess) return SGA_ERR_HIP;
  return SGA_OK;
}
#else
int sga_debug_kd_trips(unsigned long long*) { return fail(SGA_ERR_UNSUPPORTED, "loop-trip counters exist in the diagnostics build only (make trips)"); }
int sga_debug_kd_wave_times(unsigned long long*, int) { return fail(SGA_ERR_UNSUPPORTED, "wave timers exist in the diagnostics build only (make trips)"); }
#endif

}  // extern "C"

namespace sga {
// The HIP runtime resolves a kernel (code object lookup, kernel descriptor, launch metadata) the first time it is used: 100 - 200 us each,
// paid in the middle of somebody's first registration — the kernels of the late LM iterations are first launched several passes in.
// Called once per process when the first context is created: asking for a kernel's attributes resolves it without launching anything.
void preload_hot_kernels() {
  hipFuncAttributes a;
#define SGA_PRELOAD(...) (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&__VA_ARGS__))
#define SGA_PRELOAD_FACTOR(F)                                        \
  SGA_PRELOAD(search_linearize_kernel<float, F, false>);            \
  SGA_PRELOAD(search_linearize_kernel<float, F, true>);             \
  SGA_PRELOAD(nn_search_queue_kernel<float, true, F>);              \
  SGA_PRELOAD(certify_linearize_kernel<float, F, 1>);               \
  SGA_PRELOAD(linearize_kernel<float, F, 0, kLinPts>);              \
  SGA_PRELOAD(linearize_kernel<float, F, 0, 1>);                   \
  SGA_PRELOAD(batch_search_linearize_kernel<F>)
  SGA_PRELOAD_FACTOR(SGA_GICP);
  SGA_PRELOAD_FACTOR(SGA_PLANE_ICP);
  SGA_PRELOAD_FACTOR(SGA_ICP);
  SGA_PRELOAD(linearize_kernel<float, SGA_GICP, 1, kLinPts>);
  SGA_PRELOAD(linearize_kernel<float, SGA_GICP, 1, 1>);
  SGA_PRELOAD(batch_map_linearize_kernel<SGA_GICP, 1>);
  SGA_PRELOAD(reduce_rows_kernel);
  SGA_PRELOAD(batch_reduce_rows_kernel);
  SGA_PRELOAD(tile_order_kernel);
  SGA_PRELOAD(publish_kernel);
  SGA_PRELOAD(error_kernel<float, SGA_GICP>);
#undef SGA_PRELOAD_FACTOR
#undef SGA_PRELOAD
  (void)hipGetLastError();
}
}  // namespace sga

extern "C" {

// experiments / tests: when the cell grid searches (SGA_GRID) and from how many target points on an index gets one (SGA_GRID_MIN_POINTS;
// affects indices built afterwards); negative values keep the current setting
void sga_set_grid_mode(int mode, long long min_points) {
  if (mode >= 0) sga::g_grid_mode = mode;
  if (min_points >= 0) sga::g_grid_min_points = min_points;
}

// experiments / tests: which search kernel runs (queue != 0: nn_search_queue_kernel with the given tiles per wave; <= 0 keeps a value)
void sga_set_search_mode(int queue, int chunk_tiles_cold, int chunk_tiles_warm) {
  g_search_queue = queue;
  if (chunk_tiles_cold > 0) g_chunk_tiles_cold = chunk_tiles_cold;
  if (chunk_tiles_warm > 0) g_chunk_tiles_warm = chunk_tiles_warm;
}

}  // extern "C"

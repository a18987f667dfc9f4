// The layout of a linearization pass: the partial row every kernel of the pass writes and the row sum adds, and the parameter
// structs the kernels take by value.  Included by linearize.hip (all kernels of the pass) and by the host-only translation units that
// read a reduced row (error_model.hip).
#pragma once
#include "cell_grid.hpp"
#include "common.hpp"
#include "device_math.hpp"
#include "kd_search.hpp"
#include "voxel_hash.hpp"

namespace sga {

constexpr int kTile = 256;           // threads per workgroup = source points per tile
constexpr int kRow = 96;             // doubles per partial row: [0, 29) the system (21 H, 6 b, e, inliers), [32, 95) the quadratic error model
constexpr int kCols = 128;           // columns the reduction kernels handle (>= kRow)
constexpr int kModelOff = 32;        // error model: [32, 41) sum p_a g_j, [41, 59) sum p_a M'_c, [59, 95) sum p_a p_b M'_c
constexpr int kModelCols = 95;
constexpr int kStatsCol = 30;        // spare columns 30, 31: search statistics of a grid pass (cell_grid.hip), not sums over points
constexpr int kSearchBlock = 64;      // search kernels: one wave per workgroup
#ifndef SGA_MAX_BLOCKS
#define SGA_MAX_BLOCKS 2048
#endif
constexpr int kMaxBlocks = SGA_MAX_BLOCKS;  // linearize_kernel / error_kernel / certify_linearize_kernel: 8 workgroups per CU
constexpr int kReduceGroups = 64;
constexpr int kReduceSlices = 8;  // 1024 threads = 8 slices of 128 columns

// The sums of one linearization, in MOMENT form.  With M' = R^T M R and g = R^T M r of a pair (source frame, device_math.hpp) and
// p = the source point, everything the optimizer needs is linear in
//   sum M'            sum g            sum p_a M'          sum p_a g          sum p_a p_b M'          sum e, #inliers
//   (6 = H_tt)        (3 = -b_t)       (18)                (9)                (36)
// because H_rt = sum skew(p) M', H_rr = sum skew(p) M' skew(p)^T and b_r = -sum skew(p) g only recombine those (derived_entry,
// evaluated once per pass by the reducing workgroup).  The same sums ARE the coefficients of the quadratic ERROR MODEL:
// Reduction::error (reduction_omp.hpp:61-70) evaluates sum_i 1/2 r_i^T M_i r_i at a trial pose with the correspondences and
// mahalanobis matrices CACHED by the last linearization (gicp_factor.hpp:80-89); with those frozen it is a quadratic polynomial in
// Y = [R^T R_n - I | R^T (tau_n - tau)] (trial pose (R_n, tau_n) relative to the linearization pose (R, tau)):
//   e(T_n) = e0 - sum_a Y[:,a] . S1[a] + 1/2 sum_ab Y[:,a]^T S2[a][b] Y[:,b],   S1[a] = sum p~_a g,  S2[a][b] = sum p~_a p~_b M'
// with p~ = (p, 1).  sga_error evaluates it on the host: no pass over the cloud, no device round trip.
// 74 sums instead of the 29 of the direct form, but a lane adds up PTS points before a value goes through the wave reduction (the
// DPP chain is what a sum costs): 74 * (PTS + 6) / PTS instructions per point instead of 29 * 7 + the skew products.
// Row layout: [0, 21) H, [21, 27) b, 27 e, 28 inliers, [32, 41) sum p_a g_j, [41, 59) sum p_a M'_c, [59, 95) sum p_a p_b M'_c
// (c = xx, xy, xz, yy, yz, zz; pairs ab = 00, 01, 02, 11, 12, 22); columns [0, 15) and [21, 24) are derived.

// Small grids (a 15k-point scan is 60 workgroups) fold the final reduction into the producer kernel: every workgroup publishes its
// partial row (agent-scope write-through stores), takes a ticket, and the workgroup that arrives last adds the rows in fixed order
// and hands the result over — one launch and one dependent-launch gap less per pass.  (With the 2048 workgroups of a 1M-point pass
// the ticket contention costs more than the launch: those keep the separate reduce_rows_kernel.)  Where the gain ends, measured late in
// round 6 on VGICP iterations of 3k ... 400k points (the workgroups of a streaming kernel finish together and take the ticket one after
// the other, an agent-scope acquire / release each): 12 workgroups -1.6 us per pass, 24 -0.6, 40 +1.1, 63 +3.4, 120 (30k points) +10,
// 235 (60k) +25, 245 (250k points at four per lane) +30 us — the limit was 256 since round 3.
constexpr int kFuseMaxBlocks = 32;
constexpr int kSeqWord = 128;  // h_accum: [0, 128) a result, word 128 the sequence number of the last published one
struct FusedTail {
  int enabled;
  unsigned* ticket;
  double* out;        // device result (out_n doubles)
  int out_n;
  double* host;       // pinned, device-mapped host result or null
  unsigned long long seq;
};

template <typename Real>
struct LinParams {
  const float4* __restrict__ src_pts;
  const Cov8* __restrict__ src_cov;
  int n;
  int num_tiles;
  const float4* __restrict__ tgt_pts;
  const float4* __restrict__ tgt_nrm;
  const Cov8* __restrict__ tgt_cov;
  KdView kd;
  VoxelView vox;
  FlatView flat;
  int* __restrict__ corr;
  const int* __restrict__ hint;  // exact nearest neighbour per source point at this pose (kd position) or -1, from nn_search_kernel
  const unsigned char* __restrict__ reject;  // optional: verdict of a host rejector per source point in the CALLER's order (1 = reject)
  Real* __restrict__ maha;  // n*6
  int store_maha;  // cache the mahalanobis matrices for the error kernel (robust factors); otherwise they are recomputed if ever asked for
  Rigid<Real> T;
  Real max_sq;   // INFINITY = no rejector; in the pair arithmetic's type: fp64 passes compare double distances with the double threshold (rejector.hpp)
  float bound2;  // a neighbour counts only if kd_dist2 < bound2 (max_sq nudged up by an ulp, or INFINITY); the walks reach a little farther
  int robust_kind;
  Real robust_c;
  double* __restrict__ partials;
  FusedTail tail;
  // warm pass with the certificate check inside the factor kernel (certify_linearize_kernel): the certificate of the previous
  // linearization pose T_prev is checked per point on the way through; a point whose certificate fails contributes nothing to the
  // streaming part, is flagged (rex[i] = -(exploration slack) < 0) and walks at the end of its workgroup's step
  int* __restrict__ cert_nn;
  int* __restrict__ cert_nn2;
  float* __restrict__ cert_rex;
  uint32_t* __restrict__ cert_walked;
  Rigid<Real> T_prev;
  float cert_within2, cert_slack_min, cert_slack_max;
  float cert_pad;  // headroom of the certificate check (see certify)
};

template <typename Real>
struct NNParams {
  const float4* __restrict__ src_pts;
  int n;
  KdView kd;
  Rigid<Real> T;
  float bound2;      // the walks find neighbours with kd_dist2 < bound2 (the rejector's reach + kSearchMargin)
  float within2;     // a neighbour counts for the rejector only if kd_dist2 < within2
  float slack_min, slack_max;  // exploration slack of a re-walk = clamp(motion, slack_min, slack_max) (kSlackMin / kSlackMax)
  float cert_pad;    // headroom of the certificate check as a share of the point's motion (see certify; SGA_CERT_PAD)
  int* __restrict__ nn;
  int* __restrict__ nn2;   // the runner-up of every walk: second candidate of the certificate
  float* __restrict__ rex;
  int check;         // warm pass
  Rigid<Real> T_prev;
  uint32_t* __restrict__ walked;  // statistics, one counter per wave tile: lanes of warm passes that had to walk
  const uint32_t* __restrict__ tile_order;  // launch slot -> tile (longest tile first), or null: slot = tile
  uint32_t* __restrict__ tile_cost;         // out, or null: duration of the tile's wave (100 MHz ticks)
  int* __restrict__ leaves;  // diagnostics (sga_problem_set_search_stats): leaves scanned per source point in this pass, or null
  double inv_leaf;   // 2^depth / n (kd_leaf_rank)
  int chunk_tiles;   // queue-fed kernel: tiles of 64 queries per wave
  int fast;          // one-query-per-lane kernels: walk with the fast leaf scan (exact repeat where it cannot decide)
  GridView grid;     // the target's cell grid (cell_grid.hpp), if grid_walk
  int grid_walk;     // the walkers of certify_linearize_kernel try ring 1 of the grid before they walk the tree
};

template <typename Real>
struct ErrParams {
  const float4* __restrict__ src_pts;
  int n;
  int num_tiles;
  const float4* __restrict__ tgt_pts;
  const float4* __restrict__ tgt_nrm;
  const int* __restrict__ corr;
  const Real* __restrict__ maha;
  Rigid<Real> T;
  int robust_kind;
  Real robust_c;
  double* __restrict__ partials;
  FusedTail tail;
};

// ---- batched registration (batch.hip): the rounds of B independent problems ---------------------------------
// One entry of a round's table per ACTIVE pair, largest pair first: what search_linearize_kernel receives as its two arguments, for
// that pair at its pose of the round.  The table lives in device memory (it does not fit the kernel-argument segment for large B); a
// wave reads its pair's entry with scalar loads (uniform_const).  A batch over voxel maps (batch_map_linearize_kernel) fills and reads
// `p` alone — p.vox / p.flat are the pair's own map: hash, leaf size, origin, search offsets — and leaves `q` and `seedless` zero.
struct BatchPair {
  NNParams<float> q;
  LinParams<float> p;
  int ntiles;    // 64-point tiles of the pair = its partial rows, p.partials[0, ntiles)
  int seedless;  // the walks start without the neighbour of an earlier pass (first round of a registration)
  int pair;      // position in the batch: the reduced row goes to host[pair * kRow]
  int pad;
};

}  // namespace sga

// Batched registration (batch.hip): B independent (target, source) problems of ONE context — the targets all kd-trees, all Gaussian
// voxel maps or all flat maps — whose linearizations run as one search + factor launch (maps: one factor launch, the lookup inside) and
// one row reduction per round, with one hand-off to the host for all pairs.
#pragma once
#include "common.hpp"

struct sga_batch {
  sga_context* ctx = nullptr;
  std::vector<sga_problem*> problems;  // borrowed: the caller destroys the batch first
  int kind = SGA_INDEX_KDTREE;         // the target kind all members share: SGA_INDEX_KDTREE, SGA_INDEX_VOXELMAP or SGA_INDEX_FLATMAP
  std::vector<int> tiles;              // 64-point tiles per pair (0: empty source or empty target); the pair's rows are its own partials[0, tiles).
                                       // Map batches: the source's tiles — whether the map holds anything is looked up per round (batch_pair_tiles)
  std::vector<long long> tile_prefix;  // tiles of the pairs before k (count + 1 entries): the whole batch must fit an int grid
  int max_depth = 0;                   // kd batches: deepest target tree, sizes the LDS traversal stack of the launch
  // the round table (pass_layout.hpp: BatchPair): filled by the host in pinned memory, copied to the device with one command per round
  void* h_round = nullptr;
  sga::DevBuf<unsigned char> d_round;
  size_t round_bytes = 0;
  // results: count x 96 doubles + the sequence word, pinned and device-mapped (the hand-off of reduce_rows_kernel, once for all pairs)
  double* h_out = nullptr;
  double* h_out_dev = nullptr;
  sga::DevBuf<unsigned> ticket;  // arrival counter of batch_reduce_rows_kernel, zero between launches
  unsigned long long seq = 0;
};

namespace sga {
size_t batch_round_bytes(size_t count);  // linearize.hip: bytes of a round table for `count` pairs
// One linearization round over the pairs with active[k] != 0 (null: all) at the caller-frame poses T (count x 16): enqueue, hand-off,
// wait.  Afterwards h_out[k * 96 ..] holds pair k's reduced row (device frames) and every active member problem the state a lone pass
// at that pose leaves: a cold kd pass (correspondences, certificates, error model) or a map pass (correspondences, error model).
// seedless: the walks ignore the neighbours of earlier passes (kd batches; a map lookup has no seed).
// The arguments have been validated (batch.hip: batch_check).
int batch_round(sga_context* ctx, sga_batch* bt, const sga_factor_params* fp, const double* T, const unsigned char* active, bool seedless);
// 64-point tiles of a pair as it stands now: none for an empty source or an empty target
inline int batch_pair_tiles(const sga_problem* pb) { return (pb->n > 0 && pb->target->n > 0) ? static_cast<int>((pb->n + 63) / 64) : 0; }
// pair k's row of the last round as the caller's H (36, exactly symmetric), b (6), e, inliers (batch.hip)
void batch_unpack(const sga_batch* bt, size_t k, double* H, double* b, double* e, uint64_t* num_inliers);
// validation of a batch call, before any device work (batch.hip)
int batch_check(sga_context* ctx, sga_batch* bt, const sga_factor_params* fp);
// device frames (frames.hip)
const double* problem_pose(const sga_problem* pb, const double T[16], double Td[16]);
void problem_system_to_caller(const sga_problem* pb, double H[36], double b[6]);
int problem_accumulator_to_caller(sga_context* ctx, const sga_problem* pb, double* d_out30);  // the same on the device, in place (asynchronous entry points)
int problem_check_shard_frames(sga_context* ctx, sga_problem* pb);
double error_model_value(const double* acc96, const double T_lin[16], const double T[16]);  // error_model.hip
bool error_model_enabled();  // linearize.hip
}  // namespace sga

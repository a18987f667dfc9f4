// Batched registration: B independent (target, source) problems of one context, linearized by ONE search + factor launch and
// ONE row reduction per round, with one hand-off to the host for all pairs.  The kernels and the round itself
// sit beside the lone kernels whose device functions they share (linearize.hip: batch_search_linearize_kernel for kd-tree targets,
// batch_map_linearize_kernel for voxel maps, batch_round; reduce_rows.hpp: batch_reduce_rows_kernel); the lock-step LM / GN loop over
// the pairs is optimizer.hip's (sga_align_batch).  This file: the batch object and sga_batch_linearize.
//
// Scope: the members' targets are ALL kd-trees, ALL Gaussian voxel maps or ALL flat maps (one-shot, incremental or created from host
// voxels; any mix of leaf sizes, search offsets and flat contents; one map may serve several members) — a mix of kinds and projective
// indexes are refused at creation; ICP, PLANE_ICP (kd-trees and flat maps with normals), GICP; distance or null rejector; fp32 pair
// arithmetic, no robust kernel, no host rejector, error model on — the conditions under which a lone kd pass fuses search and factors
// (plan_pass) and every lone pass answers trial errors from the quadratic model.  Everything else is refused before any device work.
#include <climits>
#include <memory>

#include "batch.hpp"

namespace sga {

int batch_check(sga_context* ctx, sga_batch* bt, const sga_factor_params* fp) {
  // the parameters first: what a batch cannot do is refused whatever it is asked of (also where there is no device to hold a batch)
  if (!fp) return fail(SGA_ERR_INVALID, "null argument");
  if (fp->factor_kind < 0 || fp->factor_kind > 2) return fail(SGA_ERR_INVALID, "invalid factor_kind %d", fp->factor_kind);
  if (fp->math_mode != SGA_MATH_FP32) return fail(SGA_ERR_UNSUPPORTED, "a batch computes in fp32 pair arithmetic only");
  if (fp->robust_kind != SGA_ROBUST_NONE) return fail(SGA_ERR_UNSUPPORTED, "a batch takes no robust kernel");
  if (!error_model_enabled()) return fail(SGA_ERR_UNSUPPORTED, "a batch answers trial errors from the error model (sga_set_error_model(0) is set)");
  if (!ctx || !bt) return fail(SGA_ERR_INVALID, "null argument");
  if (bt->ctx != ctx) return fail(SGA_ERR_INVALID, "the batch belongs to another context");
  if (ctx->sharded()) return fail(SGA_ERR_UNSUPPORTED, "a batch does not run on a sharded context");
  for (size_t k = 0; k < bt->problems.size(); k++) {  // the factor against each member's target: linearize_dispatch's conditions, status and wording
    const sga_problem* pb = bt->problems[k];
    const sga_index* idx = pb->target;
    const bool flat = idx->kind == SGA_INDEX_FLATMAP, gaussian = idx->kind == SGA_INDEX_VOXELMAP;
    if (pb->rejector_fn != nullptr) return fail(SGA_ERR_UNSUPPORTED, "a member problem has a host rejector");
    if (fp->factor_kind == SGA_GICP && ((pb->n > 0 && !pb->has_covs) || (idx->n > 0 && !idx->has_covs))) return fail(SGA_ERR_INVALID, "GICP needs covariances on both source and target (problem %zu)", k);
    if (fp->factor_kind == SGA_PLANE_ICP && (gaussian || ((flat || idx->n > 0) && !idx->has_normals)))
      return fail(SGA_ERR_UNSUPPORTED, "PLANE_ICP needs a kd-tree index over a target with normals (problem %zu)", k);
  }
  return SGA_OK;
}

// pair k's reduced row -> the caller's H, b, e, inliers.  A^T H' A of a framed pair (system_to_caller) is symmetric only to rounding:
// the upper triangle is mirrored, so that H is exactly symmetric for every pair, as it is for clouds at the origin
void batch_unpack(const sga_batch* bt, size_t k, double* H, double* b, double* e, uint64_t* num_inliers) {
  const sga_problem* pb = bt->problems[k];
  sga_unpack_accumulator(bt->h_out + k * SGA_MODEL_DOUBLES, H, b, e, num_inliers);
  if (origin_is_zero(pb->src_origin)) return;
  problem_system_to_caller(pb, H, b);
  for (int i = 0; i < 6; i++)
    for (int j = i + 1; j < 6; j++) H[6 * j + i] = H[6 * i + j];
}

}  // namespace sga

using namespace sga;

extern "C" {

int sga_batch_create(sga_context* ctx, sga_problem* const* problems, size_t count, sga_batch** out) {
  if (!ctx || !out || (count > 0 && !problems)) return fail(SGA_ERR_INVALID, "null argument");
  *out = nullptr;
  if (count > static_cast<size_t>(INT_MAX) / 8) return fail(SGA_ERR_INVALID, "too many problems for one batch");
  std::unique_ptr<sga_batch> bt(new sga_batch);
  bt->ctx = ctx;
  bt->tile_prefix.push_back(0);
  for (size_t k = 0; k < count; k++) {
    sga_problem* pb = problems[k];
    if (!pb) return fail(SGA_ERR_INVALID, "problem %zu is null", k);
    if (pb->owner != ctx || pb->device != ctx->device) return fail(SGA_ERR_INVALID, "problem %zu belongs to another context", k);
    for (size_t j = 0; j < k; j++)
      if (problems[j] == pb) return fail(SGA_ERR_INVALID, "problem %zu is in the batch twice", k);
    const int kind = pb->target->kind;
    if (kind != SGA_INDEX_KDTREE && kind != SGA_INDEX_VOXELMAP && kind != SGA_INDEX_FLATMAP) return fail(SGA_ERR_UNSUPPORTED, "a batch takes kd-tree, Gaussian voxel-map or flat-map targets (problem %zu)", k);
    if (k == 0) bt->kind = kind;
    if (kind != bt->kind) return fail(SGA_ERR_UNSUPPORTED, "the targets of a batch are all kd-trees, all Gaussian voxel maps or all flat maps (problem %zu)", k);
    if (pb->n > static_cast<size_t>(INT_MAX) - 64) return fail(SGA_ERR_INVALID, "problem %zu is too large", k);
    // a map may be filled after the batch was created: its pairs are counted with the tiles of their source, the most a round launches
    const int tiles = kind == SGA_INDEX_KDTREE ? batch_pair_tiles(pb) : static_cast<int>((pb->n + 63) / 64);
    bt->problems.push_back(pb);
    bt->tiles.push_back(tiles);
    bt->tile_prefix.push_back(bt->tile_prefix.back() + (tiles + 7) / 8 * 8);  // as launched: every pair's share padded to a multiple of 8
    if (kind == SGA_INDEX_KDTREE) bt->max_depth = std::max(bt->max_depth, pb->target->kd_depth);
  }
  if (bt->tile_prefix.back() > static_cast<long long>(INT_MAX)) return fail(SGA_ERR_INVALID, "the batch has more tiles than one grid holds");
  if (count > 0) {
    SGA_ENTER(ctx);
    bt->round_bytes = batch_round_bytes(count);
    SGA_TRY(bt->d_round.alloc(bt->round_bytes));
    SGA_TRY(bt->ticket.alloc(1));
    SGA_HIP(hipMemsetAsync(bt->ticket.p, 0, sizeof(unsigned), ctx->stream));
    const size_t out_bytes = (count * SGA_MODEL_DOUBLES + 1) * sizeof(double);
    if (hipHostMalloc(&bt->h_round, bt->round_bytes, hipHostMallocDefault) != hipSuccess) return fail(SGA_ERR_HIP, "hipHostMalloc failed");
    if (hipHostMalloc(reinterpret_cast<void**>(&bt->h_out), out_bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
      (void)hipHostFree(bt->h_round);
      return fail(SGA_ERR_HIP, "hipHostMalloc failed");
    }
    std::memset(bt->h_out, 0, out_bytes);
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&bt->h_out_dev), bt->h_out, 0) != hipSuccess) {
      (void)hipHostFree(bt->h_round);
      (void)hipHostFree(bt->h_out);
      return fail(SGA_ERR_HIP, "hipHostGetDevicePointer failed");
    }
  }
  *out = bt.release();
  return SGA_OK;
}

int sga_batch_destroy(sga_batch* bt) {
  if (!bt) return SGA_OK;
  if (bt->h_round || bt->h_out) {
    (void)hipSetDevice(bt->ctx->device);
    (void)hipStreamSynchronize(bt->ctx->stream);  // no round is in flight when its buffers go
    if (bt->h_round) (void)hipHostFree(bt->h_round);
    if (bt->h_out) (void)hipHostFree(bt->h_out);
  }
  delete bt;
  return SGA_OK;
}

int sga_batch_size(const sga_batch* bt, size_t* count) {
  if (!bt || !count) return fail(SGA_ERR_INVALID, "null argument");
  *count = bt->problems.size();
  return SGA_OK;
}

int sga_batch_linearize(sga_context* ctx, sga_batch* bt, const sga_factor_params* fp, const double* T, const unsigned char* active, double* H, double* b, double* e, uint64_t* num_inliers) {
  SGA_TRY(batch_check(ctx, bt, fp));
  const size_t count = bt->problems.size();
  if (count == 0) return SGA_OK;
  if (!T || !H || !b || !e) return fail(SGA_ERR_INVALID, "null argument");
  SGA_ENTER(ctx);
  SGA_TRY(batch_round(ctx, bt, fp, T, active, false));
  for (size_t k = 0; k < count; k++) {
    if (active != nullptr && !active[k]) continue;
    batch_unpack(bt, k, H + 36 * k, b + 6 * k, e + k, num_inliers ? num_inliers + k : nullptr);
  }
  return SGA_OK;
}

}  // extern "C"

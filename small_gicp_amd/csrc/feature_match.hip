// Nearest rows in feature space: sga_features_match — a tiled brute force in double.  Target rows are staged
// through LDS, each lane owns a source row; the targets are cut into chunks so that a small problem still fills the chip, and the
// chunks' winners meet in a fixed order.  No floating-point atomics: two calls give the same bytes.
#include "cloud_ops.hpp"
#include "forest.hpp"

#include <cmath>

namespace sga {
namespace {

constexpr int kFmBlock = 64;    // source rows of a workgroup: one lane each, one wave
constexpr int kFmTile = 32;     // target rows staged in LDS at a time
constexpr int kFmMaxDim = 128;
constexpr int kFmWaves = 4096;  // the chunks are chosen so that about this many waves run: four per SIMD, what 126 VGPRs allow

}  // namespace

// For every row i of A (n x D) the row of B[first_of_chunk, end_of_chunk) of least squared distance, formed in double from the fp32
// values, the bins summed in order; the first of equal distances wins (rows are met in ascending order).  The winner of chunk c goes to
// pd / pi[c * n + i] (+inf / -1 when no row gave a distance below +inf).
//   DT == 33: the lane's row lives in registers;  DT == 0: any D <= 128, the rows of the workgroup transposed in LDS ([bin][lane]).
template <int DT>
__global__ __launch_bounds__(kFmBlock) void feature_match_kernel(const float* __restrict__ A, uint32_t n, const float* __restrict__ B, uint32_t m, int D, uint32_t chunk_rows, double* __restrict__ pd, int* __restrict__ pi) {
  extern __shared__ float fm_sh[];  // [kFmTile * D] the tile; DT == 0: behind it [D][kFmBlock] the workgroup's own rows
  const int lane = threadIdx.x;
  const int dim = DT > 0 ? DT : D;
  float* tile = fm_sh;
  float* own = fm_sh + static_cast<size_t>(kFmTile) * dim;
  const uint32_t i = blockIdx.x * kFmBlock + lane;
  const uint32_t ic = min(i, n - 1u);  // (lanes behind the last row work on a copy of it and write nothing)
  float s[DT > 0 ? DT : 1];
  if constexpr (DT > 0) {
#pragma unroll
    for (int b = 0; b < DT; b++) s[b] = A[static_cast<size_t>(ic) * DT + b];
  } else {
    for (int b = 0; b < dim; b++) own[b * kFmBlock + lane] = A[static_cast<size_t>(ic) * dim + b];
  }
  const uint32_t first = blockIdx.y * chunk_rows, end = min(first + chunk_rows, m);
  double best = static_cast<double>(INFINITY);
  int bi = -1;
  for (uint32_t t0 = first; t0 < end; t0 += kFmTile) {
    const uint32_t rows = min(static_cast<uint32_t>(kFmTile), end - t0);
    __syncthreads();  // the tile of the round before has been read
    for (uint32_t w = lane; w < static_cast<uint32_t>(kFmTile) * dim; w += kFmBlock) tile[w] = w < rows * dim ? B[static_cast<size_t>(t0) * dim + w] : 0.f;
    __syncthreads();
    for (uint32_t t = 0; t < rows; t += 4) {  // four rows at a time: four independent chains of additions
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      const float* r = tile + static_cast<size_t>(t) * dim;
      if constexpr (DT > 0) {
#pragma unroll
        for (int b = 0; b < DT; b++) {
          const double v = static_cast<double>(s[b]);
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const double x = v - static_cast<double>(r[u * DT + b]);
            acc[u] += x * x;
          }
        }
      } else {
        for (int b = 0; b < dim; b++) {
          const double v = static_cast<double>(own[b * kFmBlock + lane]);
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const double x = v - static_cast<double>(r[u * dim + b]);
            acc[u] += x * x;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (t + u < rows && acc[u] < best) {
          best = acc[u];
          bi = static_cast<int>(t0 + t + u);
        }
    }
  }
  if (i < n) {
    pd[static_cast<size_t>(blockIdx.y) * n + i] = best;
    pi[static_cast<size_t>(blockIdx.y) * n + i] = bi;
  }
}

// The chunks' winners of source row i, met in ascending order of the chunks (= of the target rows: the lowest index wins a tie); with
// mutual, the same over the reverse search for the winner j: match[i] = j only when j's nearest source row is i.  match and dist (or
// null) are a slot of the staging ring, by its device address.
__global__ __launch_bounds__(256) void feature_match_final_kernel(const double* __restrict__ pd, const int* __restrict__ pi, uint32_t n, uint32_t chunks, const double* __restrict__ rd, const int* __restrict__ ri, uint32_t m, uint32_t rchunks,
                                                                  int mutual, long long* __restrict__ match, double* __restrict__ dist) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  double best = static_cast<double>(INFINITY);
  int j = -1;
  for (uint32_t c = 0; c < chunks; c++) {
    const double d = pd[static_cast<size_t>(c) * n + i];
    if (d < best) best = d, j = pi[static_cast<size_t>(c) * n + i];
  }
  if (mutual && j >= 0) {
    double back = static_cast<double>(INFINITY);
    int ib = -1;
    for (uint32_t c = 0; c < rchunks; c++) {
      const double d = rd[static_cast<size_t>(c) * m + j];
      if (d < back) back = d, ib = ri[static_cast<size_t>(c) * m + j];
    }
    if (ib != static_cast<int>(i)) j = -1;
  }
  match[i] = j;
  if (dist != nullptr) dist[i] = j >= 0 ? sqrt(best) : static_cast<double>(INFINITY);
  __threadfence_system();
}

namespace {

struct MatchPass {
  DevBuf<double> d;
  DevBuf<int> i;
  uint32_t chunks = 0;
};

// one direction of the search enqueued: A's rows against B's
int match_pass(sga_context* ctx, const sga_features* A, const sga_features* B, MatchPass* p) {
  const uint32_t n = static_cast<uint32_t>(A->n), m = static_cast<uint32_t>(B->n);
  const int D = A->dim;
  const uint32_t blocks = (n + kFmBlock - 1) / kFmBlock, tiles = (m + kFmTile - 1) / kFmTile;
  uint32_t chunks = std::min<uint32_t>(tiles, std::max<uint32_t>(1u, kFmWaves / blocks));
  const uint32_t chunk_rows = ((tiles + chunks - 1) / chunks) * kFmTile;
  chunks = (m + chunk_rows - 1) / chunk_rows;
  p->chunks = chunks;
  SGA_TRY(p->d.alloc(static_cast<size_t>(chunks) * n));
  SGA_TRY(p->i.alloc(static_cast<size_t>(chunks) * n));
  const dim3 grid(blocks, chunks);
  count_launch(Chain::FeatureMatch);
  if (D == SGA_FPFH_DIM)
    hipLaunchKernelGGL((feature_match_kernel<SGA_FPFH_DIM>), grid, dim3(kFmBlock), static_cast<size_t>(kFmTile) * D * sizeof(float), ctx->stream, A->rows.p, n, B->rows.p, m, D, chunk_rows, p->d.p, p->i.p);
  else
    hipLaunchKernelGGL((feature_match_kernel<0>), grid, dim3(kFmBlock), static_cast<size_t>(kFmTile + kFmBlock) * D * sizeof(float), ctx->stream, A->rows.p, n, B->rows.p, m, D, chunk_rows, p->d.p, p->i.p);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

int sga_features_match(sga_context* ctx, const sga_features* source, const sga_features* target, int mutual, int64_t* match, double* dist, size_t* matched) {
  if (!ctx || !source || !target || !match) return fail(SGA_ERR_INVALID, "null argument");
  if (mutual != 0 && mutual != 1) return fail(SGA_ERR_INVALID, "match: mutual %d is not 0 or 1", mutual);
  // ---- (from here on the handles are read)
  if (matched) *matched = 0;
  if (source->device != ctx->device || target->device != ctx->device) return fail(SGA_ERR_INVALID, "features live on another device");
  if (source->dim != target->dim) return fail(SGA_ERR_INVALID, "match: the source rows have %d values, the target rows %d", source->dim, target->dim);
  const size_t n = source->n, m = target->n;
  if (n >= (1ull << 31) || m >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many rows (%zu, %zu; limit 2^31-1)", n, m);
  if (source->dim < 1 || source->dim > kFmMaxDim) return fail(SGA_ERR_INVALID, "match: dim %d outside [1,%d]", source->dim, kFmMaxDim);
  if (n == 0 || m == 0) {  // nothing is launched
    for (size_t i = 0; i < n; i++) {
      match[i] = -1;
      if (dist) dist[i] = static_cast<double>(INFINITY);
    }
    return SGA_OK;
  }
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, source->ready));
  SGA_TRY(wait_ready(ctx, target->ready));
  MatchPass fwd, rev;  // live to the end of the call (then: the stream's free list)
  SGA_TRY(match_pass(ctx, source, target, &fwd));
  if (mutual) SGA_TRY(match_pass(ctx, target, source, &rev));
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, n * (sizeof(long long) + (dist != nullptr ? sizeof(double) : 0)), &slot));
  long long* match_dev = static_cast<long long*>(slot->dev);
  double* dist_dev = dist != nullptr ? reinterpret_cast<double*>(match_dev + n) : nullptr;
  count_launch(Chain::FeatureMatch);
  hipLaunchKernelGGL(feature_match_final_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, ctx->stream, fwd.d.p, fwd.i.p, static_cast<uint32_t>(n), fwd.chunks, rev.d.p, rev.i.p, static_cast<uint32_t>(m), rev.chunks, mutual,
                     match_dev, dist_dev);
  SGA_HIP(hipGetLastError());
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait: the winners are in the slot
  const long long* host = static_cast<const long long*>(slot->host);
  size_t count = 0;
  for (size_t i = 0; i < n; i++) {
    match[i] = host[i];
    count += host[i] >= 0 ? 1 : 0;
  }
  if (dist) std::memcpy(dist, host + n, n * sizeof(double));
  if (matched) *matched = count;
  return SGA_OK;
}

int sga_debug_features_match_launches(unsigned long long* launches) { return report_launches(Chain::FeatureMatch, launches); }

}  // extern "C"

// The row sum that ends every linearization pass and its hand-off to the host: the derived columns of a row in moment form, the tail
// small grids run inside the producing kernel, the two reduction kernels and their launch.  The kernels are compiled by linearize.hip,
// the only translation unit that includes this file.
#pragma once
#include <algorithm>

#include "pass_layout.hpp"
#include "uniform.hpp"

namespace sga {

__host__ __device__ inline double derived_entry(int col, const double* m) {
  // position of (j, k) in a packed symmetric 3x3 {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}}, four bits each in one immediate: a table indexed at run
  // time would live in constant memory, and its loads, cold in every launch, would stand between the last fold and the hand-off
  auto S = [](int j, int k) { return static_cast<int>((0x542431210ull >> (4 * (3 * j + k))) & 15ull); };
  auto A = [&](int a, int j, int k) { return m[kModelOff + 9 + 6 * a + S(j, k)]; };                   // sum p_a M'_jk
  auto B = [&](int a, int b, int j, int k) { return m[kModelOff + 27 + 6 * S(a, b) + S(j, k)]; };     // sum p_a p_b M'_jk
  auto G = [&](int a, int j) { return m[kModelOff + 3 * a + j]; };                                    // sum p_a g_j
  // K = skew(p) M': K_ik = p_i1 M'_i2,k - p_i2 M'_i1,k  (i1 = i + 1, i2 = i + 2 mod 3)
  auto PK = [&](int l, int i, int k) { const int i1 = (i + 1) % 3, i2 = (i + 2) % 3; return B(l, i1, i2, k) - B(l, i2, i1, k); };  // sum p_l K_ik
  if (col >= 21) {  // b_r = -sum p x g
    const int i = col - 21, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    return G(i2, i1) - G(i1, i2);
  }
  // upper triangle of H, row-wise: row i starts at 6 i - i (i - 1) / 2
  const int i = col < 6 ? 0 : (col < 11 ? 1 : 2);
  const int j = col - (6 * i - i * (i - 1) / 2) + i;  // column in the 6x6
  if (j >= 3) {  // H_rt = sum K
    const int k = j - 3, i1 = (i + 1) % 3, i2 = (i + 2) % 3;
    return A(i1, i2, k) - A(i2, i1, k);
  }
  // H_rr = sum K skew(p)^T: [i][j] = p_j1 K_i,j2 - p_j2 K_i,j1
  const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
  return PK(j1, i, j2) - PK(j2, i, j1);
}
__host__ __device__ inline bool is_derived_col(int c) { return c < 15 || (c >= 21 && c < 24); }

// derive: the row holds a linearization in moment form — its derived columns are filled in from the totals (derived_entry)
__device__ __forceinline__ void fused_tail(const FusedTail& f, const double* __restrict__ partials, int nrows, int ncols, int row_stride, bool derive = false) {
  __shared__ unsigned sh_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this workgroup's row has left the CU
  __syncthreads();
  // agent-scope release (this workgroup's row, ordered before by the barrier) / acquire (the rows of the workgroups that arrived earlier)
  if (threadIdx.x == 0) sh_last = __hip_atomic_fetch_add(f.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == static_cast<unsigned>(nrows - 1) ? 1u : 0u;
  __syncthreads();
  if (!sh_last) return;  // workgroup-uniform
  // 2 slices of 128 columns: slice s adds rows s, s + 2, ... (independent loads), then the slices are added in fixed order
  __shared__ double sh_slice[2][kCols];
  {
    const int c = threadIdx.x & (kCols - 1), sl = threadIdx.x / kCols;
    double t = 0.0;
    if (c < ncols && sl < 2)
      for (int r = sl; r < nrows; r += 2) t += __hip_atomic_load(&partials[static_cast<size_t>(r) * row_stride + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (sl < 2) sh_slice[sl][c] = t;
  }
  __syncthreads();
  if (derive) {  // workgroup-uniform
    if (threadIdx.x < kCols) sh_slice[0][threadIdx.x] += sh_slice[1][threadIdx.x];
    __syncthreads();
    if (threadIdx.x < kCols) sh_slice[1][threadIdx.x] = 0.0;
    __syncthreads();
  }
  if (threadIdx.x < kCols) {
    const int c = threadIdx.x;
    const double t = (derive && is_derived_col(c)) ? derived_entry(c, sh_slice[0]) : sh_slice[0][c] + sh_slice[1][c];
    if (c < f.out_n) {
      const double v = c < ncols ? t : 0.0;
      f.out[c] = v;
      if (f.host != nullptr) f.host[c] = v;
    }
  }
  if (threadIdx.x == 0) __hip_atomic_store(f.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch on this stream
  if (f.host != nullptr) {
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(f.host + kSeqWord), f.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// Deterministic fp64 sum of `nrows` partial rows of `ncols` (<= 32) doubles in ONE launch of G = 32 workgroups: workgroup g sums
// rows g, g+G, g+2G, ... into row g of `stage`; the workgroup that finishes LAST (a ticket counter) adds the G stage rows in fixed
// order — which workgroup that is changes nothing in the arithmetic — and writes out[ncols] (+ zero padding up to out_n).
// Hand-off between workgroups (per-CU L1s and per-XCD L2s are not coherent): a workgroup writes its stage row, a barrier orders the
// row before lane 0's ticket increment, which is an agent-scope release / acquire (the row accesses themselves are agent-scope
// relaxed atomics, i.e. write-through stores and cache-bypassing loads); only these <= 64 workgroups touch the ticket.  (Putting the ticket into the 2048 workgroups of the producer kernel was measured: +20 us.)
// When `host` is given the result is handed to the host right here: copied into pinned, device-mapped host memory, then a
// sequence number is published (system-scope release) on which the host spins.  This replaces hipMemcpyAsync +
// hipStreamSynchronize, whose fixed cost is paid twice per optimizer iteration.
#ifdef SGA_REDUCE_STAMPS
// diagnostics build (make stamps): 100 MHz wall clock at six points of reduce_rows_kernel — 0 entry, 1 end of stage 1, 2 after the
// ticket, 3 end of stage 2, 4 after the host stores, 5 after the system fence — taken by thread 0 of the first workgroup ([0, 6)), of
// the last one ([8, 14)) and of the one that arrived last and finished the sum ([16, 22); [22] its index, [23] the workgroups)
static __device__ unsigned long long g_reduce_stamps[24];
#define SGA_STAMP(k)                                                                         \
  do {                                                                                       \
    if (threadIdx.x == 0) {                                                                  \
      const unsigned long long stamp_now = wall_clock64();                                   \
      stamp_local[k] = stamp_now;                                                            \
      if (blockIdx.x == 0) g_reduce_stamps[k] = stamp_now;                                   \
      if (blockIdx.x == gridDim.x - 1) g_reduce_stamps[8 + (k)] = stamp_now;                 \
    }                                                                                        \
  } while (0)
#else
#define SGA_STAMP(k) ((void)0)
#endif

__global__ __launch_bounds__(kReduceSlices * kCols) void reduce_rows_kernel(
  const double* __restrict__ partials, int nrows, int ncols, int row_stride, double* __restrict__ stage, unsigned* __restrict__ ticket, double* __restrict__ out, int out_n, double* __restrict__ host,
  unsigned long long seq, int derive, const uint32_t* __restrict__ stats) {
  __shared__ double sh[kReduceSlices][kCols];
  __shared__ unsigned sh_ticket;
  const int c = threadIdx.x & (kCols - 1), s = threadIdx.x / kCols;
  const int G = gridDim.x;
#ifdef SGA_REDUCE_STAMPS
  unsigned long long stamp_local[6] = {0, 0, 0, 0, 0, 0};
#endif
  SGA_STAMP(0);
  // stage 1: (workgroup g, slice s) adds rows g + G * s, g + G * (s + 8), ...: four independent chains, the loads of a chain in flight together
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < ncols) {
    const int step = G * kReduceSlices;
    int r = blockIdx.x + G * s;
    for (; r + 3 * step < nrows; r += 4 * step) {
      const double v0 = partials[static_cast<size_t>(r) * row_stride + c], v1 = partials[static_cast<size_t>(r + step) * row_stride + c];
      const double v2 = partials[static_cast<size_t>(r + 2 * step) * row_stride + c], v3 = partials[static_cast<size_t>(r + 3 * step) * row_stride + c];
      a0 += v0, a1 += v1, a2 += v2, a3 += v3;
    }
    for (; r < nrows; r += step) a0 += partials[static_cast<size_t>(r) * row_stride + c];
  }
  sh[s][c] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  auto fold = [&]() {  // sh[0][c] = sum over the slices, fixed order
    if (threadIdx.x < kCols) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < kReduceSlices; k++) t += sh[k][threadIdx.x];
      sh[0][threadIdx.x] = t;
    }
    __syncthreads();
  };
  fold();
  SGA_STAMP(1);
  if (G > 1) {
    if (threadIdx.x < kCols) __hip_atomic_store(&stage[blockIdx.x * kCols + threadIdx.x], sh[0][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) sh_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);  // release this workgroup's stage row, acquire the earlier ones
    __syncthreads();
    SGA_STAMP(2);
    if (sh_ticket != static_cast<unsigned>(G - 1)) return;  // workgroup-uniform
    // the last workgroup adds the G <= 64 stage rows: slice s takes rows s, s + 8, ...: at most 8 loads per thread, all in flight
    double v[kReduceGroups / kReduceSlices];
#pragma unroll
    for (int k = 0; k < kReduceGroups / kReduceSlices; k++) {
      const int g = s + k * kReduceSlices;
      v[k] = g < G ? __hip_atomic_load(&stage[g * kCols + c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    }
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kReduceGroups / kReduceSlices; k++) t += v[k];
    __syncthreads();
    sh[s][c] = t;
    __syncthreads();
    fold();
  }
  SGA_STAMP(3);
  if (threadIdx.x < kCols) {
    const int cc = threadIdx.x;
    const double t = (derive && is_derived_col(cc)) ? derived_entry(cc, sh[0]) : sh[0][cc];  // moment form: H_rr, H_rt, b_r from the totals
    if (cc < out_n) {
      double r = cc < ncols ? t : 0.0;
      if (stats != nullptr && (cc == kStatsCol || cc == kStatsCol + 1)) r = static_cast<double>(stats[cc - kStatsCol]);  // a grid pass's search statistics ride along in two spare columns
      out[cc] = r;
      if (host != nullptr) host[cc] = r;
    }
  }
  if (G > 1 && threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch on this stream
  if (host != nullptr) {
    SGA_STAMP(4);
    // only the two waves that stored the result fence it; all sixteen meet at the barrier.  (A system-scope fence writes the L2 back and
    // invalidates it, ~0.15 us per wave, one wave after the other: sixteen of them stood 2.6 us in front of the sequence word, two 0.7:
    // profiles/reduce_chain_split.txt, blocks 2 and 3.)
    if (threadIdx.x < kCols) __threadfence_system();
    __syncthreads();
    SGA_STAMP(5);
    if (threadIdx.x == 0) __hip_atomic_store(reinterpret_cast<unsigned long long*>(host + kSeqWord), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
#ifdef SGA_REDUCE_STAMPS
  if (threadIdx.x == 0) {  // the workgroup that finished the sum
    for (int k = 0; k < 6; k++) g_reduce_stamps[16 + k] = stamp_local[k];
    g_reduce_stamps[22] = blockIdx.x, g_reduce_stamps[23] = gridDim.x;
  }
#endif
}

// The sums of a round: workgroup k adds the rows of the k-th active pair in the fixed order of reduce_rows_kernel's single-workgroup form
// (slice s: rows s, s + 8, ... in four chains; then the slices), derives the moment-form columns and stores the pair's kRow doubles
// into the pinned, device-mapped result block.  The workgroup that arrives last publishes the round's sequence number: ONE hand-off
// for all pairs (the release / acquire chain of box_reduce_publish, notes.hpp).
__global__ __launch_bounds__(kReduceSlices * kCols) void batch_reduce_rows_kernel(const BatchPair* __restrict__ pairs, unsigned* __restrict__ ticket, double* __restrict__ host, double* __restrict__ seq_word, unsigned long long seq) {
  __shared__ double sh[kReduceSlices][kCols];
  __shared__ unsigned sh_ticket;
  const BatchPair* d = uniform_const(pairs + blockIdx.x);
  const double* __restrict__ partials = d->p.partials;
  const int nrows = d->ntiles, out_row = d->pair;
  const int c = threadIdx.x & (kCols - 1), s = threadIdx.x / kCols;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (c < kModelCols) {
    constexpr int step = kReduceSlices;
    int r = s;
    for (; r + 3 * step < nrows; r += 4 * step) {
      const double v0 = partials[static_cast<size_t>(r) * kRow + c], v1 = partials[static_cast<size_t>(r + step) * kRow + c];
      const double v2 = partials[static_cast<size_t>(r + 2 * step) * kRow + c], v3 = partials[static_cast<size_t>(r + 3 * step) * kRow + c];
      a0 += v0, a1 += v1, a2 += v2, a3 += v3;
    }
    for (; r < nrows; r += step) a0 += partials[static_cast<size_t>(r) * kRow + c];
  }
  sh[s][c] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (threadIdx.x < kCols) {
    double t = 0.0;
#pragma unroll
    for (int k = 0; k < kReduceSlices; k++) t += sh[k][threadIdx.x];
    sh[0][threadIdx.x] = t;
  }
  __syncthreads();
  if (threadIdx.x < kRow) {
    const int cc = threadIdx.x;
    const double t = is_derived_col(cc) ? derived_entry(cc, sh[0]) : sh[0][cc];
    host[static_cast<size_t>(out_row) * kRow + cc] = cc < kModelCols ? t : 0.0;
  }
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) sh_ticket = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (sh_ticket != gridDim.x - 1) return;  // workgroup-uniform
  if (threadIdx.x == 0) {
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next round
    __threadfence_system();
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(seq_word), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

// partial rows (one per workgroup of linearize_kernel / error_kernel, or one per 64 source points when the search kernel does the factor algebra itself);
// the stage-1 rows of the reduction follow them
static size_t partial_rows(size_t n) { return std::max<size_t>(kMaxBlocks, (n + 63) / 64); }

static int reduce_groups(int nrows) { return nrows > 256 ? std::min(kReduceGroups, std::max(8, nrows / 128)) : 1; }  // <= 256 rows: one workgroup, no hand-off between workgroups

static void launch_reduce(sga_context* ctx, const double* partials, int nrows, int ncols, int row_stride, double* stage, double* out, int out_n, double* host, unsigned long long seq, bool derive = false, const uint32_t* stats = nullptr) {
  const int groups = reduce_groups(nrows);
  hipLaunchKernelGGL(reduce_rows_kernel, dim3(groups), dim3(kReduceSlices * kCols), 0, ctx->stream, partials, nrows, ncols, row_stride, stage, ctx->d_ticket.p, out, out_n, host, seq, derive ? 1 : 0, stats);
}

}  // namespace sga

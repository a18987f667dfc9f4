// The bounding box of a cloud's records in double, as the cloud kernels reduce it (pack, merge, deskew, crop): the ordered encoding, the
// workgroup's reduction, the note of a launch that serves one cloud and the per-member hand-off of a launch that serves many.
#pragma once
#include <cmath>

#include "cloud_ops.hpp"
#include "device_io.hpp"
#include "forest.hpp"
#include "notes.hpp"

namespace sga {

// order-preserving unsigned encoding of doubles (atomicMin / atomicMax on 64-bit words)
__host__ __device__ inline unsigned long long box_enc64(double d) {
  unsigned long long u;
  memcpy(&u, &d, 8);
  return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__host__ __device__ inline double box_dec64(unsigned long long e) {
  const unsigned long long u = (e >> 63) ? e & 0x7fffffffffffffffull : ~e;
  double d;
  memcpy(&d, &u, 8);
  return d;
}

// The box of a workgroup's threads (lo = +inf / hi = -inf for none) joined into acc = {min x y z, max x y z (encoded), ...} with six
// atomics; on return they have been issued and fenced (agent scope) and the workgroup has met.  Called by all threads.
__device__ __forceinline__ void box64_reduce_block(double lo[3], double hi[3], unsigned long long* __restrict__ acc) {
  __shared__ double sh_box[kIoBlock / 64][6];
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      lo[k] = fmin(lo[k], __shfl_xor(lo[k], off));
      hi[k] = fmax(hi[k], __shfl_xor(hi[k], off));
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
      sh_box[wave][k] = lo[k];
      sh_box[wave][3 + k] = hi[k];
    }
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    double v = sh_box[0][k];
    for (int w = 1; w < kIoBlock / 64; w++) v = k < 3 ? fmin(v, sh_box[w][k]) : fmax(v, sh_box[w][k]);
    if (k < 3)
      atomicMin(&acc[k], box_enc64(v));
    else
      atomicMax(&acc[k], box_enc64(v));
  }
  __threadfence();
  __syncthreads();
}

// box_reduce_publish for doubles: d_box64 = {min x y z, max x y z (encoded), arrival counter, 0}, identity values and counter 0 between
// launches; the last workgroup writes the six words into payload words 1..6 of the note, restores the accumulator and publishes.
__device__ __forceinline__ void box64_reduce_publish(double lo[3], double hi[3], unsigned long long* __restrict__ d_box64, unsigned long long* __restrict__ slot, unsigned long long seq) {
  __shared__ bool sh_last;
  box64_reduce_block(lo, hi, d_box64);
  if (threadIdx.x == 0) sh_last = __hip_atomic_fetch_add(&d_box64[6], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  if (!sh_last) return;  // workgroup-uniform
  if (threadIdx.x < 6) {
    const int k = threadIdx.x;
    slot[1 + k] = __hip_atomic_load(&d_box64[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&d_box64[k], box_enc64(k < 3 ? static_cast<double>(INFINITY) : -static_cast<double>(INFINITY)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (threadIdx.x == 0) __hip_atomic_store(&d_box64[6], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) note_publish(slot, seq);
}

// ---- one box per member of a batched launch (deskew, crop): the host side ------------------------------------------------------------------
// A member has eight words of the call's table — acc = {min x y z, max x y z (encoded), two words of the kernel's own}, identity values
// and zeros when the launch starts — and a slot of kBoxSlotWords words in the context's box block (cloud_ops.hpp), which its last
// workgroup writes before it arrives (forest_box_arrive; written in both kernels: a shared device function moved crop_cloud_kernel's
// register row, profiles/cloud_ops_kernel_resources.txt).  add: the accumulators and the ticket as sections of the call's table; init:
// their values at the start, into the zeroed host image; begin: the table's device memory (it lives to the end of the call) and the call's
// begin, `hand` is what the kernel receives; read: after the wait, member j's box — of its records — kept with its cloud.
struct MemberBoxes {
  TableSection<unsigned long long> acc;
  TableSection<unsigned> ticket;
  void add(TableLayout& lay, size_t members) { acc = lay.add<unsigned long long>(8 * members), ticket = lay.add<unsigned>(1); }
  void init(unsigned long long* host) const {
    for (size_t w = 0; w < acc.count; w++)
      if (w % 8 < 6) TableLayout::at(acc, host)[w] = box_enc64(w % 8 < 3 ? INFINITY : -INFINITY);
  }
  int begin(sga_context* ctx, const TableLayout& lay, DevBuf<unsigned long long>& table, ForestBoxes* hand) const {
    SGA_TRY(table.alloc(lay.words()));
    *hand = ForestBoxes{nullptr, 0u, nullptr, 0ull};
    if (acc.count == 0) return SGA_OK;  // (a call without boxes)
    SGA_TRY(forest_call_begin(ctx, acc.count / 8, kBoxSlotWords, &hand->seq));
    *hand = ForestBoxes{TableLayout::at(ticket, table.p), static_cast<unsigned>(acc.count / 8), ctx->h_forest_dev, hand->seq};
    return SGA_OK;
  }
  static void read(const sga_context* ctx, size_t j, sga_cloud* c) {
    const unsigned long long* slot = forest_slot_host(ctx, j, kBoxSlotWords);
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) lo[a] = box_dec64(slot[kBoxSlotLo + a]), hi[a] = box_dec64(slot[kBoxSlotHi + a]);
    cloud_set_box(c, lo, hi, true, false);
  }
};

}  // namespace sga

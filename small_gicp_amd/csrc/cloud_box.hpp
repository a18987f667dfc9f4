// The bounding box of a cloud's records in double, as the cloud kernels reduce it (cloud.hip: pack, merge, deskew; cloud_crop.hip: crop):
// the ordered encoding, the workgroup's reduction into a 64-bit accumulator, and the box a cloud keeps on the host.
#pragma once
#include <cmath>

#include "device_io.hpp"

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

// cloud.hip.  The box of the records (device frame) from the box of the inputs, when there is one (lo <= hi): fp32 of (box - origin) —
// relative: the inputs ARE the records — rounded outwards on request.
void cloud_set_box(sga_cloud* c, const double lo[3], const double hi[3], bool relative, bool outward);

}  // namespace sga

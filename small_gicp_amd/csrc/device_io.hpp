// What the entry points that read or write caller memory on the device share (cloud_io.hip, cloud_pose.hip, cloud_crop.hip, problem.hip; defined in device_io.hip): the
// checks of a caller's pointers, the ordering of a caller's stream against the context's, and the strided row loads of their kernels.
#pragma once
#include "common.hpp"

namespace sga {

// dtype / cols / stride of one array (nothing is dereferenced but the struct itself)
int check_layout(const sga_device_array* a, const char* what, bool is_cov);
// [p, p + bytes) must be device memory of the context's device, inside one allocation
int check_device_range(const sga_context* ctx, const void* p, size_t bytes, size_t align, const char* what, const char* host_entry);
int check_array(const sga_context* ctx, const sga_device_array* a, size_t rows, const char* what, const char* host_entry);

// The caller's stream before, the context's stream behind: an event on user_stream the context's stream waits for ahead of the first
// kernel that touches caller memory (io_begin), an event behind the last such kernel that user_stream waits for (io_end).  No host wait.
struct IoOrder {
  hipStream_t user = nullptr;
  bool active = false;
};
int io_begin(sga_context* ctx, void* user_stream, int flags, IoOrder* ord);
int io_end(sga_context* ctx, const IoOrder& ord);

constexpr int kIoBlock = 256;    // points per workgroup
constexpr int kIoTile = 2048;    // elements of the LDS tile rows are staged through (8 KB of floats, 16 KB of doubles)

// Rows [base, base + 256) of a strided array, the NV entries sel[] of each: thread t gets row base + t.  The rows are contiguous in
// memory (stride elements each, the unused ones included), so the workgroup reads them with unit-stride loads into an LDS tile — every
// line is touched once, which matters most for pinned host memory behind PCIe: mapped memory is not cached, and a per-thread stride of
// 12 bytes would touch every line three times — and each thread then picks its entries; rows wider than the tile are read where they
// are.  Called by all threads of the workgroup (barriers inside); rows at or past n give zeros.
template <typename T, int NV>
__device__ __forceinline__ void load_rows(const T* __restrict__ src, size_t base, size_t n, int stride, const int (&sel)[NV], T* __restrict__ sh, T (&out)[NV]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int v = 0; v < NV; v++) out[v] = T(0);
  const int rows = stride <= kIoTile ? min(kIoBlock, kIoTile / stride) : 0;
  if (rows == 0) {
    if (base + t < n) {
#pragma unroll
      for (int v = 0; v < NV; v++) out[v] = src[(base + t) * static_cast<size_t>(stride) + sel[v]];
    }
    return;
  }
  const size_t fend = n * static_cast<size_t>(stride);
  const int count = rows * stride;
  for (int r0 = 0; r0 < kIoBlock; r0 += rows) {  // (workgroup-uniform trip count)
    const size_t f0 = (base + r0) * static_cast<size_t>(stride);
    if (f0 >= fend) break;
    for (int e = t; e < count; e += kIoBlock) sh[e] = f0 + e < fend ? src[f0 + e] : T(0);
    __syncthreads();
    if (t >= r0 && t < r0 + rows) {
#pragma unroll
      for (int v = 0; v < NV; v++) out[v] = sh[(t - r0) * stride + sel[v]];
    }
    __syncthreads();
  }
}

}  // namespace sga

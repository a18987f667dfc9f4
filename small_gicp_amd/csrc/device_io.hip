// Device-resident clouds, queries and results: what the entry points that take their data from, and leave their
// results in, device memory of the context's device have in common (device_io.hpp) — sga_cloud_create_device, sga_cloud_export_device
// (cloud_io.hip), sga_index_knn_device, sga_problem_get_factors_device (problem.hip).  Nothing of the caller's data touches the host; the
// caller's stream and the context's are ordered by two events (io_begin / io_end), never by a host wait.  Every caller pointer is checked
// against the allocation it lies in before a kernel is given it: a wrong row count must be an error code, not a fault on a device other
// people are using.
#include "device_io.hpp"

namespace sga {

static size_t elem_size(int dtype) { return dtype == SGA_F64 ? 8 : 4; }

int check_layout(const sga_device_array* a, const char* what, bool is_cov) {
  if (a->dtype != SGA_F32 && a->dtype != SGA_F64) return fail(SGA_ERR_INVALID, "%s: dtype %d is neither SGA_F32 nor SGA_F64", what, a->dtype);
  if (is_cov ? (a->cols != 6 && a->cols != 9 && a->cols != 16) : a->cols != 3) return fail(SGA_ERR_INVALID, "%s: cols = %d (%s)", what, a->cols, is_cov ? "covariances are 6, 9 or 16 per row" : "3 per row");
  if (a->stride < a->cols) return fail(SGA_ERR_INVALID, "%s: stride %d < cols %d", what, a->stride, a->cols);
  return SGA_OK;
}

int check_device_range(const sga_context* ctx, const void* p, size_t bytes, size_t align, const char* what, const char* host_entry) {
  if (p == nullptr) return fail(SGA_ERR_INVALID, "%s: null data pointer", what);
  if (reinterpret_cast<uintptr_t>(p) % align != 0) return fail(SGA_ERR_INVALID, "%s: %p is not aligned to its %zu-byte elements", what, p, align);
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();  // an ordinary (pageable) host pointer
    return fail(SGA_ERR_INVALID, "%s: %p is not device memory (pageable host memory?): host arrays go through %s", what, p, host_entry);
  }
  if (at.type != hipMemoryTypeDevice) return fail(SGA_ERR_INVALID, "%s: %p is host memory, not device memory: host arrays, pinned or pageable, go through %s", what, p, host_entry);
  if (at.device != ctx->device) return fail(SGA_ERR_INVALID, "%s: %p lives on device %d, the context on device %d", what, p, at.device, ctx->device);
  hipDeviceptr_t base = nullptr;
  size_t size = 0;
  if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SGA_ERR_INVALID, "%s: the allocation of %p is unknown to the runtime", what, p);
  }
  const uintptr_t b = reinterpret_cast<uintptr_t>(base), q = reinterpret_cast<uintptr_t>(p);
  if (q < b || bytes > size || q - b > size - bytes) return fail(SGA_ERR_INVALID, "%s: [%p, +%zu bytes) reaches past its allocation [%p, +%zu bytes)", what, p, bytes, base, size);
  return SGA_OK;
}
int check_array(const sga_context* ctx, const sga_device_array* a, size_t rows, const char* what, const char* host_entry) {
  size_t bytes = 0;
  if (__builtin_mul_overflow(rows * elem_size(a->dtype), static_cast<size_t>(a->stride), &bytes)) return fail(SGA_ERR_INVALID, "%s: %zu rows of stride %d overflow the address space", what, rows, a->stride);
  return check_device_range(ctx, a->data, bytes, elem_size(a->dtype), what, host_entry);
}

int io_begin(sga_context* ctx, void* user_stream, int flags, IoOrder* ord) {
  ord->user = static_cast<hipStream_t>(user_stream);
  ord->active = ord->user != ctx->stream && !(flags & SGA_IO_NO_ORDER);
  if (!ord->active) return SGA_OK;
  if (!ctx->ev_io_in) SGA_HIP(hipEventCreateWithFlags(&ctx->ev_io_in, hipEventDisableTiming));
  if (!ctx->ev_io_out) SGA_HIP(hipEventCreateWithFlags(&ctx->ev_io_out, hipEventDisableTiming));
  SGA_HIP(hipEventRecord(ctx->ev_io_in, ord->user));
  SGA_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_io_in, 0));
  return SGA_OK;
}
int io_end(sga_context* ctx, const IoOrder& ord) {
  if (ord.active) {
    SGA_HIP(hipEventRecord(ctx->ev_io_out, ctx->stream));
    SGA_HIP(hipStreamWaitEvent(ord.user, ctx->ev_io_out, 0));
  }
  if (!ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

}  // namespace sga

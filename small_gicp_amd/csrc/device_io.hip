// Device-resident clouds, queries and results: the entry points that take their data from, and leave their results
// in, device memory of the context's device — sga_cloud_create_device, sga_cloud_export_device, sga_index_knn_device,
// sga_problem_get_factors_device.  Nothing of the caller's data touches the host; the caller's stream and the context's are ordered by two
// events (io_begin / io_end), never by a host wait.  Every caller pointer is checked against the allocation it lies in before a kernel
// is given it: a wrong row count must be an error code, not a fault on a device other people are using.
#include "common.hpp"
#include "notes.hpp"

#include <cmath>
#include <memory>

namespace sga {

// problem.hip: the launches of index_knn_impl / sga_problem_get_factors on device buffers, nothing else
int index_knn_check_k(const sga_index* index, int k);
int index_knn_enqueue(sga_context* ctx, const sga_index* index, const float* d_q, size_t m, int k, double max_sq_dist, long long* d_idx, float* d_sq_dist);
int problem_factors_enqueue(sga_context* ctx, const sga_problem* pb, long long* d_idx, float* d_m);

namespace {

constexpr int kIoBlock = 256;    // points per workgroup
constexpr int kIoTile = 2048;    // elements of the LDS tile rows are staged through (8 KB of floats, 16 KB of doubles)

// Rows [base, base + 256) of a strided array, the NV entries sel[] of each: thread t gets row base + t.  The rows are contiguous in
// memory (stride elements each, the unused ones included), so the workgroup reads them with unit-stride loads into an LDS tile — every
// line is touched once, as pack_cloud_kernel does for stride 3 — and each thread then picks its entries; rows wider than the tile are
// read where they are.  Called by all threads of the workgroup (barriers inside); rows at or past n give zeros.
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

// box_reduce_publish for doubles: d_box64 = {min x y z, max x y z (encoded), arrival counter, 0}, identity values and counter 0 between
// launches; the last workgroup writes the six words into payload words 1..6 of the note, restores the accumulator and publishes.
__device__ __forceinline__ void box64_reduce_publish(double lo[3], double hi[3], unsigned long long* __restrict__ d_box64, unsigned long long* __restrict__ slot, unsigned long long seq) {
  __shared__ double sh_box[kIoBlock / 64][6];
  __shared__ bool sh_last;
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
      atomicMin(&d_box64[k], box_enc64(v));
    else
      atomicMax(&d_box64[k], box_enc64(v));
  }
  __threadfence();
  __syncthreads();
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

// the six entries of a covariance row: packed (6), 3x3 (9) or the reference's 4x4 (16) — m[0], m[1], m[2], m[5], m[6], m[10] of a 4x4
struct CovSel {
  int s[6];
};
inline CovSel cov_sel(int cols) {
  if (cols == 9) return {{0, 1, 2, 4, 5, 8}};
  if (cols == 16) return {{0, 1, 2, 5, 6, 10}};
  return {{0, 1, 2, 3, 4, 5}};
}

struct PackArgs {
  const void* xyz;  // rows of sx elements, the first three used; null: attributes only
  const void* nrm;  // or null
  const void* cov;  // or null (all three of the kernel's T)
  int sx, sn, sc;
  CovSel csel;
  double o[3];
  int recentre;     // records = fl32(double(x) - o); 0: the plain cast
  float4* pts;      // null: a box pass
  float4* onrm;
  Cov8* ocov;
};

}  // namespace

// Strided float or double rows in device memory -> the 16 / 16 / 32-byte records (pts != null) and / or the bounding box of the finite
// input coordinates as a note (box != null).  T = float: box is the context's int accumulator and the note is box_reduce_publish's, as
// pack_cloud_kernel's; T = double: the 64-bit accumulator, six ordered words in payload words 1..6 — the box host_bbox computes.
template <typename T>
__global__ __launch_bounds__(kIoBlock) void pack_device_cloud_kernel(const PackArgs a, size_t n, void* __restrict__ box, unsigned long long* __restrict__ note_slot, unsigned long long seq) {
  __shared__ T sh[kIoTile];
  const size_t base = blockIdx.x * static_cast<size_t>(kIoBlock);
  const size_t i = base + threadIdx.x;
  const int sel3[3] = {0, 1, 2};
  T p[3] = {T(0), T(0), T(0)};
  if (a.xyz != nullptr) load_rows<T, 3>(static_cast<const T*>(a.xyz), base, n, a.sx, sel3, sh, p);  // (null: a pass over attributes of another dtype)
  if (a.xyz != nullptr && a.pts != nullptr && i < n) {
    float x, y, z;
    if (a.recentre) {
      x = static_cast<float>(static_cast<double>(p[0]) - a.o[0]);
      y = static_cast<float>(static_cast<double>(p[1]) - a.o[1]);
      z = static_cast<float>(static_cast<double>(p[2]) - a.o[2]);
    } else {
      x = static_cast<float>(p[0]), y = static_cast<float>(p[1]), z = static_cast<float>(p[2]);
    }
    a.pts[i] = make_float4(x, y, z, __uint_as_float(static_cast<uint32_t>(i)));
  }
  if (a.nrm != nullptr) {
    T q[3];
    load_rows<T, 3>(static_cast<const T*>(a.nrm), base, n, a.sn, sel3, sh, q);
    if (i < n) a.onrm[i] = make_float4(static_cast<float>(q[0]), static_cast<float>(q[1]), static_cast<float>(q[2]), 0.f);
  }
  if (a.cov != nullptr) {
    T m[6];
    load_rows<T, 6>(static_cast<const T*>(a.cov), base, n, a.sc, a.csel.s, sh, m);
    if (i < n) {
      Cov8 c;
      c.xx = static_cast<float>(m[0]);
      c.xy = static_cast<float>(m[1]);
      c.xz = static_cast<float>(m[2]);
      c.yy = static_cast<float>(m[3]);
      c.yz = static_cast<float>(m[4]);
      c.zz = static_cast<float>(m[5]);
      c.pad0 = c.pad1 = 0.f;
      a.ocov[i] = c;
    }
  }
  if (box == nullptr) return;  // (uniform)
  if constexpr (sizeof(T) == 4) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 3; k++)
        if (fabsf(p[k]) <= 3.4028234e38f) lo[k] = hi[k] = p[k];  // finite coordinates only (what the origin is chosen from)
    }
    box_reduce_publish(lo, hi, static_cast<int*>(box), note_slot, seq);
  } else {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (i < n) {
#pragma unroll
      for (int k = 0; k < 3; k++)
        if (p[k] - p[k] == 0.0) lo[k] = hi[k] = p[k];
    }
    box64_reduce_publish(lo, hi, static_cast<unsigned long long*>(box), note_slot, seq);
  }
}

namespace {
struct UnpackArgs {
  void* xyz;  // rows of sx elements, three written; or null
  void* nrm;
  void* cov;
  int sx, sn, sc, ccols;
  double o[3];
  int add_origin;
};
}  // namespace

// Records -> strided float or double rows in device memory, the points in the caller's frame: double(record) + origin, rounded to T
// (add_origin == 0: the records as they are — what sga_cloud_download gives for a cloud whose origin is zero).  Covariance rows are
// packed (6), 3x3 (9) or 4x4 with a zero fourth row and column (16).  Elements of a row beyond its columns are left untouched.
template <typename T>
__global__ __launch_bounds__(kIoBlock) void unpack_device_cloud_kernel(const float4* __restrict__ pts, const float4* __restrict__ nrm, const Cov8* __restrict__ cov, size_t n, const UnpackArgs a) {
  const size_t i = blockIdx.x * static_cast<size_t>(kIoBlock) + threadIdx.x;
  if (i >= n) return;
  if (a.xyz != nullptr) {
    const float4 p = pts[i];
    T* o = static_cast<T*>(a.xyz) + i * static_cast<size_t>(a.sx);
    if (a.add_origin) {
      o[0] = static_cast<T>(static_cast<double>(p.x) + a.o[0]);
      o[1] = static_cast<T>(static_cast<double>(p.y) + a.o[1]);
      o[2] = static_cast<T>(static_cast<double>(p.z) + a.o[2]);
    } else {
      o[0] = static_cast<T>(p.x), o[1] = static_cast<T>(p.y), o[2] = static_cast<T>(p.z);
    }
  }
  if (a.nrm != nullptr) {
    const float4 q = nrm[i];
    T* o = static_cast<T*>(a.nrm) + i * static_cast<size_t>(a.sn);
    o[0] = static_cast<T>(q.x), o[1] = static_cast<T>(q.y), o[2] = static_cast<T>(q.z);
  }
  if (a.cov != nullptr) {
    const Cov8 c = cov[i];
    T* o = static_cast<T*>(a.cov) + i * static_cast<size_t>(a.sc);
    const T xx = static_cast<T>(c.xx), xy = static_cast<T>(c.xy), xz = static_cast<T>(c.xz), yy = static_cast<T>(c.yy), yz = static_cast<T>(c.yz), zz = static_cast<T>(c.zz);
    if (a.ccols == 6) {
      o[0] = xx, o[1] = xy, o[2] = xz, o[3] = yy, o[4] = yz, o[5] = zz;
    } else if (a.ccols == 9) {
      o[0] = xx, o[1] = xy, o[2] = xz, o[3] = xy, o[4] = yy, o[5] = yz, o[6] = xz, o[7] = yz, o[8] = zz;
    } else {
      o[0] = xx, o[1] = xy, o[2] = xz, o[3] = T(0), o[4] = xy, o[5] = yy, o[6] = yz, o[7] = T(0), o[8] = xz, o[9] = yz, o[10] = zz, o[11] = T(0), o[12] = T(0), o[13] = T(0), o[14] = T(0), o[15] = T(0);
    }
  }
}

// kNN queries (strided float or double rows) -> m x 3 floats in the index's device frame: fl32(double(q) - origin)
template <typename T>
__global__ __launch_bounds__(kIoBlock) void knn_queries_kernel(const T* __restrict__ q, int stride, size_t m, double ox, double oy, double oz, float* __restrict__ out) {
  __shared__ T sh[kIoTile];
  const size_t base = blockIdx.x * static_cast<size_t>(kIoBlock);
  const size_t i = base + threadIdx.x;
  const int sel3[3] = {0, 1, 2};
  T p[3];
  load_rows<T, 3>(q, base, m, stride, sel3, sh, p);
  if (i >= m) return;
  out[3 * i] = static_cast<float>(static_cast<double>(p[0]) - ox);
  out[3 * i + 1] = static_cast<float>(static_cast<double>(p[1]) - oy);
  out[3 * i + 2] = static_cast<float>(static_cast<double>(p[2]) - oz);
}

// the results of a search in an empty index: no neighbour anywhere
__global__ __launch_bounds__(kIoBlock) void knn_fill_none_kernel(long long* __restrict__ idx, float* __restrict__ d2, size_t count) {
  const size_t i = blockIdx.x * static_cast<size_t>(kIoBlock) + threadIdx.x;
  if (i >= count) return;
  idx[i] = -1ll;
  d2[i] = INFINITY;
}

namespace {

size_t elem_size(int dtype) { return dtype == SGA_F64 ? 8 : 4; }

// dtype / cols / stride of one array (nothing is dereferenced but the struct itself)
int check_layout(const sga_device_array* a, const char* what, bool is_cov) {
  if (a->dtype != SGA_F32 && a->dtype != SGA_F64) return fail(SGA_ERR_INVALID, "%s: dtype %d is neither SGA_F32 nor SGA_F64", what, a->dtype);
  if (is_cov ? (a->cols != 6 && a->cols != 9 && a->cols != 16) : a->cols != 3) return fail(SGA_ERR_INVALID, "%s: cols = %d (%s)", what, a->cols, is_cov ? "covariances are 6, 9 or 16 per row" : "3 per row");
  if (a->stride < a->cols) return fail(SGA_ERR_INVALID, "%s: stride %d < cols %d", what, a->stride, a->cols);
  return SGA_OK;
}

// [p, p + bytes) must be device memory of the context's device, inside one allocation
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

// The caller's stream before, the context's stream behind: an event on user_stream the context's stream waits for ahead of the first
// kernel that touches caller memory (io_begin), an event behind the last such kernel that user_stream waits for (io_end).  No host wait.
struct IoOrder {
  hipStream_t user = nullptr;
  bool active = false;
};
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

// the 64-bit box accumulator, made on first use
int ensure_box64(sga_context* ctx) {
  if (ctx->d_box64.p != nullptr) return SGA_OK;
  SGA_TRY(ctx->d_box64.alloc(8));
  const unsigned long long init[8] = {box_enc64(INFINITY), box_enc64(INFINITY), box_enc64(INFINITY), box_enc64(-INFINITY), box_enc64(-INFINITY), box_enc64(-INFINITY), 0ull, 0ull};
  if (hipMemcpyAsync(ctx->d_box64.p, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    ctx->d_box64.release();
    return fail(SGA_ERR_HIP, "box accumulator init failed");
  }
  return SGA_OK;
}

template <typename T>
void launch_pack(sga_context* ctx, const PackArgs& a, size_t n, void* box, unsigned long long* slot, unsigned long long seq) {
  hipLaunchKernelGGL(pack_device_cloud_kernel<T>, dim3((n + kIoBlock - 1) / kIoBlock), dim3(kIoBlock), 0, ctx->stream, a, n, box, slot, seq);
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

int sga_cloud_create_device(sga_context* ctx, const sga_device_array* points, const sga_device_array* normals, const sga_device_array* covs, size_t n, const double origin[3], void* user_stream, int flags, sga_cloud** out) {
  if (out) *out = nullptr;
  if (n == 0) return SGA_OK;  // nothing to read: no cloud is made (an empty cloud comes from sga_cloud_create_f32 with n = 0)
  if (!ctx || !points || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "cloud too large (%zu points; limit 2^31-1)", n);
  if ((flags & SGA_IO_RELATIVE) && !origin) return fail(SGA_ERR_INVALID, "SGA_IO_RELATIVE needs an origin");
  SGA_TRY(check_layout(points, "points", false));
  if (normals) SGA_TRY(check_layout(normals, "normals", false));
  if (covs) SGA_TRY(check_layout(covs, "covs", true));
  const bool f64 = points->dtype == SGA_F64;
  const char* host_entry = f64 ? "sga_cloud_create_f64" : "sga_cloud_create_f32";
  SGA_TRY(check_array(ctx, points, n, "points", host_entry));
  if (normals) SGA_TRY(check_array(ctx, normals, n, "normals", host_entry));
  if (covs) SGA_TRY(check_array(ctx, covs, n, "covs", host_entry));
  SGA_ENTER(ctx);
  std::unique_ptr<sga_cloud> c(new sga_cloud);
  c->device = ctx->device;
  c->n = n;
  c->has_normals = normals != nullptr;
  c->has_covs = covs != nullptr;
  SGA_TRY(c->pts.alloc(n));
  if (normals) SGA_TRY(c->nrm.alloc(n));
  if (covs) SGA_TRY(c->cov.alloc(n));
  if (f64) SGA_TRY(ensure_box64(ctx));
  void* const box = f64 ? static_cast<void*>(ctx->d_box64.p) : static_cast<void*>(ctx->d_box.p);
  const bool relative = (flags & SGA_IO_RELATIVE) != 0;
  // `a`: the points with the attributes of their dtype; `other`: the attributes of the other dtype (a launch of their own, behind)
  PackArgs a{}, other{};
  a.xyz = points->data, a.sx = points->stride;
  a.csel = other.csel = cov_sel(covs ? covs->cols : 6);
  a.pts = other.pts = c->pts.p, a.onrm = other.onrm = c->nrm.p, a.ocov = other.ocov = c->cov.p;
  if (normals) {
    PackArgs& w = normals->dtype == points->dtype ? a : other;
    w.nrm = normals->data, w.sn = normals->stride;
  }
  if (covs) {
    PackArgs& w = covs->dtype == points->dtype ? a : other;
    w.cov = covs->data, w.sc = covs->stride;
  }
  IoOrder ord;
  SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  // The box of the finite input coordinates.  The origin is chosen from it (origin == NULL: the one host wait the data forces); a
  // blocking context, which waits anyway, also keeps it with the cloud, as the host entry points do.  A stream-ordered context with the
  // origin given waits for nothing and its cloud carries no box (an optimisation of the voxel grid's sort, never a result).
  const bool want_box = origin == nullptr || !ctx->stream_ordered;
  unsigned long long* slot = nullptr;
  unsigned long long seq = 0;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  auto read_box = [&]() -> int {
    unsigned long long payload[kNoteWords - 1];
    SGA_TRY(note_wait(ctx, seq, payload));
    if (f64) {
      for (int k = 0; k < 3; k++) lo[k] = box_dec64(payload[k]), hi[k] = box_dec64(payload[3 + k]);
    } else {
      float flo[3], fhi[3];
      box_note_decode(payload, flo, fhi);
      for (int k = 0; k < 3; k++) lo[k] = flo[k], hi[k] = fhi[k];
    }
    return SGA_OK;
  };
  if (want_box) seq = note_begin(ctx, &slot);
  if (origin != nullptr) {
    for (int k = 0; k < 3; k++) c->origin[k] = a.o[k] = origin[k];
    a.recentre = relative ? 0 : 1;
    if (f64)
      launch_pack<double>(ctx, a, n, want_box ? box : nullptr, slot, seq);
    else
      launch_pack<float>(ctx, a, n, want_box ? box : nullptr, slot, seq);
    SGA_HIP(hipGetLastError());
  } else if (f64) {
    // a box pass, then the pack pass: the subtraction is done in double before the rounding
    PackArgs b = a;
    b.pts = nullptr, b.nrm = b.cov = nullptr;
    launch_pack<double>(ctx, b, n, box, slot, seq);
    SGA_HIP(hipGetLastError());
    SGA_TRY(read_box());
    choose_origin(lo, hi, c->origin);
    for (int k = 0; k < 3; k++) a.o[k] = c->origin[k];
    a.recentre = 1;
    launch_pack<double>(ctx, a, n, nullptr, nullptr, 0ull);
    SGA_HIP(hipGetLastError());
  } else {
    // one pass; a second, points only, when the chosen origin is not zero (the host path's shape)
    launch_pack<float>(ctx, a, n, box, slot, seq);
    SGA_HIP(hipGetLastError());
    SGA_TRY(read_box());
    choose_origin(lo, hi, c->origin);
    if (!origin_is_zero(c->origin)) {
      PackArgs b = a;
      b.nrm = b.cov = nullptr;
      for (int k = 0; k < 3; k++) b.o[k] = c->origin[k];
      b.recentre = 1;
      launch_pack<float>(ctx, b, n, nullptr, nullptr, 0ull);
      SGA_HIP(hipGetLastError());
    }
  }
  if (other.nrm != nullptr || other.cov != nullptr) {
    if (f64)
      launch_pack<float>(ctx, other, n, nullptr, nullptr, 0ull);
    else
      launch_pack<double>(ctx, other, n, nullptr, nullptr, 0ull);
    SGA_HIP(hipGetLastError());
  }
  SGA_TRY(io_end(ctx, ord));
  if (want_box && origin != nullptr) SGA_TRY(read_box());  // (a blocking context: the stream has drained, the note is there)
  if (want_box && lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2]) {
    c->has_box = true;
    const bool outward = origin == nullptr && !f64;  // sga_cloud_create_f32 rounds the box of (input - origin) outwards; every other host path takes the box of the records
    for (int k = 0; k < 3; k++) {
      const double ok = relative ? 0.0 : c->origin[k];
      const float l = static_cast<float>(lo[k] - ok), h = static_cast<float>(hi[k] - ok);
      c->box_lo[k] = outward ? std::nextafterf(l, -INFINITY) : l;
      c->box_hi[k] = outward ? std::nextafterf(h, INFINITY) : h;
    }
  }
  SGA_TRY(mark_ready(ctx, c->ready));
  *out = c.release();
  return SGA_OK;
}

int sga_cloud_export_device(sga_context* ctx, const sga_cloud* cloud, const sga_device_array* points, const sga_device_array* normals, const sga_device_array* covs, void* user_stream, int flags) {
  if (!ctx || !cloud) return fail(SGA_ERR_INVALID, "null argument");
  if (points) SGA_TRY(check_layout(points, "points", false));
  if (normals) SGA_TRY(check_layout(normals, "normals", false));
  if (covs) SGA_TRY(check_layout(covs, "covs", true));
  if (normals && !cloud->has_normals) return fail(SGA_ERR_INVALID, "cloud has no normals");
  if (covs && !cloud->has_covs) return fail(SGA_ERR_INVALID, "cloud has no covariances");
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (n == 0 || (!points && !normals && !covs)) return SGA_OK;
  const sga_device_array* first = points ? points : normals ? normals : covs;
  if ((normals && normals->dtype != first->dtype) || (covs && covs->dtype != first->dtype)) return fail(SGA_ERR_INVALID, "points, normals and covs must share one dtype");
  if (points) SGA_TRY(check_array(ctx, points, n, "points", "sga_cloud_download"));
  if (normals) SGA_TRY(check_array(ctx, normals, n, "normals", "sga_cloud_download"));
  if (covs) SGA_TRY(check_array(ctx, covs, n, "covs", "sga_cloud_download"));
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, cloud->ready));
  IoOrder ord;
  SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  UnpackArgs a{};
  a.xyz = points ? const_cast<void*>(points->data) : nullptr, a.sx = points ? points->stride : 0;
  a.nrm = normals ? const_cast<void*>(normals->data) : nullptr, a.sn = normals ? normals->stride : 0;
  a.cov = covs ? const_cast<void*>(covs->data) : nullptr, a.sc = covs ? covs->stride : 0, a.ccols = covs ? covs->cols : 6;
  for (int k = 0; k < 3; k++) a.o[k] = cloud->origin[k];
  const dim3 grid((n + kIoBlock - 1) / kIoBlock), block(kIoBlock);
  if (first->dtype == SGA_F64) {
    a.add_origin = 1;  // sga_cloud_download_f64: always the sum in double
    hipLaunchKernelGGL(unpack_device_cloud_kernel<double>, grid, block, 0, ctx->stream, cloud->pts.p, cloud->nrm.p, cloud->cov.p, n, a);
  } else {
    a.add_origin = origin_is_zero(cloud->origin) ? 0 : 1;  // sga_cloud_download: the records as they are when the origin is zero
    hipLaunchKernelGGL(unpack_device_cloud_kernel<float>, grid, block, 0, ctx->stream, cloud->pts.p, cloud->nrm.p, cloud->cov.p, n, a);
  }
  SGA_HIP(hipGetLastError());
  return io_end(ctx, ord);
}

int sga_index_knn_device(sga_context* ctx, const sga_index* index, const sga_device_array* queries, size_t m, int k, double max_sq_dist, int64_t* d_idx, float* d_sq_dist, void* user_stream, int flags) {
  if (m == 0) return SGA_OK;
  if (!ctx || !index || !queries || !d_idx || !d_sq_dist) return fail(SGA_ERR_INVALID, "null argument");
  if (m >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many queries (%zu; limit 2^31-1)", m);
  if (k < 1 || k > 128) return fail(SGA_ERR_INVALID, "k must be in [1,128]");
  SGA_TRY(check_layout(queries, "queries", false));
  if (index->device != ctx->device) return fail(SGA_ERR_INVALID, "index lives on another device");
  if (index->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "sga_index_knn_device does not search projective indices (host queries: sga_index_knn)");
  SGA_TRY(index_knn_check_k(index, k));
  SGA_TRY(check_array(ctx, queries, m, "queries", queries->dtype == SGA_F64 ? "sga_index_knn_f64" : "sga_index_knn"));
  SGA_TRY(check_device_range(ctx, d_idx, m * static_cast<size_t>(k) * sizeof(int64_t), sizeof(int64_t), "d_idx", "sga_index_knn"));
  SGA_TRY(check_device_range(ctx, d_sq_dist, m * static_cast<size_t>(k) * sizeof(float), sizeof(float), "d_sq_dist", "sga_index_knn"));
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, index->ready));
  const bool empty = index->n == 0 || (index->kind != SGA_INDEX_KDTREE && index->hkeys.p == nullptr);
  DevBuf<float> d_q;
  if (!empty) SGA_TRY(d_q.alloc(m * 3));
  IoOrder ord;
  SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  if (empty) {
    const size_t count = m * static_cast<size_t>(k);
    hipLaunchKernelGGL(knn_fill_none_kernel, dim3((count + kIoBlock - 1) / kIoBlock), dim3(kIoBlock), 0, ctx->stream, reinterpret_cast<long long*>(d_idx), d_sq_dist, count);
    SGA_HIP(hipGetLastError());
  } else {
    const dim3 grid((m + kIoBlock - 1) / kIoBlock), block(kIoBlock);
    if (queries->dtype == SGA_F64)
      hipLaunchKernelGGL(knn_queries_kernel<double>, grid, block, 0, ctx->stream, static_cast<const double*>(queries->data), queries->stride, m, index->origin[0], index->origin[1], index->origin[2], d_q.p);
    else
      hipLaunchKernelGGL(knn_queries_kernel<float>, grid, block, 0, ctx->stream, static_cast<const float*>(queries->data), queries->stride, m, index->origin[0], index->origin[1], index->origin[2], d_q.p);
    SGA_HIP(hipGetLastError());
    SGA_TRY(index_knn_enqueue(ctx, index, d_q.p, m, k, max_sq_dist, reinterpret_cast<long long*>(d_idx), d_sq_dist));
  }
  return io_end(ctx, ord);
}

int sga_problem_get_factors_device(sga_context* ctx, const sga_problem* problem, int64_t* d_target_index, float* d_mahalanobis6, void* user_stream, int flags) {
  if (!ctx || !problem || (!d_target_index && !d_mahalanobis6)) return fail(SGA_ERR_INVALID, "null argument");
  if (problem->device != ctx->device) return fail(SGA_ERR_INVALID, "problem lives on another device");
  const size_t n = problem->n;
  if (n == 0) return SGA_OK;
  if (d_target_index) SGA_TRY(check_device_range(ctx, d_target_index, n * sizeof(int64_t), sizeof(int64_t), "d_target_index", "sga_problem_get_factors"));
  if (d_mahalanobis6) SGA_TRY(check_device_range(ctx, d_mahalanobis6, n * 6 * sizeof(float), sizeof(float), "d_mahalanobis6", "sga_problem_get_factors"));
  SGA_ENTER(ctx);
  IoOrder ord;
  SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  SGA_TRY(problem_factors_enqueue(ctx, problem, reinterpret_cast<long long*>(d_target_index), d_mahalanobis6));
  return io_end(ctx, ord);
}

}  // extern "C"

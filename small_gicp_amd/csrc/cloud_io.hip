// Clouds in and out: host arrays (pageable through the context's pinned staging ring, pinned ones read in place) and device arrays of the
// caller's become the 16 / 16 / 32-byte device records through ONE pack kernel, and leave through ONE unpack
// kernel.  Here too: the staging ring, the host box pass and sga_host_alloc / _free.
#include "cloud_box.hpp"
#include "device_io.hpp"
#include "notes.hpp"

#include <cmath>
#include <memory>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace sga {
namespace {

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

struct UnpackArgs {
  void* xyz;  // rows of sx elements, three written; or null
  void* nrm;
  void* cov;
  int sx, sn, sc, ccols;
  double o[3];
  int add_origin;
};

}  // namespace

// Strided float or double rows a kernel of this device can read — device memory, or pinned HOST memory (the staging ring, a caller's
// pinned buffer), of which load_rows reads every dword over PCIe exactly once — -> the 16 / 16 / 32-byte records (pts != null) and / or
// the bounding box of the finite INPUT coordinates as a note (box != null; notes.hpp): how an upload that no CPU pass has seen learns
// its origin.  T = float: box is the context's int accumulator and the note is box_reduce_publish's; T = double: the 64-bit accumulator,
// six ordered words in payload words 1..6 — the box host_bbox computes.
template <typename T>
__global__ __launch_bounds__(kIoBlock) void pack_cloud_kernel(const PackArgs a, size_t n, void* __restrict__ box, unsigned long long* __restrict__ note_slot, unsigned long long seq) {
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

// Records -> strided float or double rows in device memory, the points in the caller's frame: double(record) + origin, rounded to T
// (add_origin == 0: the records as they are — what sga_cloud_download gives for a cloud whose origin is zero).  Covariance rows are
// packed (6), 3x3 (9) or 4x4 with a zero fourth row and column (16).  Elements of a row beyond its columns are left untouched.
template <typename T>
__global__ __launch_bounds__(kIoBlock) void unpack_cloud_kernel(const float4* __restrict__ pts, const float4* __restrict__ nrm, const Cov8* __restrict__ cov, size_t n, const UnpackArgs a) {
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

const void* pinned_device_view(const void* p, size_t bytes, bool* on_device) {
  if (p == nullptr) return nullptr;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // an ordinary (pageable) pointer: not an error of ours
    return nullptr;
  }
  if (on_device != nullptr && a.type == hipMemoryTypeDevice) *on_device = true;
  if (a.type != hipMemoryTypeHost || a.devicePointer == nullptr) return nullptr;
  (void)bytes;
  return a.devicePointer;
}

namespace {

int launch_pack(sga_context* ctx, bool f64, const PackArgs& a, size_t n, void* box, unsigned long long* slot, unsigned long long seq) {
  const dim3 grid((n + kIoBlock - 1) / kIoBlock), block(kIoBlock);
  if (f64)
    hipLaunchKernelGGL(pack_cloud_kernel<double>, grid, block, 0, ctx->stream, a, n, box, slot, seq);
  else
    hipLaunchKernelGGL(pack_cloud_kernel<float>, grid, block, 0, ctx->stream, a, n, box, slot, seq);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}
int launch_unpack(sga_context* ctx, bool f64, const sga_cloud* cloud, const UnpackArgs& a) {
  const dim3 grid((cloud->n + kIoBlock - 1) / kIoBlock), block(kIoBlock);
  if (f64)
    hipLaunchKernelGGL(unpack_cloud_kernel<double>, grid, block, 0, ctx->stream, cloud->pts.p, cloud->nrm.p, cloud->cov.p, cloud->n, a);
  else
    hipLaunchKernelGGL(unpack_cloud_kernel<float>, grid, block, 0, ctx->stream, cloud->pts.p, cloud->nrm.p, cloud->cov.p, cloud->n, a);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// How a cloud learns its frame: the origin given (the records are relative to it, or become so: recentre) or chosen from the bounding box.
enum class UploadFrame { Given, GivenRecentre, FromBox };

// The records of cloud c from arrays a kernel can read where they are — device memory, or pinned host memory by its device address: the
// one sequence behind sga_cloud_create_device and the pinned uploads.  c->origin is the given origin, or receives the one chosen from the
// box.  want_box (FromBox needs it): lo / hi receive the box of the finite INPUT coordinates (left at lo > hi otherwise, and when no
// coordinate is finite); the kernel hands it over as a note (notes.hpp), so the host waits for that launch.  f64 needs ensure_box64.
// drain: the arrays may change once the call returns, so the stream is synchronised — unless a note has shown that the last launch is over.
int pack_from_view(sga_context* ctx, bool f64, PackArgs a, size_t n, UploadFrame frame, bool want_box, bool drain, sga_cloud* c, double lo[3], double hi[3]) {
  for (int k = 0; k < 3; k++) lo[k] = INFINITY, hi[k] = -INFINITY;
  void* const box = !want_box ? nullptr : f64 ? static_cast<void*>(ctx->d_box64.p) : static_cast<void*>(ctx->d_box.p);
  unsigned long long* slot = nullptr;
  const unsigned long long seq = want_box ? note_begin(ctx, &slot) : 0ull;
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
  bool in_flight = true;  // the last launch: nobody has waited for it
  if (frame != UploadFrame::FromBox) {
    for (int k = 0; k < 3; k++) a.o[k] = c->origin[k];
    a.recentre = frame == UploadFrame::GivenRecentre ? 1 : 0;
    SGA_TRY(launch_pack(ctx, f64, a, n, box, slot, seq));
    if (want_box) {
      SGA_TRY(read_box());
      in_flight = false;
    }
  } else {
    // float: one pass, and a second, points only, when the chosen origin is not zero (far from the origin: rare).  double: a box pass,
    // then the pack pass — the subtraction is done in double before the rounding
    PackArgs first = a;
    if (f64) first.pts = nullptr, first.nrm = first.cov = nullptr;
    SGA_TRY(launch_pack(ctx, f64, first, n, box, slot, seq));
    SGA_TRY(read_box());
    in_flight = false;
    choose_origin(lo, hi, c->origin);
    if (f64 || !origin_is_zero(c->origin)) {
      if (!f64) a.nrm = a.cov = nullptr;
      for (int k = 0; k < 3; k++) a.o[k] = c->origin[k];
      a.recentre = 1;
      SGA_TRY(launch_pack(ctx, f64, a, n, nullptr, nullptr, 0ull));
      in_flight = true;
    }
  }
  if (drain && in_flight) SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

// ---- uploads ------------------------------------------------------------------------------------------------------------------
// A slot of the context's pinned staging ring with room for `bytes` (grow-only).  A slot handed out before is reused only after the
// event recorded behind its reader (stage_release) has completed.
int stage_acquire(sga_context* ctx, size_t bytes, sga_context::StageSlot** out) {
  sga_context::StageSlot& slot = ctx->stage[ctx->stage_next++ % sga_context::kStageSlots];
  if (slot.busy) {
    SGA_HIP(hipEventSynchronize(slot.done));
    slot.busy = false;
  }
  if (slot.bytes < bytes) {
    if (slot.host) (void)hipHostFree(slot.host);
    slot.host = slot.dev = nullptr;
    slot.bytes = 0;
    size_t want = 1u << 20;
    while (want < bytes) want <<= 1;
    if (hipHostMalloc(&slot.host, want, hipHostMallocMapped) != hipSuccess) return fail(SGA_ERR_HIP, "hipHostMalloc(%zu bytes) failed", want);
    if (hipHostGetDevicePointer(&slot.dev, slot.host, 0) != hipSuccess) return fail(SGA_ERR_HIP, "hipHostGetDevicePointer failed");
    slot.bytes = want;
  }
  *out = &slot;
  return SGA_OK;
}
// behind the launch that reads the slot
int stage_release(sga_context* ctx, sga_context::StageSlot* slot) {
  if (!slot->done) SGA_HIP(hipEventCreateWithFlags(&slot->done, hipEventDisableTiming));
  SGA_HIP(hipEventRecord(slot->done, ctx->stream));
  slot->busy = true;
  return SGA_OK;
}

// One pass over a pageable xyz array: copy it into the staging slot AND take the bounding box of its finite coordinates (the origin of
// the device frame is chosen from it).  Twelve running minima / maxima (four points) so that the compiler keeps them in vector registers;
// a 115k-point scan (1.4 MB) went through a scalar box pass and a memcpy before: two passes, ~0.25 ms.
#if defined(__x86_64__)
// 24 floats (8 points) per step: three 8-wide vectors whose lanes keep their coordinate (24 is a multiple of 3)
__attribute__((target("avx2"))) static void copy_with_box_wide(const float* __restrict__ src, float* __restrict__ dst, size_t count /* floats, a multiple of 24 */, float lo24[24], float hi24[24]) {
  const __m256 absmask = _mm256_castsi256_ps(_mm256_set1_epi32(0x7fffffff)), fmax = _mm256_set1_ps(3.4028234e38f);
  __m256 lo0 = _mm256_loadu_ps(lo24), lo1 = _mm256_loadu_ps(lo24 + 8), lo2 = _mm256_loadu_ps(lo24 + 16);
  __m256 hi0 = _mm256_loadu_ps(hi24), hi1 = _mm256_loadu_ps(hi24 + 8), hi2 = _mm256_loadu_ps(hi24 + 16);
  for (size_t i = 0; i < count; i += 24) {
    const __m256 a = _mm256_loadu_ps(src + i), b = _mm256_loadu_ps(src + i + 8), c = _mm256_loadu_ps(src + i + 16);
    _mm256_storeu_ps(dst + i, a);
    _mm256_storeu_ps(dst + i + 8, b);
    _mm256_storeu_ps(dst + i + 16, c);
    // non-finite values (NaN compares false, inf fails <= FLT_MAX) are replaced by the running bound: they change nothing
    const __m256 ma = _mm256_cmp_ps(_mm256_and_ps(a, absmask), fmax, _CMP_LE_OQ), mb = _mm256_cmp_ps(_mm256_and_ps(b, absmask), fmax, _CMP_LE_OQ), mc = _mm256_cmp_ps(_mm256_and_ps(c, absmask), fmax, _CMP_LE_OQ);
    lo0 = _mm256_min_ps(_mm256_blendv_ps(lo0, a, ma), lo0);
    lo1 = _mm256_min_ps(_mm256_blendv_ps(lo1, b, mb), lo1);
    lo2 = _mm256_min_ps(_mm256_blendv_ps(lo2, c, mc), lo2);
    hi0 = _mm256_max_ps(_mm256_blendv_ps(hi0, a, ma), hi0);
    hi1 = _mm256_max_ps(_mm256_blendv_ps(hi1, b, mb), hi1);
    hi2 = _mm256_max_ps(_mm256_blendv_ps(hi2, c, mc), hi2);
  }
  _mm256_storeu_ps(lo24, lo0), _mm256_storeu_ps(lo24 + 8, lo1), _mm256_storeu_ps(lo24 + 16, lo2);
  _mm256_storeu_ps(hi24, hi0), _mm256_storeu_ps(hi24 + 8, hi1), _mm256_storeu_ps(hi24 + 16, hi2);
}
#endif
static void copy_with_box_plain(const float* __restrict__ src, float* __restrict__ dst, size_t first, size_t count, float lo24[24], float hi24[24]) {
  for (size_t f = first; f < count; f++) {
    const float v = src[f];
    dst[f] = v;
    const int j = static_cast<int>(f % 24);  // 24 is a multiple of 3: lane j keeps coordinate j % 3
    if (__builtin_fabsf(v) <= 3.4028234e38f) {
      lo24[j] = v < lo24[j] ? v : lo24[j];
      hi24[j] = v > hi24[j] ? v : hi24[j];
    }
  }
}
static void copy_with_box(const float* src, float* dst, size_t n, double lo[3], double hi[3]) {
  float lo24[24], hi24[24];
  for (int j = 0; j < 24; j++) lo24[j] = INFINITY, hi24[j] = -INFINITY;
  const size_t count = n * 3;
  size_t body = 0;
#if defined(__x86_64__)
  static const bool avx2 = __builtin_cpu_supports("avx2");
  if (avx2) {
    body = count / 24 * 24;
    copy_with_box_wide(src, dst, body, lo24, hi24);
  }
#endif
  copy_with_box_plain(src, dst, body, count, lo24, hi24);
  for (int k = 0; k < 3; k++) {
    lo[k] = INFINITY, hi[k] = -INFINITY;
    for (int j = k; j < 24; j += 3) {
      lo[k] = lo24[j] < lo[k] ? lo24[j] : lo[k];
      hi[k] = hi24[j] > hi[k] ? hi24[j] : hi[k];
    }
  }
}

// the host arrays of an upload (xyz 3 floats per point, normals 3, covariances 6) and the records of c they become
static PackArgs host_pack_args(const float* xyz, const float* normals, const float* cov6, sga_cloud* c) {
  PackArgs a{};
  a.xyz = xyz, a.nrm = normals, a.cov = cov6;
  a.sx = a.sn = 3, a.sc = 6;
  a.csel = cov_sel(6);
  a.pts = c->pts.p, a.onrm = c->nrm.p, a.ocov = c->cov.p;
  return a;
}

// The cloud of n points from host arrays: xyz (3 floats per point), optional normals (3) and covariances (6).
//   * pageable arrays are copied once into a slot of the context's pinned staging ring (the box is taken in the same pass) and the pack
//     kernel reads the slot over PCIe; in stream-ordered mode the call returns with the kernel in flight (the slot is reused only after
//     the event recorded behind it) — the caller's arrays are free as soon as the call returns either way;
//   * arrays that already live in pinned host memory (sga_host_alloc, hipHostMalloc) are read by the pack kernel where they are: no CPU
//     pass at all; the box comes back from the kernel as a note (notes.hpp), so the kernel has finished reading when the call returns.
static int cloud_upload(sga_context* ctx, const float* xyz, const float* normals, const float* cov6, size_t n, UploadFrame frame, const double origin_in[3], sga_cloud** out) {
  if (!ctx || !out || (n > 0 && !xyz)) return fail(SGA_ERR_INVALID, "null argument");
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "cloud too large (%zu points; limit 2^31-1)", n);
  *out = nullptr;
  SGA_ENTER(ctx);
  std::unique_ptr<sga_cloud> c;
  SGA_TRY(cloud_make(ctx, frame != UploadFrame::FromBox ? origin_in : nullptr, n, normals != nullptr, cov6 != nullptr, &c));
  if (n == 0) {
    *out = c.release();
    return SGA_OK;
  }
  const size_t fx = n * 3, fn = normals ? n * 3 : 0, fc = cov6 ? n * 6 : 0;
  static const bool zero_copy = !(getenv("SGA_UPLOAD_PINNED") && atoi(getenv("SGA_UPLOAD_PINNED")) == 0);
  bool on_device = false;
  const float* view = static_cast<const float*>(pinned_device_view(xyz, fx * sizeof(float), &on_device));
  if (on_device) return fail(SGA_ERR_INVALID, "xyz is device memory: clouds that live on the device are made by sga_cloud_create_device");
  const float* dx = zero_copy ? view : nullptr;
  const float* dn = (dx && normals) ? static_cast<const float*>(pinned_device_view(normals, fn * sizeof(float))) : nullptr;
  const float* dc = (dx && cov6) ? static_cast<const float*>(pinned_device_view(cov6, fc * sizeof(float))) : nullptr;
  double lo[3], hi[3];
  if (dx && (!normals || dn) && (!cov6 || dc)) {
    // ---- the caller's arrays are pinned: the kernel reads them in place (a given origin: no box; drained: the caller's buffer is being read)
    SGA_TRY(pack_from_view(ctx, false, host_pack_args(dx, dn, dc, c.get()), n, frame, frame == UploadFrame::FromBox, true, c.get(), lo, hi));
  } else {
    // ---- pageable arrays: one CPU pass into the staging ring
    sga_context::StageSlot* slot = nullptr;
    SGA_TRY(stage_acquire(ctx, (fx + fn + fc) * sizeof(float), &slot));
    float* stage = static_cast<float*>(slot->host);
    const float* dstage = static_cast<const float*>(slot->dev);
    copy_with_box(xyz, stage, n, lo, hi);
    if (normals) std::memcpy(stage + fx, normals, fn * sizeof(float));
    if (cov6) std::memcpy(stage + fx + fn, cov6, fc * sizeof(float));
    if (frame == UploadFrame::FromBox) choose_origin(lo, hi, c->origin);
    PackArgs a = host_pack_args(dstage, normals ? dstage + fx : nullptr, cov6 ? dstage + fx + fn : nullptr, c.get());
    for (int k = 0; k < 3; k++) a.o[k] = c->origin[k];
    a.recentre = (frame == UploadFrame::GivenRecentre || (frame == UploadFrame::FromBox && !origin_is_zero(c->origin))) ? 1 : 0;
    SGA_TRY(launch_pack(ctx, false, a, n, nullptr, nullptr, 0ull));
    if (ctx->stream_ordered) {
      SGA_TRY(stage_release(ctx, slot));
    } else {
      SGA_HIP(hipStreamSynchronize(ctx->stream));
    }
  }
  // relative to a given origin the box of the inputs IS the box of the records; otherwise (box - origin), rounded outwards
  cloud_set_box(c.get(), lo, hi, frame == UploadFrame::Given, frame != UploadFrame::Given);
  SGA_TRY(mark_ready(ctx, c->ready));
  *out = c.release();
  return SGA_OK;
}

// bounding box over the finite coordinates of n points with `stride` values per point
template <typename S>
static void host_bbox(const S* xyz, size_t n, size_t stride, double lo[3], double hi[3]) {
  for (int k = 0; k < 3; k++) lo[k] = INFINITY, hi[k] = -INFINITY;
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) {
      const double v = static_cast<double>(xyz[stride * i + k]);
      if (v - v == 0.0) {  // finite
        lo[k] = v < lo[k] ? v : lo[k];
        hi[k] = v > hi[k] ? v : hi[k];
      }
    }
}

namespace sga {
// absolute fp32 coordinates, recentred about a GIVEN origin (multi.hip: the shards of one source share a device frame)
int cloud_create_f32_about(sga_context* ctx, const float* xyz, const float* normals, const float* cov6, size_t n, const double origin[3], sga_cloud** out) {
  return cloud_upload(ctx, xyz, normals, cov6, n, origin_is_zero(origin) ? UploadFrame::Given : UploadFrame::GivenRecentre, origin, out);
}
void host_bbox_f32(const float* xyz, size_t n, double lo[3], double hi[3]) { host_bbox(xyz, n, 3, lo, hi); }
void host_bbox_f64(const double* xyzw, size_t n, double lo[3], double hi[3]) { host_bbox(xyzw, n, 4, lo, hi); }
}  // namespace sga
extern "C" {

int sga_cloud_create_f32_origin(sga_context* ctx, const float* xyz_rel, const float* normals, const float* cov6, size_t n, const double origin[3], sga_cloud** out) {
  return cloud_upload(ctx, xyz_rel, normals, cov6, n, UploadFrame::Given, origin, out);  // relative to `origin` (null: zero): the records go to the device as they are
}

int sga_cloud_create_f32(sga_context* ctx, const float* xyz, const float* normals, const float* cov6, size_t n, sga_cloud** out) {
  return cloud_upload(ctx, xyz, normals, cov6, n, UploadFrame::FromBox, nullptr, out);  // the origin: chosen from the box the upload takes in passing
}

// Pinned host memory for the caller's scans: sga_cloud_create_f32 reads arrays that live in it in place (no staging copy on the CPU).
int sga_host_alloc(size_t bytes, void** out) {
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  *out = nullptr;
  if (bytes == 0) return SGA_OK;
  if (hipHostMalloc(out, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return fail(SGA_ERR_HIP, "hipHostMalloc(%zu bytes) failed", bytes);
  }
  return SGA_OK;
}
int sga_host_free(void* p) {
  if (p && hipHostFree(p) != hipSuccess) {
    (void)hipGetLastError();
    return fail(SGA_ERR_HIP, "hipHostFree failed");
  }
  return SGA_OK;
}

int sga_cloud_create_f64_origin(sga_context* ctx, const double* xyzw, const double* normals4, const double* cov4x4, size_t n, const double origin_in[3], sga_cloud** out) {
  if (!ctx || !out || (n > 0 && !xyzw)) return fail(SGA_ERR_INVALID, "null argument");
  double origin[3] = {0, 0, 0};
  if (origin_in) {
    for (int k = 0; k < 3; k++) origin[k] = origin_in[k];
  } else {
    double lo[3], hi[3];
    host_bbox(xyzw, n, 4, lo, hi);
    choose_origin(lo, hi, origin);
  }
  std::vector<float> xyz(n * 3), nrm, cov;
  for (size_t i = 0; i < n; i++)
    for (int k = 0; k < 3; k++) xyz[3 * i + k] = static_cast<float>(xyzw[4 * i + k] - origin[k]);  // in double, then rounded: what fp32 can hold of the cloud is its shape, not its place
  if (normals4) {
    nrm.resize(n * 3);
    for (size_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) nrm[3 * i + k] = static_cast<float>(normals4[4 * i + k]);
  }
  if (cov4x4) {
    cov.resize(n * 6);
    const CovSel sel = cov_sel(16);  // (symmetric: storage order irrelevant)
    for (size_t i = 0; i < n; i++)
      for (int k = 0; k < 6; k++) cov[6 * i + k] = static_cast<float>(cov4x4[16 * i + sel.s[k]]);
  }
  return cloud_upload(ctx, xyz.data(), normals4 ? nrm.data() : nullptr, cov4x4 ? cov.data() : nullptr, n, UploadFrame::Given, origin, out);
}

int sga_cloud_create_f64(sga_context* ctx, const double* xyzw, const double* normals4, const double* cov4x4, size_t n, sga_cloud** out) {
  return sga_cloud_create_f64_origin(ctx, xyzw, normals4, cov4x4, n, nullptr, out);
}

// Clouds from, and into, device memory of the caller's (device_io.hpp: the pointer checks and the two events that
// order the caller's stream against the context's).
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
  std::unique_ptr<sga_cloud> c;  // (origin == NULL: chosen from the box below)
  SGA_TRY(cloud_make(ctx, origin, n, normals != nullptr, covs != nullptr, &c));
  if (f64) SGA_TRY(ensure_box64(ctx));
  const bool relative = (flags & SGA_IO_RELATIVE) != 0;
  // `a`: the points with the attributes of their dtype; `other`: the attributes of the other dtype (a launch of their own)
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
  if (other.nrm != nullptr || other.cov != nullptr) SGA_TRY(launch_pack(ctx, !f64, other, n, nullptr, nullptr, 0ull));
  // The box of the finite input coordinates.  The origin is chosen from it (origin == NULL: the one host wait the data forces); a
  // blocking context, which waits anyway, also keeps it with the cloud, as the host entry points do.  A stream-ordered context with the
  // origin given waits for nothing and its cloud carries no box (an optimisation of the voxel grid's sort, never a result).
  const bool want_box = origin == nullptr || !ctx->stream_ordered;
  const UploadFrame frame = origin == nullptr ? UploadFrame::FromBox : relative ? UploadFrame::Given : UploadFrame::GivenRecentre;
  double lo[3], hi[3];
  SGA_TRY(pack_from_view(ctx, f64, a, n, frame, want_box, false, c.get(), lo, hi));
  SGA_TRY(io_end(ctx, ord));
  // sga_cloud_create_f32 rounds the box of (input - origin) outwards; every other host path this one mirrors takes the box of the records
  cloud_set_box(c.get(), lo, hi, relative, origin == nullptr && !f64);
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
  const bool f64 = first->dtype == SGA_F64;
  // double rows: always the sum in double (sga_cloud_download_f64); float rows: the records as they are when the origin is zero (sga_cloud_download)
  a.add_origin = (f64 || !origin_is_zero(cloud->origin)) ? 1 : 0;
  SGA_TRY(launch_unpack(ctx, f64, cloud, a));
  return io_end(ctx, ord);
}

// fp32 rows leave the device in the caller's frame (the kernel adds the origin in double); the f64 download moves the same 12 bytes per
// point over the link — the records — and widens them, and adds the origin, here
static int cloud_download_impl(sga_context* ctx, const sga_cloud* cloud, float* xyz, double* xyz64, float* normals, float* cov6) {
  if (!ctx || !cloud) return fail(SGA_ERR_INVALID, "null argument");
  if (normals && !cloud->has_normals) return fail(SGA_ERR_INVALID, "cloud has no normals");
  if (cov6 && !cloud->has_covs) return fail(SGA_ERR_INVALID, "cloud has no covariances");
  const size_t n = cloud->n;
  if (n == 0) return SGA_OK;
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, cloud->ready));
  DevBuf<float> sx, sn, sc;
  std::vector<float> rel;
  float* xyz_dst = xyz;
  if (xyz64) {
    rel.resize(n * 3);
    xyz_dst = rel.data();
  }
  if (xyz_dst) SGA_TRY(sx.alloc(n * 3));
  if (normals) SGA_TRY(sn.alloc(n * 3));
  if (cov6) SGA_TRY(sc.alloc(n * 6));
  UnpackArgs a{};
  a.xyz = sx.p, a.nrm = sn.p, a.cov = sc.p;
  a.sx = a.sn = 3, a.sc = a.ccols = 6;
  for (int k = 0; k < 3; k++) a.o[k] = cloud->origin[k];
  a.add_origin = (xyz && !origin_is_zero(cloud->origin)) ? 1 : 0;
  SGA_TRY(launch_unpack(ctx, false, cloud, a));
  if (xyz_dst) SGA_HIP(hipMemcpyAsync(xyz_dst, sx.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (normals) SGA_HIP(hipMemcpyAsync(normals, sn.p, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  if (cov6) SGA_HIP(hipMemcpyAsync(cov6, sc.p, n * 6 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t i = 0; i < rel.size(); i++) xyz64[i] = static_cast<double>(rel[i]) + cloud->origin[i % 3];
  return SGA_OK;
}

int sga_cloud_download(sga_context* ctx, const sga_cloud* cloud, float* xyz, float* normals, float* cov6) { return cloud_download_impl(ctx, cloud, xyz, nullptr, normals, cov6); }

int sga_cloud_download_f64(sga_context* ctx, const sga_cloud* cloud, double* xyz, float* normals, float* cov6) { return cloud_download_impl(ctx, cloud, nullptr, xyz, normals, cov6); }

}  // extern "C"

// Clouds: every sga_cloud_* entry point.  Host arrays (pageable through the context's pinned staging ring, pinned ones read in place)
// and device arrays of the caller's become the 16 / 16 / 32-byte device records through ONE pack kernel, and
// leave through ONE unpack kernel; slices, downloads and the small getters; posed clouds joined into one; sweeps
// deskewed with a pose per point.  (Crop and gather: cloud_crop.hip; the box helpers both share: cloud_box.hpp.)
#include "cloud_box.hpp"
#include "device_io.hpp"
#include "forest.hpp"
#include "lie.hpp"
#include "voxel_steps.hpp"
#include "notes.hpp"

#include <cmath>
#include <memory>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace sga {
namespace {

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

__global__ void slice_cloud_kernel(const float4* __restrict__ pts, const float4* __restrict__ nrm, const Cov8* __restrict__ cov, size_t first, size_t count, float4* __restrict__ opts, float4* __restrict__ onrm, Cov8* __restrict__ ocov) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= count) return;
  float4 p = pts[first + i];
  p.w = __uint_as_float(static_cast<uint32_t>(i));  // indices of the slice start at 0
  opts[i] = p;
  if (nrm) onrm[i] = nrm[first + i];
  if (cov) ocov[i] = cov[first + i];
}

// What a pose does to one record, stated once for merge_cloud_kernel and deskew_cloud_kernel: the point R r + t (posed_point,
// voxel_steps.hpp), the normal R n and the covariance R C R^T are evaluated in double from the fp32 records, with the insert kernels'
// expressions (voxelmap.hip: fvm_update_kernel, ivm_update_kernel), and rounded once.
__device__ __forceinline__ float4 posed_normal_record(const Pose12& T, const float4 q) {
  double N[3];
#pragma unroll
  for (int a = 0; a < 3; a++) N[a] = T.r[3 * a] * q.x + T.r[3 * a + 1] * q.y + T.r[3 * a + 2] * q.z;
  return make_float4(static_cast<float>(N[0]), static_cast<float>(N[1]), static_cast<float>(N[2]), 0.f);
}
__device__ __forceinline__ void posed_cov_record(const Pose12& T, const Cov8* __restrict__ in, Cov8* __restrict__ out) {
  const float4* cin = reinterpret_cast<const float4*>(in);
  const float4 c0 = cin[0], c1 = cin[1];  // xx xy xz yy | yz zz 0 0
  const double Cm[3][3] = {{c0.x, c0.y, c0.z}, {c0.y, c0.w, c1.x}, {c0.z, c1.x, c1.y}};
  double RC[3][3], C6[6];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) RC[a][b] = T.r[3 * a] * Cm[0][b] + T.r[3 * a + 1] * Cm[1][b] + T.r[3 * a + 2] * Cm[2][b];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = a; b < 3; b++) C6[k++] = RC[a][0] * T.r[3 * b] + RC[a][1] * T.r[3 * b + 1] + RC[a][2] * T.r[3 * b + 2];
  float4* cout = reinterpret_cast<float4*>(out);
  cout[0] = make_float4(static_cast<float>(C6[0]), static_cast<float>(C6[1]), static_cast<float>(C6[2]), static_cast<float>(C6[3]));
  cout[1] = make_float4(static_cast<float>(C6[4]), static_cast<float>(C6[5]), 0.f, 0.f);
}

// One member of a merge (read with scalar loads): its records, its pose with the offset between the two device
// frames folded in — t = (R o_m + t_m) - o, formed on the host in double — and its stretch of the output.
struct MergeMember {
  const float4* pts;
  const float4* nrm;  // read only when the output keeps the attribute
  const Cov8* cov;
  Pose12 T;
  uint32_t n, off;
};
static_assert(sizeof(MergeMember) % 8 == 0, "the table is copied in 8-byte words");

// Posed clouds -> one cloud: workgroup b moves 256 points of the member m with prefix[m] <= b < prefix[m + 1] to their place in the
// concatenation, each record posed by the member's pose (above); w is the point's index in the output.  box != null: the
// bounding box of the posed points that are finite, taken BEFORE the rounding (which is monotone: the rounded box bounds the records
// exactly), leaves as a note in payload words 1..6 (box64_reduce_publish).
__global__ __launch_bounds__(kIoBlock) void merge_cloud_kernel(const MergeMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, float4* __restrict__ opts, float4* __restrict__ onrm, Cov8* __restrict__ ocov,
                                                               unsigned long long* __restrict__ box, unsigned long long* __restrict__ note_slot, unsigned long long seq) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const MergeMember& g = *uniform_const(members + m);
  const uint32_t i = (blockIdx.x - prefix[m]) * static_cast<uint32_t>(kIoBlock) + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < g.n) {
    const Pose12& T = g.T;
    const uint32_t j = g.off + i;
    double x, y, z;
    posed_point(T, g.pts[i], x, y, z);
    opts[j] = make_float4(static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), __uint_as_float(j));
    if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0) lo[0] = hi[0] = x, lo[1] = hi[1] = y, lo[2] = hi[2] = z;  // a non-finite point stays out of the box
    if (onrm != nullptr) onrm[j] = posed_normal_record(T, g.nrm[i]);
    if (ocov != nullptr) posed_cov_record(T, g.cov + i, ocov + j);
  }
  if (box == nullptr) return;  // (uniform)
  box64_reduce_publish(lo, hi, box, note_slot, seq);
}

// One member of a deskew (read with scalar loads): its records and where they go, its times, what its twist
// and its origin contribute to every point's pose (lie.hpp), and where its box is reduced and handed over.
struct DeskewMember {
  const float4* pts;
  const float4* nrm;  // or null
  const Cov8* cov;
  float4* opts;
  float4* onrm;
  Cov8* ocov;
  const void* times;         // float or double (tf64), tstride elements apart: device memory, or pinned host memory by its device address
  unsigned long long* acc;   // {min x y z, max x y z (encoded), arrival counter, 0} in the call's table, identity values and 0 at the start; null: no box
  unsigned long long* slot;  // six words of the context's box block (pinned, device-mapped)
  double ref_time;
  TwistConst c;
  uint32_t n, blocks;
  int tstride, tf64;
};
static_assert(sizeof(DeskewMember) % 8 == 0, "the table is copied in 8-byte words");

// Sweeps -> sweeps as seen from the sensor frame at ref_time: workgroup b takes 256 points of the member m with prefix[m] <= b <
// prefix[m + 1]; point i gets the pose exp((s_i - ref_time) xi) — in double, from the member's constants, with no cancellation for any
// angle (lie.hpp) — and is posed as a member of a merge is.  w is the index.  A non-finite time makes every entry of the pose a NaN.
// g.acc != null: the box of the member's finite unrounded points is joined in its accumulator; the member's last workgroup writes it into
// the member's words of the box block, and the last member to arrive publishes the call's sequence number (forest_box_arrive).
__global__ __launch_bounds__(kIoBlock) void deskew_cloud_kernel(const DeskewMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, const ForestBoxes hand) {
  __shared__ bool sh_last;
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const DeskewMember& g = *uniform_const(members + m);
  const uint32_t i = (blockIdx.x - prefix[m]) * static_cast<uint32_t>(kIoBlock) + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < g.n) {
    const size_t ti = static_cast<size_t>(i) * static_cast<size_t>(g.tstride);
    const double s = g.tf64 ? static_cast<const double*>(g.times)[ti] : static_cast<double>(static_cast<const float*>(g.times)[ti]);
    Pose12 T;
    twist_pose(g.c, s - g.ref_time, T.r, T.t);
    double x, y, z;
    posed_point(T, g.pts[i], x, y, z);
    g.opts[i] = make_float4(static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), __uint_as_float(i));
    if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0) lo[0] = hi[0] = x, lo[1] = hi[1] = y, lo[2] = hi[2] = z;  // a non-finite point stays out of the box
    if (g.onrm != nullptr) g.onrm[i] = posed_normal_record(T, g.nrm[i]);
    if (g.ocov != nullptr) posed_cov_record(T, g.cov + i, g.ocov + i);
  }
  if (g.acc == nullptr) return;  // (uniform: a call has boxes for all members or for none)
  box64_reduce_block(lo, hi, g.acc);
  if (threadIdx.x == 0) sh_last = __hip_atomic_fetch_add(&g.acc[6], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == g.blocks - 1u;
  __syncthreads();
  if (!sh_last) return;  // workgroup-uniform
  if (threadIdx.x < 6) g.slot[threadIdx.x] = __hip_atomic_load(&g.acc[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) forest_box_arrive(hand);
}

namespace {

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

// The box of the records (device frame) from the box of the inputs, when there is one (lo <= hi): fp32 of (box - origin) — relative:
// the inputs ARE the records — rounded outwards on request.
void cloud_set_box(sga_cloud* c, const double lo[3], const double hi[3], bool relative, bool outward) {
  if (!(lo[0] <= hi[0] && lo[1] <= hi[1] && lo[2] <= hi[2])) return;
  c->has_box = true;
  for (int k = 0; k < 3; k++) {
    const double ok = relative ? 0.0 : c->origin[k];
    const float l = static_cast<float>(lo[k] - ok), h = static_cast<float>(hi[k] - ok);
    c->box_lo[k] = outward ? std::nextafterf(l, -INFINITY) : l;
    c->box_hi[k] = outward ? std::nextafterf(h, INFINITY) : h;
  }
}

namespace {

// ---- sga_cloud_merge -----------------------------------------------------------------------------------------
constexpr size_t kMergeMaxMembers = 1u << 15;

// Member m's pose for an output frame at `o`: R as given (column-major T16, null: the identity), t = c - o with c = R o_m + t_m the
// member's origin in the caller's frame.  Every product and sum is rounded on its own, in the order written (no contraction): the
// offset is a function of the inputs alone, and c - o — the form of pose_to_device — is formed ONCE here, so a merge far from the origin
// cancels nothing on the device.
Pose12 merge_pose(const double* T16, const double o_m[3], const double o[3]) {
#pragma clang fp contract(off)
  Pose12 T;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T.r[3 * r + c] = T16 ? T16[4 * c + r] : (r == c ? 1.0 : 0.0);
    const double t = T16 ? T16[12 + r] : 0.0;
    const double c = ((T.r[3 * r] * o_m[0] + T.r[3 * r + 1] * o_m[1]) + T.r[3 * r + 2] * o_m[2]) + t;
    T.t[r] = c - o[r];
  }
  return T;
}

// One pass over the non-empty members `live`: the table ([members][prefix of the grid: live + 1]) and ONE launch over the concatenation.  want_box: the box of the finite posed points, relative to o,
// arrives as a note the call waits for (lo > hi: no finite point).
int merge_pass(sga_context* ctx, const sga_cloud* const* clouds, const double* T, const std::vector<size_t>& live, const double o[3], sga_cloud* c, bool want_box, DevBuf<unsigned long long>& table, double lo[3], double hi[3]) {
  const size_t count = live.size();
  std::vector<MergeMember> members(count);
  std::vector<uint32_t> prefix(count + 1, 0u);
  uint32_t off = 0;
  for (size_t j = 0; j < count; j++) {
    const size_t k = live[j];
    MergeMember& g = members[j];
    std::memset(&g, 0, sizeof(g));
    g.pts = clouds[k]->pts.p;
    g.nrm = c->has_normals ? clouds[k]->nrm.p : nullptr;
    g.cov = c->has_covs ? clouds[k]->cov.p : nullptr;
    g.T = merge_pose(T ? T + 16 * k : nullptr, clouds[k]->origin, o);
    g.n = static_cast<uint32_t>(clouds[k]->n);
    g.off = off;
    off += g.n;
    prefix[j + 1] = prefix[j] + (g.n + kIoBlock - 1u) / kIoBlock;
  }
  const uint32_t* d_prefix = nullptr;
  count_launch(Chain::Merge);
  SGA_TRY(upload_entries(ctx, table, members, prefix, &d_prefix));
  unsigned long long* note = nullptr;
  const unsigned long long seq = want_box ? note_begin(ctx, &note) : 0ull;
  count_launch(Chain::Merge);
  hipLaunchKernelGGL(merge_cloud_kernel, dim3(prefix[count]), dim3(kIoBlock), 0, ctx->stream, reinterpret_cast<const MergeMember*>(table.p), d_prefix, static_cast<int>(count), c->pts.p, c->nrm.p, c->cov.p,
                     want_box ? ctx->d_box64.p : nullptr, note, seq);
  SGA_HIP(hipGetLastError());
  if (want_box) {
    unsigned long long payload[kNoteWords - 1];
    SGA_TRY(note_wait(ctx, seq, payload));
    for (int k = 0; k < 3; k++) lo[k] = box_dec64(payload[k]), hi[k] = box_dec64(payload[3 + k]);
  }
  return SGA_OK;
}

int cloud_merge(sga_context* ctx, const sga_cloud* const* clouds, const double* T, size_t count, const double origin[3], sga_cloud** out) {
  if (out) *out = nullptr;  // on any failure *out is NULL
  if (!ctx || !out || (count > 0 && !clouds)) return fail(SGA_ERR_INVALID, "null argument");
  if (count > kMergeMaxMembers) return fail(SGA_ERR_INVALID, "too many members (%zu; limit %zu)", count, kMergeMaxMembers);
  for (size_t k = 0; k < count; k++)
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "null argument: clouds[%zu] is NULL", k);
  for (size_t k = 0; T != nullptr && k < count; k++)
    for (int e = 0; e < 16; e++)
      if (!(T[16 * k + e] - T[16 * k + e] == 0.0)) return fail(SGA_ERR_INVALID, "pose %zu has a non-finite entry", k);
  for (int k = 0; origin != nullptr && k < 3; k++)
    if (!(origin[k] - origin[k] == 0.0)) return fail(SGA_ERR_INVALID, "origin has a non-finite entry");
  // ---- (from here on the handles are read)
  size_t total = 0;
  std::vector<size_t> live;  // empty members take no workgroups
  bool normals = true, covs = true;  // an attribute is kept when every non-empty member has it
  for (size_t k = 0; k < count; k++) {
    if (clouds[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", k);
    if (clouds[k]->n == 0) continue;
    live.push_back(k);
    total += clouds[k]->n;
    normals = normals && clouds[k]->has_normals;
    covs = covs && clouds[k]->has_covs;
  }
  if (total >= (1ull << 31)) return fail(SGA_ERR_INVALID, "merged cloud too large (%zu points; limit 2^31-1)", total);
  if (total > 0) SGA_HIP(hipSetDevice(ctx->device));  // (no member, or empty members only: no attributes, no device work)
  StreamScope stream_scope(ctx->stream);
  std::unique_ptr<sga_cloud> c(new sga_cloud);
  c->device = ctx->device;
  c->n = total;
  for (int k = 0; k < 3; k++) c->origin[k] = origin ? origin[k] : 0.0;
  if (total == 0) {
    *out = c.release();
    return SGA_OK;
  }
  c->has_normals = normals;
  c->has_covs = covs;
  SGA_TRY(c->pts.alloc(total));
  if (normals) SGA_TRY(c->nrm.alloc(total));
  if (covs) SGA_TRY(c->cov.alloc(total));
  // The box of the finite posed points.  The origin is chosen from it (origin == NULL: the one host wait the data forces); a blocking
  // context, which waits anyway, also keeps it with the cloud.  A stream-ordered context with the origin given waits for nothing and its
  // cloud carries no box — sga_cloud_create_device's contract.
  const bool want_box = origin == nullptr || !ctx->stream_ordered;
  if (want_box) SGA_TRY(ensure_box64(ctx));
  for (size_t k : live) SGA_TRY(wait_ready(ctx, clouds[k]->ready));  // made by another context in stream-ordered mode (common.hpp: Ready)
  DevBuf<unsigned long long> table, table2;  // live to the end of the call (then: the stream's free list)
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  // origin == NULL: the first pass writes the records for the origin zero, so its box IS the box of the posed points in the caller's
  // frame — the same numbers whatever follows.  An origin other than zero (a submap far from the origin: rare) takes a second pass, which
  // starts from the members' records again and brings the box of its own records.
  SGA_TRY(merge_pass(ctx, clouds, T, live, c->origin, c.get(), want_box, table, lo, hi));
  if (origin == nullptr) {
    choose_origin(lo, hi, c->origin);
    if (!origin_is_zero(c->origin)) SGA_TRY(merge_pass(ctx, clouds, T, live, c->origin, c.get(), true, table2, lo, hi));
  }
  // (a note has shown that the last launch is over; without one the context is stream-ordered)
  cloud_set_box(c.get(), lo, hi, true, false);  // the rounding is monotone: the rounded box of the unrounded records is the box of the records
  SGA_TRY(mark_ready(ctx, c->ready));
  *out = c.release();
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

// Is [p, p + bytes) pinned host memory a kernel of this device can read (hipHostMalloc / hipHostRegister / sga_host_alloc)?  -> its device address
// on_device (optional): set when p is device memory, which no host entry point takes
static const void* pinned_device_view(const void* p, size_t bytes, bool* on_device = nullptr) {
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
  std::unique_ptr<sga_cloud> c(new sga_cloud);
  c->device = ctx->device;
  c->n = n;
  for (int k = 0; k < 3; k++) c->origin[k] = (frame != UploadFrame::FromBox && origin_in) ? origin_in[k] : 0.0;
  c->has_normals = normals != nullptr;
  c->has_covs = cov6 != nullptr;
  SGA_TRY(c->pts.alloc(n));
  if (normals) SGA_TRY(c->nrm.alloc(n));
  if (cov6) SGA_TRY(c->cov.alloc(n));
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

// The cloud whose fp32 coordinates are given RELATIVE to `origin` (true position = xyz_rel + origin): the records go to the device as they are.
// recentre_by != nullptr: absolute fp32 coordinates, records = fl32(double(x) - recentre_by).
static int cloud_create_rel(sga_context* ctx, const float* xyz, const float* normals, const float* cov6, size_t n, const double origin[3], const double* recentre_by, sga_cloud** out) {
  static const double zero[3] = {0, 0, 0};
  return cloud_upload(ctx, xyz, normals, cov6, n, recentre_by ? UploadFrame::GivenRecentre : UploadFrame::Given, origin ? origin : zero, out);
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

// ---- sga_cloud_deskew ------------------------------------------------------------------------------------------
// `count` sweeps, each point of member k posed by exp((s - ref_time_k) xi_k): one table — [members][prefix of the grid][box accumulators:
// 8 words per member][ticket] — and ONE launch over the concatenation.  The times come from host arrays (times != null: all members'
// in ONE slot of the staging ring, which the kernel reads by its device address) or, for a single member, from a device array (dtimes).
// A blocking context waits for the members' boxes (the context's box block: its one wait); a stream-ordered one waits for nothing.
static int cloud_deskew(sga_context* ctx, const sga_cloud* const* clouds, const float* const* times, const sga_device_array* dtimes, const double* twists, const double* ref_times, size_t count, void* user_stream, int flags, sga_cloud** out) {
  null_out(out, count);
  if (!ctx || (count > 0 && (!out || !clouds || (!times && !dtimes) || !twists))) return fail(SGA_ERR_INVALID, "null argument");
  if (count > kMergeMaxMembers) return fail(SGA_ERR_INVALID, "too many members (%zu; limit %zu)", count, kMergeMaxMembers);
  for (size_t k = 0; k < count; k++) {
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "null argument: clouds[%zu] is NULL", k);
    if (times != nullptr && !times[k]) return fail(SGA_ERR_INVALID, "null argument: times[%zu] is NULL", k);
  }
  for (size_t k = 0; k < count; k++) {
    for (int e = 0; e < 6; e++)
      if (!(twists[6 * k + e] - twists[6 * k + e] == 0.0)) return fail(SGA_ERR_INVALID, "twist %zu has a non-finite entry", k);
    if (ref_times != nullptr && !(ref_times[k] - ref_times[k] == 0.0)) return fail(SGA_ERR_INVALID, "reference time %zu is not finite", k);
  }
  if (count == 0) return SGA_OK;
  // ---- (from here on the handles are read)
  std::vector<size_t> live;  // empty members take no workgroups
  size_t total = 0, blocks = 0;
  for (size_t k = 0; k < count; k++) {
    if (clouds[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", k);
    if (clouds[k]->n == 0) continue;
    live.push_back(k);
    total += clouds[k]->n;
    blocks += (clouds[k]->n + kIoBlock - 1) / kIoBlock;
  }
  if (blocks >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points in all (%zu)", total);
  if (!live.empty()) SGA_HIP(hipSetDevice(ctx->device));
  for (size_t k : live) {
    if (times != nullptr) {
      bool on_device = false;
      (void)pinned_device_view(times[k], clouds[k]->n * sizeof(float), &on_device);
      if (on_device) return fail(SGA_ERR_INVALID, "times[%zu] is device memory: times that live on the device go through sga_cloud_deskew_device", k);
    } else {
      const size_t elem = dtimes->dtype == SGA_F64 ? 8 : 4;
      size_t span = 0;  // the last element read ends here: a column of a wider array need not own the rest of its last row
      if (__builtin_mul_overflow(clouds[k]->n - 1, static_cast<size_t>(dtimes->stride) * elem, &span) || __builtin_add_overflow(span, elem, &span))
        return fail(SGA_ERR_INVALID, "times: %zu rows of stride %d overflow the address space", clouds[k]->n, dtimes->stride);
      SGA_TRY(check_device_range(ctx, dtimes->data, span, elem, "times", "sga_cloud_deskew"));
    }
  }
  StreamScope stream_scope(ctx->stream);
  std::vector<std::unique_ptr<sga_cloud>> made(count);
  for (size_t k = 0; k < count; k++) {
    const sga_cloud* in = clouds[k];
    std::unique_ptr<sga_cloud> c(new sga_cloud);
    c->device = ctx->device;
    c->n = in->n;
    for (int a = 0; a < 3; a++) c->origin[a] = in->origin[a];  // a sweep moves by metres: it stays in its frame
    if (in->n > 0) {  // (an empty member: an empty cloud without attributes)
      c->has_normals = in->has_normals;
      c->has_covs = in->has_covs;
      SGA_TRY(c->pts.alloc(in->n));
      if (in->has_normals) SGA_TRY(c->nrm.alloc(in->n));
      if (in->has_covs) SGA_TRY(c->cov.alloc(in->n));
    }
    made[k] = std::move(c);
  }
  auto hand_over = [&]() {
    for (size_t k = 0; k < count; k++) out[k] = made[k].release();
    return SGA_OK;
  };
  if (live.empty()) return hand_over();
  const size_t L = live.size();
  const bool want_box = !ctx->stream_ordered;
  for (size_t k : live) SGA_TRY(wait_ready(ctx, clouds[k]->ready));  // made by another context in stream-ordered mode (common.hpp: Ready)
  // ---- host times: all members' in one slot of the staging ring
  sga_context::StageSlot* tslot = nullptr;
  if (times != nullptr) {
    SGA_TRY(stage_acquire(ctx, total * sizeof(float), &tslot));
    size_t off = 0;
    for (size_t k : live) {
      std::memcpy(static_cast<float*>(tslot->host) + off, times[k], clouds[k]->n * sizeof(float));
      off += clouds[k]->n;
    }
  }
  // ---- the table
  TableLayout lay;
  const auto s_members = lay.add<DeskewMember>(L);
  const auto s_prefix = lay.add_prefixes(1, L);
  const auto s_acc = lay.add<unsigned long long>(want_box ? 8 * L : 0);
  const auto s_ticket = lay.add<unsigned>(1);
  DevBuf<unsigned long long> table;  // lives to the end of the call (then: the stream's free list)
  SGA_TRY(table.alloc(lay.words()));
  ForestBoxes hand{nullptr, 0u, nullptr, 0ull};
  if (want_box) {
    SGA_TRY(forest_call_begin(ctx, L, kDeskewSlotWords, &hand.seq));
    hand.ticket = lay.at(s_ticket, table.p);
    hand.total = static_cast<unsigned>(L);
    hand.seq_word = ctx->h_forest_dev;
  }
  std::vector<DeskewMember> members(L);
  std::vector<uint32_t> prefix(L + 1, 0u);
  size_t toff = 0;
  for (size_t j = 0; j < L; j++) {
    const size_t k = live[j];
    const sga_cloud* in = clouds[k];
    DeskewMember& g = members[j];
    std::memset(&g, 0, sizeof(g));
    g.pts = in->pts.p, g.nrm = in->has_normals ? in->nrm.p : nullptr, g.cov = in->has_covs ? in->cov.p : nullptr;
    g.opts = made[k]->pts.p, g.onrm = made[k]->nrm.p, g.ocov = made[k]->cov.p;
    if (times != nullptr) {
      g.times = static_cast<const float*>(tslot->dev) + toff, g.tstride = 1, g.tf64 = 0;
      toff += in->n;
    } else {
      g.times = dtimes->data, g.tstride = dtimes->stride, g.tf64 = dtimes->dtype == SGA_F64 ? 1 : 0;
    }
    if (want_box) g.acc = lay.at(s_acc, table.p) + 8 * j, g.slot = forest_slot_dev(ctx, j, kDeskewSlotWords);
    g.ref_time = ref_times ? ref_times[k] : 1.0;
    g.c = twist_const(twists + 6 * k, in->origin);
    g.n = static_cast<uint32_t>(in->n);
    g.blocks = (g.n + kIoBlock - 1u) / kIoBlock;
    prefix[j + 1] = prefix[j] + g.blocks;
  }
  IoOrder ord;
  if (dtimes != nullptr) SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  auto enqueue = [&]() -> int {
    count_launch(Chain::Deskew);
    SGA_TRY(upload_table(ctx, table.p, lay.words(), [&](unsigned long long* host) {
      lay.put(s_members, host, members.data());
      lay.put(s_prefix, host, prefix.data());
      for (size_t w = 0; w < s_acc.count; w++)
        if (w % 8 < 6) lay.at(s_acc, host)[w] = box_enc64(w % 8 < 3 ? INFINITY : -INFINITY);
    }));
    count_launch(Chain::Deskew);
    hipLaunchKernelGGL(deskew_cloud_kernel, dim3(prefix[L]), dim3(kIoBlock), 0, ctx->stream, lay.at(s_members, table.p), lay.at(s_prefix, table.p), static_cast<int>(L), hand);
    SGA_HIP(hipGetLastError());
    return SGA_OK;
  };
  if (!want_box) {  // a stream-ordered context waits for nothing
    SGA_TRY(enqueue());
    if (tslot != nullptr) SGA_TRY(stage_release(ctx, tslot));
  } else {  // (a blocking context: the wait shows that the kernel is over)
    SGA_TRY(forest_call_wait(ctx, enqueue(), hand.seq, "boxes of a deskew"));
    for (size_t j = 0; j < L; j++) {
      const unsigned long long* slot = forest_slot_host(ctx, j, kDeskewSlotWords);
      double lo[3], hi[3];
      for (int a = 0; a < 3; a++) lo[a] = box_dec64(slot[kDeskewSlotLo + a]), hi[a] = box_dec64(slot[kDeskewSlotHi + a]);
      cloud_set_box(made[live[j]].get(), lo, hi, true, false);  // the rounding is monotone: the rounded box of the unrounded records is the box of the records
    }
  }
  if (dtimes != nullptr) SGA_TRY(io_end(ctx, ord));
  for (size_t k : live) SGA_TRY(mark_ready(ctx, made[k]->ready));
  return hand_over();
}

namespace sga {
// absolute fp32 coordinates, recentred about a GIVEN origin (multi.hip: the shards of one source share a device frame)
int cloud_create_f32_about(sga_context* ctx, const float* xyz, const float* normals, const float* cov6, size_t n, const double origin[3], sga_cloud** out) {
  return cloud_create_rel(ctx, xyz, normals, cov6, n, origin, origin_is_zero(origin) ? nullptr : origin, out);
}
void host_bbox_f32(const float* xyz, size_t n, double lo[3], double hi[3]) { host_bbox(xyz, n, 3, lo, hi); }
void host_bbox_f64(const double* xyzw, size_t n, double lo[3], double hi[3]) { host_bbox(xyzw, n, 4, lo, hi); }
}  // namespace sga
extern "C" {

int sga_cloud_create_f32_origin(sga_context* ctx, const float* xyz_rel, const float* normals, const float* cov6, size_t n, const double origin[3], sga_cloud** out) {
  return cloud_create_rel(ctx, xyz_rel, normals, cov6, n, origin, nullptr, out);
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
    for (size_t i = 0; i < n; i++) {
      const double* m = cov4x4 + 16 * i;  // symmetric: storage order irrelevant
      cov[6 * i + 0] = static_cast<float>(m[0]);
      cov[6 * i + 1] = static_cast<float>(m[1]);
      cov[6 * i + 2] = static_cast<float>(m[2]);
      cov[6 * i + 3] = static_cast<float>(m[5]);
      cov[6 * i + 4] = static_cast<float>(m[6]);
      cov[6 * i + 5] = static_cast<float>(m[10]);
    }
  }
  return cloud_create_rel(ctx, xyz.data(), normals4 ? nrm.data() : nullptr, cov4x4 ? cov.data() : nullptr, n, origin, nullptr, out);
}

int sga_cloud_create_f64(sga_context* ctx, const double* xyzw, const double* normals4, const double* cov4x4, size_t n, sga_cloud** out) {
  return sga_cloud_create_f64_origin(ctx, xyzw, normals4, cov4x4, n, nullptr, out);
}

int sga_cloud_origin(const sga_cloud* cloud, double origin[3]) {
  if (!cloud || !origin) return fail(SGA_ERR_INVALID, "null argument");
  for (int k = 0; k < 3; k++) origin[k] = cloud->origin[k];
  return SGA_OK;
}

int sga_cloud_slice(sga_context* ctx, const sga_cloud* cloud, size_t first, size_t count, sga_cloud** out) {
  if (!ctx || !cloud || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (first > cloud->n || count > cloud->n - first) return fail(SGA_ERR_INVALID, "slice [%zu, %zu) outside a cloud of %zu points", first, first + count, cloud->n);
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  *out = nullptr;
  SGA_ENTER(ctx);
  auto* c = new sga_cloud;
  c->device = ctx->device;
  c->n = count;
  for (int k = 0; k < 3; k++) c->origin[k] = cloud->origin[k];  // the slice stays in its cloud's device frame: shards of one registration share it
  c->has_normals = cloud->has_normals;
  c->has_covs = cloud->has_covs;
  int rc = c->pts.alloc(count);
  if (rc == SGA_OK && cloud->has_normals) rc = c->nrm.alloc(count);
  if (rc == SGA_OK && cloud->has_covs) rc = c->cov.alloc(count);
  if (rc != SGA_OK) {
    delete c;
    return rc;
  }
  if (count > 0) {
    hipLaunchKernelGGL(slice_cloud_kernel, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, cloud->pts.p, cloud->has_normals ? cloud->nrm.p : nullptr, cloud->has_covs ? cloud->cov.p : nullptr, first, count, c->pts.p, c->nrm.p, c->cov.p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
      delete c;
      return fail(SGA_ERR_HIP, "slice kernel: %s", hipGetErrorString(e));
    }
  }
  *out = c;
  return SGA_OK;
}

// Posed clouds joined into one (the host loop of src/test/registration_test.cpp:84 over points, normals and covs, on the device)
int sga_cloud_merge(sga_context* ctx, const sga_cloud* const* clouds, const double* T, size_t count, const double origin[3], sga_cloud** out) { return cloud_merge(ctx, clouds, T, count, origin, out); }

int sga_cloud_transform(sga_context* ctx, const sga_cloud* cloud, const double T[16], const double origin[3], sga_cloud** out) { return cloud_merge(ctx, &cloud, T, 1, origin, out); }

// Sweeps deskewed on the device: every point posed by exp((its time - ref_time) twist), DESIGN.md section 3.19
int sga_cloud_deskew_batch(sga_context* ctx, const sga_cloud* const* clouds, const float* const* times, const double* twists, const double* ref_times, size_t count, sga_cloud** out) {
  return cloud_deskew(ctx, clouds, times, nullptr, twists, ref_times, count, nullptr, 0, out);
}

int sga_cloud_deskew(sga_context* ctx, const sga_cloud* cloud, const float* times, const double twist[6], double ref_time, sga_cloud** out) {
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  return cloud_deskew(ctx, &cloud, &times, nullptr, twist, &ref_time, 1, nullptr, 0, out);
}

int sga_cloud_deskew_device(sga_context* ctx, const sga_cloud* cloud, const sga_device_array* times, const double twist[6], double ref_time, void* user_stream, int flags, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!out || !times) return fail(SGA_ERR_INVALID, "null argument");
  if (times->dtype != SGA_F32 && times->dtype != SGA_F64) return fail(SGA_ERR_INVALID, "times: dtype %d is neither SGA_F32 nor SGA_F64", times->dtype);
  if (times->cols != 1 || times->stride < 1) return fail(SGA_ERR_INVALID, "times: cols = %d, stride = %d (one time per row, rows one element or more apart)", times->cols, times->stride);
  return cloud_deskew(ctx, &cloud, nullptr, times, twist, &ref_time, 1, user_stream, flags, out);
}

int sga_debug_cloud_deskew_launches(unsigned long long* launches) { return report_launches(Chain::Deskew, launches); }

int sga_debug_cloud_merge_launches(unsigned long long* launches) { return report_launches(Chain::Merge, launches); }

int sga_debug_cloud_box(const sga_cloud* cloud, int* has_box, float lo[3], float hi[3]) {
  if (!cloud || !has_box || !lo || !hi) return fail(SGA_ERR_INVALID, "null argument");
  *has_box = cloud->has_box ? 1 : 0;
  for (int k = 0; k < 3; k++) lo[k] = cloud->has_box ? cloud->box_lo[k] : 0.f, hi[k] = cloud->has_box ? cloud->box_hi[k] : 0.f;
  return SGA_OK;
}

int sga_cloud_destroy(sga_cloud* cloud) {
  if (cloud) {
    (void)hipSetDevice(cloud->device);
    delete cloud;
  }
  return SGA_OK;
}

int sga_cloud_size(const sga_cloud* cloud, size_t* n) {
  if (!cloud || !n) return fail(SGA_ERR_INVALID, "null argument");
  *n = cloud->n;
  return SGA_OK;
}

int sga_cloud_has(const sga_cloud* cloud, int* has_normals, int* has_covs) {
  if (!cloud) return fail(SGA_ERR_INVALID, "null argument");
  if (has_normals) *has_normals = cloud->has_normals;
  if (has_covs) *has_covs = cloud->has_covs;
  return SGA_OK;
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
  std::unique_ptr<sga_cloud> c(new sga_cloud);
  c->device = ctx->device;
  c->n = n;
  c->has_normals = normals != nullptr;
  c->has_covs = covs != nullptr;
  SGA_TRY(c->pts.alloc(n));
  if (normals) SGA_TRY(c->nrm.alloc(n));
  if (covs) SGA_TRY(c->cov.alloc(n));
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
  for (int k = 0; k < 3 && origin != nullptr; k++) c->origin[k] = origin[k];
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

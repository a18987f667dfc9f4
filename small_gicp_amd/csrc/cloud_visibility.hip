// The free-space check of a mapping loop on the device: sga_cloud_visibility — the range image of a posed scan
// (the least range per cell, by a 64-bit atomicMin on the bit pattern of the double), the state of every map point against the cells of
// its window (unobserved, consistent, occluded, seen through) with its clearance, the four counts, and the crop's stable compaction
// (cloud_crop.hip: cloud_crop_stat, cloud_ops.hpp) over the seen-through points or over all the others.  The rule is stated in
// include/small_gicp_amd.h and restated in tests/visibility_ref.py.
#include "cloud_ops.hpp"
#include "projective.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kVisBlock = 64;  // points of a workgroup: one lane each, one wave
constexpr int kVisCountThreads = 1024;
constexpr unsigned long long kVisEmpty = ~0ull;  // a cell without a return: the byte fill's all-ones, above the bits of every range

// The projection's constants (kernel arguments: read with scalar loads)
struct VisImage {
  int W, H;
  double fov_up, span;  // span = fov_up - fov_down
  double min_range;
};

// What the state kernel receives
struct VisArgs {
  const float4* pts;  // the map's records, its order
  double rt[9];       // rt[3 k + j] = R[j][k]: row k of R^T
  double d[3];        // o_m - t
  VisImage g;
  double max_range, margin, margin_ratio;
  const unsigned long long* img;  // [v * W + u]
  uint8_t* state;                 // n, device memory: what the count kernel reads
  double* flag;                   // n, or null: 0.0 where the compaction keeps the point, 1.0 where it does not (held against 0.5)
  uint8_t* state_host;            // the states, the clearances and the image into a slot of the staging ring, by its device address; or null
  double* clearance_host;
  double* img_host;
  uint32_t n, cells;
  int wh, wv;
  int keep;  // 1: the seen-through are kept, 2: all the others
};

__device__ __forceinline__ bool vis_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The projection, stated once (small_gicp_amd.h: sga_cloud_visibility): true iff s is in the image; then 0 <= u < W, 0 <= v < H.
__device__ __forceinline__ bool vis_project(const VisImage& g, double sx, double sy, double sz, double& rho, int& u, int& v) {
  rho = 0.0, u = 0, v = 0;
  if (!(vis_finite(sx) && vis_finite(sy) && vis_finite(sz))) return false;
  rho = sqrt((proj_sq(sx) + proj_sq(sy)) + proj_sq(sz));
  if (!(rho > 0.0) || !vis_finite(rho)) return false;
  const double az = atan2(sy, sx);
  const double el = asin(sz / rho);
  const double su = (az / (2.0 * M_PI) + 0.5) * static_cast<double>(g.W);
  const double sv = (g.fov_up - el) / g.span * static_cast<double>(g.H);
  if (!(vis_finite(su) && vis_finite(sv))) return false;
  if (!(su >= 0.0 && su <= static_cast<double>(g.W))) return false;  // (|az| <= pi: cannot happen; keeps every index inside the image whatever atan2 returns)
  u = static_cast<int>(su);
  if (u == g.W) u = 0;
  if (!(sv >= 0.0)) return false;
  const double vf = floor(sv);
  if (!(vf < static_cast<double>(g.H))) return false;
  v = static_cast<int>(vf);
  return true;
}

}  // namespace

// The range image: one thread per return of the scan.  A finite return in the image with rho >= min_range lowers its cell to rho.  The
// plain load skips the atomic where the cell is nearer already (it may read an older, greater value: then the atomic decides).
__global__ __launch_bounds__(kVisBlock) void visibility_image_kernel(const float4* __restrict__ pts, uint32_t n, double ox, double oy, double oz, const VisImage g, unsigned long long* __restrict__ img) {
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kVisBlock) + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  double rho;
  int u, v;
  if (!vis_project(g, static_cast<double>(p.x) + ox, static_cast<double>(p.y) + oy, static_cast<double>(p.z) + oz, rho, u, v)) return;
  if (!(rho >= g.min_range)) return;
  unsigned long long* cell = img + (static_cast<size_t>(v) * g.W + u);
  const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(rho));  // rho > 0: positive doubles order as their bits
  if (*cell <= bits) return;
  atomicMin(cell, bits);
}

// The state, the clearance and the keep flag of every map point, each written at the point's own index; one lane per point.  The first
// `cells` threads of the grid also hand the image's cells to the host (all-ones becomes +inf) when it is asked for.
__global__ __launch_bounds__(kVisBlock) void visibility_state_kernel(const VisArgs a) {
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kVisBlock) + threadIdx.x;
  if (a.img_host != nullptr && i < a.cells) {
    const unsigned long long c = a.img[i];
    a.img_host[i] = c == kVisEmpty ? static_cast<double>(INFINITY) : __longlong_as_double(static_cast<long long>(c));
  }
  if (i < a.n) {
    const float4 p = a.pts[i];
    const double w0 = static_cast<double>(p.x) + a.d[0], w1 = static_cast<double>(p.y) + a.d[1], w2 = static_cast<double>(p.z) + a.d[2];
    const double sx = (a.rt[0] * w0 + a.rt[1] * w1) + a.rt[2] * w2;
    const double sy = (a.rt[3] * w0 + a.rt[4] * w1) + a.rt[5] * w2;
    const double sz = (a.rt[6] * w0 + a.rt[7] * w1) + a.rt[8] * w2;
    double rho;
    int u, v;
    int state = 0;
    double clearance = static_cast<double>(NAN);
    if (vis_project(a.g, sx, sy, sz, rho, u, v) && rho >= a.g.min_range && rho <= a.max_range) {
      unsigned long long lo = kVisEmpty, hi = 0ull;  // the least and the greatest finite cell of the window (no range is 0)
      for (int dv = -a.wv; dv <= a.wv; dv++) {
        const int vc = v + dv;
        if (vc < 0 || vc >= a.g.H) continue;
        const unsigned long long* __restrict__ row = a.img + static_cast<size_t>(vc) * a.g.W;  // one contiguous run per window row, but for the seam
        for (int du = -a.wh; du <= a.wh; du++) {
          int uc = (u + du) % a.g.W;  // (|du| <= 16 may exceed a narrow image more than once)
          if (uc < 0) uc += a.g.W;
          const unsigned long long c = row[uc];
          if (c == kVisEmpty) continue;
          lo = c < lo ? c : lo;
          hi = c > hi ? c : hi;
        }
      }
      if (lo != kVisEmpty) {
        const double m = __longlong_as_double(static_cast<long long>(lo)), M = __longlong_as_double(static_cast<long long>(hi));
        const double tol = a.margin + a.margin_ratio * rho;
        state = rho + tol < m ? 3 : (rho - tol > M ? 2 : 1);
        clearance = m - rho;
      }
    }
    a.state[i] = static_cast<uint8_t>(state);
    if (a.flag != nullptr) a.flag[i] = (state == 3) == (a.keep == 1) ? 0.0 : 1.0;
    if (a.state_host != nullptr) a.state_host[i] = static_cast<uint8_t>(state);
    if (a.clearance_host != nullptr) a.clearance_host[i] = clearance;
  }
  if (a.state_host != nullptr || a.clearance_host != nullptr || a.img_host != nullptr) __threadfence_system();
}

// The four counts, by ONE workgroup: thread t counts the states 4 t .. 4 t + 3, 4 (t + 1024) .., a word at a time; the counts are
// integers, so the order in which the waves' sums meet in LDS cannot change them.  out4 = {unobserved, consistent, occluded, seen
// through} in a slot of the staging ring.
__global__ __launch_bounds__(kVisCountThreads) void visibility_count_kernel(const uint8_t* __restrict__ state, uint32_t n, unsigned long long* __restrict__ out4) {
  __shared__ uint32_t sh[4];
  const int tid = threadIdx.x;
  if (tid < 4) sh[tid] = 0u;
  __syncthreads();
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  auto add = [&](uint32_t s) {
#pragma unroll
    for (int k = 0; k < 4; k++) c[k] += s == static_cast<uint32_t>(k) ? 1u : 0u;
  };
  const uint32_t words = n / 4u;  // (the states start at an 8-byte boundary)
  const uint32_t* __restrict__ state4 = reinterpret_cast<const uint32_t*>(state);
  for (uint32_t w = tid; w < words; w += kVisCountThreads) {
    const uint32_t x = state4[w];
    add(x & 0xffu), add((x >> 8) & 0xffu), add((x >> 16) & 0xffu), add(x >> 24);
  }
  if (static_cast<uint32_t>(tid) < n - 4u * words) add(state[4u * words + tid]);
#pragma unroll
  for (int k = 0; k < 4; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_xor(c[k], off);
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; k++) atomicAdd(&sh[k], c[k]);
  }
  __syncthreads();
  if (tid < 4) out4[tid] = sh[tid];
  if (tid < 4) __threadfence_system();
}

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

// what sga_cloud_visibility refuses of its arguments (no handle is read)
int visibility_check(const double* T, const sga_visibility& p, const int64_t* kept, sga_cloud* const* out) {
  if (p.width < 1 || p.height < 1) return fail(SGA_ERR_INVALID, "visibility: an image of %d x %d", p.width, p.height);
  if (static_cast<long long>(p.width) * p.height > (1ll << 24)) return fail(SGA_ERR_INVALID, "visibility: an image of %d x %d has more than 2^24 cells", p.width, p.height);
  if (!is_finite(p.fov_up) || !is_finite(p.fov_down) || std::fabs(p.fov_up) > M_PI / 2 || std::fabs(p.fov_down) > M_PI / 2) return fail(SGA_ERR_INVALID, "visibility: fov_up and fov_down must lie in [-pi/2, pi/2] (radians)");
  if (!(p.fov_up > p.fov_down)) return fail(SGA_ERR_INVALID, "visibility: fov_up must be above fov_down");
  if (!is_finite(p.min_range) || p.min_range < 0.0) return fail(SGA_ERR_INVALID, "visibility: min_range must be finite and >= 0");
  if (!(p.max_range >= p.min_range)) return fail(SGA_ERR_INVALID, "visibility: max_range is NaN or below min_range (+inf is allowed)");
  if (!is_finite(p.margin) || p.margin < 0.0 || !is_finite(p.margin_ratio) || p.margin_ratio < 0.0) return fail(SGA_ERR_INVALID, "visibility: margin and margin_ratio must be finite and >= 0");
  if (p.window_h < 0 || p.window_h > 16 || p.window_v < 0 || p.window_v > 16) return fail(SGA_ERR_INVALID, "visibility: window %d x %d is outside [0, 16]", p.window_h, p.window_v);
  if (p.keep < 0 || p.keep > 2) return fail(SGA_ERR_INVALID, "visibility: keep %d is not 0 (no cloud), 1 (the seen-through) or 2 (all the others)", p.keep);
  if (p.keep == 0 && out != nullptr) return fail(SGA_ERR_INVALID, "visibility: keep is 0 but an output cloud is asked for");
  if (p.keep != 0 && out == nullptr) return fail(SGA_ERR_INVALID, "visibility: keep is %d but there is no place for the output cloud", p.keep);
  if (p.keep == 0 && kept != nullptr) return fail(SGA_ERR_INVALID, "visibility: kept is given but keep is 0");
  for (int k = 0; T != nullptr && k < 16; k++)
    if (!is_finite(T[k])) return fail(SGA_ERR_INVALID, "visibility: T has a non-finite entry");
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_visibility_default(sga_visibility* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->width = 1024, p->height = 64;
  p->fov_up = 3.0 * M_PI / 180.0, p->fov_down = -25.0 * M_PI / 180.0;
  p->min_range = 0.5, p->max_range = 60.0;
  p->margin = 0.2, p->margin_ratio = 0.01;
  p->window_h = 1, p->window_v = 1;
}

int sga_cloud_visibility(sga_context* ctx, const sga_cloud* map, const sga_cloud* scan, const double T[16], const sga_visibility* params, uint8_t* state, double* clearance, double* range_image, int64_t* kept,
                         sga_visibility_stats* stats, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !map || !scan || !params) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(visibility_check(T, *params, kept, out));
  // ---- (from here on the handles are read)
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (map->device != ctx->device) return fail(SGA_ERR_INVALID, "map lives on another device");
  if (scan->device != ctx->device) return fail(SGA_ERR_INVALID, "scan lives on another device");
  const size_t n = map->n, ns = scan->n;
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many map points (%zu; limit 2^31-1)", n);
  if (ns >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many scan points (%zu; limit 2^31-1)", ns);
  CropStat cs{nullptr, nullptr, 0.5, Chain::Visibility};
  if (n == 0 && range_image == nullptr) return out ? cloud_crop_stat(ctx, map, cs, kept, out) : SGA_OK;  // an empty cloud, zeroed stats; nothing is enqueued
  SGA_ENTER(ctx);
  if (ns > 0) SGA_TRY(wait_ready(ctx, scan->ready));  // made on another context that returned before its kernels had run
  if (n > 0) SGA_TRY(wait_ready(ctx, map->ready));
  const size_t cells = static_cast<size_t>(params->width) * static_cast<size_t>(params->height);
  // the image, behind it the keep flags, behind them the states (bytes); lives to the end of the call (then: the stream's free list)
  const size_t flag_words = out ? n : 0, state_words = (n + 7) / 8;
  DevBuf<unsigned long long> buf;
  SGA_TRY(buf.alloc(cells + flag_words + state_words));
  // the counts, the clearances, the image and the states leave through ONE slot of the staging ring, which the kernels write by its device address
  const size_t c_words = clearance != nullptr ? n : 0, i_words = range_image != nullptr ? cells : 0;
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, (4 + c_words + i_words + (state != nullptr ? state_words : 0)) * 8, &slot));
  unsigned long long* slot_dev = static_cast<unsigned long long*>(slot->dev);
  VisArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pts = map->pts.p;
  for (int k = 0; k < 3; k++) {
    for (int j = 0; j < 3; j++) a.rt[3 * k + j] = T ? T[4 * k + j] : (j == k ? 1.0 : 0.0);  // R[j][k]: T is column-major
    a.d[k] = map->origin[k] - (T ? T[12 + k] : 0.0);
  }
  a.g = VisImage{params->width, params->height, params->fov_up, params->fov_up - params->fov_down, params->min_range};
  a.max_range = params->max_range, a.margin = params->margin, a.margin_ratio = params->margin_ratio;
  a.img = buf.p;
  a.flag = out ? reinterpret_cast<double*>(buf.p + cells) : nullptr;
  a.state = reinterpret_cast<uint8_t*>(buf.p + cells + flag_words);
  a.clearance_host = clearance != nullptr ? reinterpret_cast<double*>(slot_dev + 4) : nullptr;
  a.img_host = range_image != nullptr ? reinterpret_cast<double*>(slot_dev + 4 + c_words) : nullptr;
  a.state_host = state != nullptr ? reinterpret_cast<uint8_t*>(slot_dev + 4 + c_words + i_words) : nullptr;
  a.n = static_cast<uint32_t>(n), a.cells = static_cast<uint32_t>(cells);
  a.wh = params->window_h, a.wv = params->window_v;
  a.keep = params->keep;
  count_launch(Chain::Visibility);
  SGA_HIP(hipMemsetAsync(buf.p, 0xff, cells * 8, ctx->stream));
  if (ns > 0) {
    count_launch(Chain::Visibility);
    hipLaunchKernelGGL(visibility_image_kernel, dim3(static_cast<unsigned>((ns + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, ctx->stream, scan->pts.p, static_cast<uint32_t>(ns), scan->origin[0], scan->origin[1],
                       scan->origin[2], a.g, buf.p);
    SGA_HIP(hipGetLastError());
  }
  const size_t threads = n > i_words ? n : i_words;  // (> 0: a call with an empty map has come here for the image)
  count_launch(Chain::Visibility);
  hipLaunchKernelGGL(visibility_state_kernel, dim3(static_cast<unsigned>((threads + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  if (n > 0) {
    count_launch(Chain::Visibility);
    hipLaunchKernelGGL(visibility_count_kernel, dim3(1), dim3(kVisCountThreads), 0, ctx->stream, a.state, a.n, slot_dev);
    SGA_HIP(hipGetLastError());
  }
  sga_cloud* made = nullptr;
  if (out) {
    cs.d = a.flag;
    SGA_TRY(cloud_crop_stat(ctx, map, cs, kept, &made));  // (its wait shows that everything above has run; an empty map: an empty cloud, no wait)
  }
  if (!out || n == 0) SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait: the counts are in the slot
  const unsigned long long* host = static_cast<const unsigned long long*>(slot->host);
  if (stats && n > 0) {
    stats->points = n;
    stats->unobserved = static_cast<size_t>(host[0]), stats->consistent = static_cast<size_t>(host[1]);
    stats->occluded = static_cast<size_t>(host[2]), stats->seen_through = static_cast<size_t>(host[3]);
  }
  if (clearance) std::memcpy(clearance, host + 4, n * sizeof(double));
  if (range_image) std::memcpy(range_image, host + 4 + c_words, cells * sizeof(double));
  if (state) std::memcpy(state, host + 4 + c_words + i_words, n);
  if (out) *out = made;
  return SGA_OK;
}

int sga_debug_cloud_visibility_launches(unsigned long long* launches) { return report_launches(Chain::Visibility, launches); }

}  // extern "C"

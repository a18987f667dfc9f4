// Plane segmentation on the device: sga_cloud_segment_plane — RANSAC over triples of records.  One lane per
// hypothesis for the draw, the tests and the orientation (a table of unit normals and anchors); the scores tiled over (points x
// hypotheses): a workgroup holds its points in registers as doubles and walks a tile of hypotheses staged in LDS, one ballot per wave and
// point row, one integer atomic per workgroup and hypothesis; the best by one workgroup; the refit sums and the final flags in fixed
// slots and a fixed order; the crop's stable compaction (cloud_crop.hip: cloud_crop_stat) when a cloud is asked for.  The host solves
// the 3x3 eigenproblem (rigid_fit.hip: sym3_eigen) between the two waits.  No floating-point atomic, no spin, no grid barrier.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "ransac.hpp"

#include <algorithm>
#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kPlBlock = 256;                          // every kernel but the selection
constexpr int kPlRows = 4;                             // score kernel: points of a lane, in registers (12 doubles)
constexpr int kPlPointTile = kPlBlock * kPlRows;       // ... points of a workgroup: 1024
constexpr int kPlHypTile = 32;                         // ... hypotheses of a workgroup, in LDS
constexpr int kPlHypWords = 8;                         // a row of the table: nhat (3), a (3), valid (1.0 / 0.0), 0
constexpr int kPlSelectThreads = 1024;
constexpr int kPlSums = 11;                            // count, sum x (3), sum x x^T (xx xy xz yy yz zz), sum of squared distances
constexpr uint32_t kPlMaxGroups = 256;                 // workgroups of the sums and the flags kernel: G = min(256, ceil(n / 1024))
constexpr uint32_t kPlDropped = 0xFFFFFFFFu;
constexpr uint64_t kPlMaxIterations = 1ull << 20;
constexpr size_t kPlHeadBytes = 64;                    // the slot's head: best word, scored, nhat (3), a (3)

// What the kernels receive (kernel arguments: read with scalar loads)
struct PlaneArgs {
  const float4* pts;  // the cloud's records, its order
  uint32_t n, H;
  uint64_t seed;
  double thr;
  double ax, ay, az, axis_norm, cos_max;  // the constraint (has_axis)
  int has_axis, keep;
  double* table;               // H rows of kPlHypWords
  uint32_t* scores;            // H
  unsigned long long* status;  // [0] the best word (score << 32 | 0xFFFFFFFF - h; 0: nothing scored), [1] hypotheses scored
  // a slot of the staging ring, by its device address
  unsigned long long* head_host;  // the best word, scored; behind them as doubles: nhat, a of the best hypothesis
  uint32_t* scores_host;          // H, or null
  double* sums_host;              // G x kPlSums
  double* final_host;             // G x {count, sum of squared distances}
  // the final plane (flags kernel)
  double fn[3], fa[3];
  double* flag;  // n, or null: 0.0 where the compaction keeps the point, 1.0 where it does not (held against 0.5)
  uint32_t G;
};

struct Vec3 {
  double x, y, z;
};
__host__ __device__ __forceinline__ double norm3(const Vec3 a) { return sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); }

// THE distance, stated once: every kernel that decides "inlier" calls this function, so a record is an inlier of the scores, of the sums
// and of the flags alike.  (nx dx + ny dy) + nz dz with the products fused into the sums.
__device__ __forceinline__ double plane_dist(double nx, double ny, double nz, double ax, double ay, double az, double x, double y, double z) {
  return fma(nz, z - az, fma(ny, y - ay, nx * (x - ax)));
}

// orientation and the axis constraint of a unit normal; false: the constraint drops it
__host__ __device__ __forceinline__ bool plane_orient(Vec3& n, int has_axis, double ax, double ay, double az, double axis_norm, double cos_max) {
  if (has_axis != 0) {
    double s = (n.x * ax + n.y * ay) + n.z * az;
    if (s < 0.0) n = {-n.x, -n.y, -n.z}, s = -s;
    return s / axis_norm >= cos_max;
  }
  const double lead = n.z != 0.0 ? n.z : (n.y != 0.0 ? n.y : n.x);
  if (lead < 0.0) n = {-n.x, -n.y, -n.z};
  return true;
}

// the records t, t + 256 G, ... of lane t of workgroup g: the order of every sum over points
template <typename Body>
__device__ __forceinline__ void plane_for_points(const PlaneArgs& a, Body&& body) {
  const uint32_t stride = a.G * static_cast<uint32_t>(kPlBlock);  // <= 65536, and n < 2^31: no wrap
  for (uint32_t i = blockIdx.x * static_cast<uint32_t>(kPlBlock) + threadIdx.x; i < a.n; i += stride) body(i, a.pts[i]);
}

// the 256 lanes' partials of C sums meet in a fixed binary tree; sh[c][0] holds the totals afterwards
template <int C>
__device__ __forceinline__ void plane_block_tree(double (*sh)[kPlBlock], const double* acc) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int c = 0; c < C; c++) sh[c][tid] = acc[c];
  __syncthreads();
  for (int off = kPlBlock / 2; off > 0; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int c = 0; c < C; c++) sh[c][tid] += sh[c][tid + off];
    }
    __syncthreads();
  }
}

}  // namespace

// One lane per hypothesis: the draw, the degeneracy tests, the unit normal and its orientation; row h of the table and scores[h] = 0, or
// 0xFFFFFFFF for a dropped hypothesis (the selection counts the others).
__global__ __launch_bounds__(kPlBlock) void plane_hypotheses_kernel(const PlaneArgs a) {
  const uint32_t h = blockIdx.x * static_cast<uint32_t>(kPlBlock) + threadIdx.x;
  if (h >= a.H) return;
  uint64_t id[3];
  ransac_draw(a.seed, h, a.n, id);  // three distinct numbers below n
  const float4 pa = a.pts[id[0]], pb = a.pts[id[1]], pc = a.pts[id[2]];
  const Vec3 A{pa.x, pa.y, pa.z};
  const Vec3 u{static_cast<double>(pb.x) - A.x, static_cast<double>(pb.y) - A.y, static_cast<double>(pb.z) - A.z};
  const Vec3 v{static_cast<double>(pc.x) - A.x, static_cast<double>(pc.y) - A.y, static_cast<double>(pc.z) - A.z};
  const Vec3 m{u.y * v.z - u.z * v.y, u.z * v.x - u.x * v.z, u.x * v.y - u.y * v.x};
  const double lm = norm3(m);
  bool valid = !(!(lm > 0.0) || lm < 1e-9 * norm3(u) * norm3(v) || !(lm < static_cast<double>(INFINITY)));
  Vec3 nh{0.0, 0.0, 0.0};
  if (valid) {
    nh = {m.x / lm, m.y / lm, m.z / lm};
    valid = plane_orient(nh, a.has_axis, a.ax, a.ay, a.az, a.axis_norm, a.cos_max);
  }
  double* row = a.table + static_cast<size_t>(kPlHypWords) * h;
  row[0] = nh.x, row[1] = nh.y, row[2] = nh.z;
  row[3] = A.x, row[4] = A.y, row[5] = A.z;
  row[6] = valid ? 1.0 : 0.0;
  row[7] = 0.0;
  a.scores[h] = valid ? 0u : kPlDropped;
}

// The hot path.  Workgroup (x, y) scores the points [1024 x, 1024 x + 1024) against the hypotheses [32 y, 32 y + 32).  Lane t holds the
// records 1024 x + 256 j + t, j = 0 .. 3, as doubles (a record beyond n is NaN: never an inlier); the 32 table rows are staged in LDS,
// where every lane reads the same address — a broadcast.  Per hypothesis and wave the inliers are four 64-bit ballots and their
// popcounts, added by the wave's first lane to the hypothesis' counter in LDS; at the end ONE global atomicAdd per hypothesis carries the
// workgroup's count to scores[h].  Integer sums: no order enters.  A dropped hypothesis is skipped by a branch on a value read through
// readfirstlane: uniform.
__global__ __launch_bounds__(kPlBlock) void plane_score_kernel(const PlaneArgs a) {
  __shared__ double hyp[kPlHypTile][kPlHypWords];
  __shared__ int live[kPlHypTile];
  __shared__ unsigned count[kPlHypTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const uint32_t h0 = blockIdx.y * static_cast<uint32_t>(kPlHypTile);
  const int nh = static_cast<int>(min(static_cast<uint32_t>(kPlHypTile), a.H - h0));  // >= 1: the grid has ceil(H / 32) rows
  {
    static_assert(kPlHypTile * kPlHypWords == kPlBlock, "one table word per lane");
    const int s = tid / kPlHypWords, w = tid % kPlHypWords;
    const double word = s < nh ? a.table[static_cast<size_t>(kPlHypWords) * (h0 + s) + w] : 0.0;
    hyp[s][w] = word;
    if (w == 6) live[s] = word != 0.0 ? 1 : 0;
  }
  if (tid < kPlHypTile) count[tid] = 0u;
  double x[kPlRows], y[kPlRows], z[kPlRows];
  const uint32_t first = blockIdx.x * static_cast<uint32_t>(kPlPointTile) + tid;  // < n + 1024 < 2^32
#pragma unroll
  for (int j = 0; j < kPlRows; j++) {
    const uint32_t i = first + static_cast<uint32_t>(kPlBlock * j);
    if (i < a.n) {
      const float4 p = a.pts[i];
      x[j] = p.x, y[j] = p.y, z[j] = p.z;
    } else {
      x[j] = y[j] = z[j] = static_cast<double>(NAN);
    }
  }
  __syncthreads();
  for (int s = 0; s < nh; s++) {
    if (__builtin_amdgcn_readfirstlane(live[s]) == 0) continue;
    const double nx = hyp[s][0], ny = hyp[s][1], nz = hyp[s][2], ax = hyp[s][3], ay = hyp[s][4], az = hyp[s][5];
    unsigned c = 0u;
#pragma unroll
    for (int j = 0; j < kPlRows; j++) c += static_cast<unsigned>(__popcll(__ballot(fabs(plane_dist(nx, ny, nz, ax, ay, az, x[j], y[j], z[j])) <= a.thr)));
    if (lane == 0 && c != 0u) atomicAdd(&count[s], c);
  }
  __syncthreads();
  if (tid < nh && count[tid] != 0u) atomicAdd(&a.scores[h0 + tid], count[tid]);  // (a dropped hypothesis counted nothing: its word stays)
}

// The best word over the scores and the number of hypotheses scored, by ONE workgroup: thread t takes h = t, t + 1024, ..., the threads
// meet in a tree of integer maxima and sums.  The scores leave for the host on the way, when they are asked for.
__global__ __launch_bounds__(kPlSelectThreads) void plane_select_kernel(const PlaneArgs a) {
  __shared__ unsigned long long sh_key[kPlSelectThreads];
  __shared__ uint32_t sh_cnt[kPlSelectThreads];
  const int tid = threadIdx.x;
  unsigned long long key = 0ull;
  uint32_t cnt = 0u;
  for (uint32_t h = tid; h < a.H; h += kPlSelectThreads) {
    const uint32_t s = a.scores[h];
    if (a.scores_host != nullptr) a.scores_host[h] = s;
    if (s == kPlDropped) continue;
    cnt++;
    const unsigned long long k = (static_cast<unsigned long long>(s) << 32) | (0xFFFFFFFFull - h);
    key = k > key ? k : key;
  }
  sh_key[tid] = key, sh_cnt[tid] = cnt;
  __syncthreads();
  for (int off = kPlSelectThreads / 2; off > 0; off >>= 1) {
    if (tid < off) {
      sh_key[tid] = sh_key[tid + off] > sh_key[tid] ? sh_key[tid + off] : sh_key[tid];
      sh_cnt[tid] += sh_cnt[tid + off];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.status[0] = sh_key[0], a.status[1] = sh_cnt[0];
    a.head_host[0] = sh_key[0], a.head_host[1] = sh_cnt[0];
  }
  __threadfence_system();
}

// Over the best hypothesis' inliers, x = r_i - a: the count, sum x, sum x x^T and the sum of squared distances, in double.  Workgroup g
// of G: plane_for_points' order, plane_block_tree's tree, the totals in slot g of the staging slot; the host adds the slots in order.
__global__ __launch_bounds__(kPlBlock) void plane_sums_kernel(const PlaneArgs a) {
  __shared__ double sh[kPlSums][kPlBlock];
  const unsigned long long best = a.status[0];
  if (best == 0ull) return;  // nothing scored (uniform): the host reads the head alone
  const uint32_t h = static_cast<uint32_t>(0xFFFFFFFFull - (best & 0xFFFFFFFFull));
  const double* row = a.table + static_cast<size_t>(kPlHypWords) * h;
  const double nx = row[0], ny = row[1], nz = row[2], ax = row[3], ay = row[4], az = row[5];
  double acc[kPlSums];
#pragma unroll
  for (int c = 0; c < kPlSums; c++) acc[c] = 0.0;
  plane_for_points(a, [&](uint32_t, const float4 p) {
    const double d = plane_dist(nx, ny, nz, ax, ay, az, p.x, p.y, p.z);
    if (!(fabs(d) <= a.thr)) return;
    const double x = static_cast<double>(p.x) - ax, y = static_cast<double>(p.y) - ay, z = static_cast<double>(p.z) - az;
    acc[0] += 1.0;
    acc[1] += x, acc[2] += y, acc[3] += z;
    acc[4] += x * x, acc[5] += x * y, acc[6] += x * z, acc[7] += y * y, acc[8] += y * z, acc[9] += z * z;
    acc[10] += d * d;
  });
  plane_block_tree<kPlSums>(sh, acc);
  if (threadIdx.x < kPlSums) a.sums_host[static_cast<size_t>(kPlSums) * blockIdx.x + threadIdx.x] = sh[threadIdx.x][0];
  if (blockIdx.x == 0 && threadIdx.x < 6) reinterpret_cast<double*>(a.head_host)[2 + threadIdx.x] = row[threadIdx.x];
  __threadfence_system();
}

// The final plane (fn about fa): the flag of every point for the compaction, the final inliers' count and their sum of squared
// distances, in the order of the sums kernel.
__global__ __launch_bounds__(kPlBlock) void plane_flags_kernel(const PlaneArgs a) {
  __shared__ double sh[2][kPlBlock];
  double acc[2] = {0.0, 0.0};
  plane_for_points(a, [&](uint32_t i, const float4 p) {
    const double d = plane_dist(a.fn[0], a.fn[1], a.fn[2], a.fa[0], a.fa[1], a.fa[2], p.x, p.y, p.z);
    const bool in = fabs(d) <= a.thr;
    if (a.flag != nullptr) a.flag[i] = in == (a.keep == 1) ? 0.0 : 1.0;
    if (in) acc[0] += 1.0, acc[1] += d * d;
  });
  plane_block_tree<2>(sh, acc);
  if (threadIdx.x < 2) a.final_host[2 * static_cast<size_t>(blockIdx.x) + threadIdx.x] = sh[threadIdx.x][0];
  __threadfence_system();
}

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

// what sga_cloud_segment_plane refuses of its arguments (no handle is read)
int plane_check(const sga_plane_params& p, const int64_t* kept, sga_cloud* const* out) {
  if (p.keep < 0 || p.keep > 2) return fail(SGA_ERR_INVALID, "segment_plane: keep %d is not 0 (no cloud), 1 (the plane's points) or 2 (the rest)", p.keep);
  if (p.keep == 0 && out != nullptr) return fail(SGA_ERR_INVALID, "segment_plane: keep is 0 but an output cloud is asked for");
  if (p.keep != 0 && out == nullptr) return fail(SGA_ERR_INVALID, "segment_plane: keep is %d but there is no place for the output cloud", p.keep);
  if (p.keep == 0 && kept != nullptr) return fail(SGA_ERR_INVALID, "segment_plane: kept is given but keep is 0");
  if (!(is_finite(p.distance_threshold) && p.distance_threshold > 0.0)) return fail(SGA_ERR_INVALID, "segment_plane: distance_threshold must be finite and > 0");
  if (p.iterations < 1 || p.iterations > kPlMaxIterations) return fail(SGA_ERR_INVALID, "segment_plane: iterations must be in [1, 2^20]");
  bool axis = false;
  for (int k = 0; k < 3; k++) {
    if (!is_finite(p.axis[k])) return fail(SGA_ERR_INVALID, "segment_plane: axis has a non-finite entry");
    axis = axis || p.axis[k] != 0.0;
  }
  if (!(p.max_angle >= 0.0 && p.max_angle <= 1.5707963267948966)) return fail(SGA_ERR_INVALID, "segment_plane: max_angle must be in [0, pi/2]");
  if (axis && !(p.max_angle > 0.0)) return fail(SGA_ERR_INVALID, "segment_plane: an axis needs a max_angle in (0, pi/2]");
  if (p.min_inliers < 3) return fail(SGA_ERR_INVALID, "segment_plane: min_inliers %llu is below 3", static_cast<unsigned long long>(p.min_inliers));
  if (p.refit != 0 && p.refit != 1) return fail(SGA_ERR_INVALID, "segment_plane: refit %d is not 0 or 1", p.refit);
  return SGA_OK;
}

// The refit's host arithmetic (small_gicp_amd_debug.h: sga_debug_plane_from_sums states it)
bool plane_from_sums(uint64_t k, const double sx[3], const double sxx[6], double normal[3], double offset[3], double values[3]) {
  if (k < 1) return false;
  for (int c = 0; c < 3; c++)
    if (!is_finite(sx[c])) return false;
  for (int c = 0; c < 6; c++)
    if (!is_finite(sxx[c])) return false;
  const double kd = static_cast<double>(k);
  for (int c = 0; c < 3; c++) offset[c] = sx[c] / kd;
  const double S[6] = {sxx[0] - sx[0] * sx[0] / kd, sxx[1] - sx[0] * sx[1] / kd, sxx[2] - sx[0] * sx[2] / kd, sxx[3] - sx[1] * sx[1] / kd, sxx[4] - sx[1] * sx[2] / kd, sxx[5] - sx[2] * sx[2] / kd};
  double vec[3][3];
  sym3_eigen(S, values, vec);
  if (k < 3) return false;
  if (!(values[1] - values[0] > 1e-12 * values[2])) return false;
  Vec3 n{vec[0][0], vec[0][1], vec[0][2]};
  if (!(norm3(n) > 0.0)) return false;
  (void)plane_orient(n, 0, 0.0, 0.0, 0.0, 1.0, 0.0);
  normal[0] = n.x, normal[1] = n.y, normal[2] = n.z;
  return true;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_plane_default(sga_plane_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->distance_threshold = 0.1;
  p->iterations = 1000;
  p->min_inliers = 3;
  p->refit = 1;
}

int sga_cloud_segment_plane(sga_context* ctx, const sga_cloud* cloud, const sga_plane_params* params, double plane[4], uint32_t* scores, int64_t* kept, sga_cloud** out, sga_plane_result* result) {
  if (out) *out = nullptr;
  if (!ctx || !cloud || !params || !plane || !result) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(plane_check(*params, kept, out));
  // ---- (from here on the handles are read)
  std::memset(result, 0, sizeof(*result));
  for (int k = 0; k < 4; k++) plane[k] = 0.0;
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", n);
  const size_t H = static_cast<size_t>(params->iterations);
  SGA_ENTER(ctx);
  // no plane: an empty cloud (keep 1), or every record through the compaction (keep 2)
  auto no_plane = [&]() -> int {
    if (!out) return SGA_OK;
    if (params->keep == 1 || n == 0) {
      std::unique_ptr<sga_cloud> none;
      SGA_TRY(cloud_make_like(ctx, cloud, 0, &none));
      *out = none.release();
      return SGA_OK;
    }
    CropStat all{nullptr, nullptr, 0.5, Chain::Plane, true};
    count_launch(Chain::PlaneWait);
    return cloud_crop_stat(ctx, cloud, all, kept, out);
  };
  if (n < 3) {  // no triple: every hypothesis is dropped, nothing of this file is launched
    for (size_t h = 0; scores != nullptr && h < H; h++) scores[h] = kPlDropped;
    return no_plane();
  }
  SGA_TRY(wait_ready(ctx, cloud->ready));
  DevBuf<double> table, flag;  // all live to the end of the call (then: the stream's free list)
  DevBuf<uint32_t> dscores;
  DevBuf<unsigned long long> status;
  SGA_TRY(table.alloc(static_cast<size_t>(kPlHypWords) * H));
  SGA_TRY(dscores.alloc(H));
  SGA_TRY(status.alloc(2));
  if (out) SGA_TRY(flag.alloc(n));
  const uint32_t G = static_cast<uint32_t>(std::min<size_t>(kPlMaxGroups, (n + 1023) / 1024));
  // the head, the partial sums of both kernels and the scores leave through ONE slot of the staging ring, which the kernels write by its device address
  const size_t sums_bytes = static_cast<size_t>(G) * kPlSums * sizeof(double), final_bytes = static_cast<size_t>(G) * 2 * sizeof(double);
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, kPlHeadBytes + sums_bytes + final_bytes + (scores != nullptr ? H * sizeof(uint32_t) : 0), &slot));
  char* slot_dev = static_cast<char*>(slot->dev);
  PlaneArgs a;
  std::memset(&a, 0, sizeof(a));
  a.pts = cloud->pts.p;
  a.n = static_cast<uint32_t>(n), a.H = static_cast<uint32_t>(H);
  a.seed = params->seed;
  a.thr = params->distance_threshold;
  a.ax = params->axis[0], a.ay = params->axis[1], a.az = params->axis[2];
  a.has_axis = a.ax != 0.0 || a.ay != 0.0 || a.az != 0.0 ? 1 : 0;
  a.axis_norm = a.has_axis ? norm3(Vec3{a.ax, a.ay, a.az}) : 1.0;
  a.cos_max = std::cos(params->max_angle);
  a.keep = params->keep;
  a.table = table.p, a.scores = dscores.p, a.status = status.p;
  a.head_host = reinterpret_cast<unsigned long long*>(slot_dev);
  a.sums_host = reinterpret_cast<double*>(slot_dev + kPlHeadBytes);
  a.final_host = reinterpret_cast<double*>(slot_dev + kPlHeadBytes + sums_bytes);
  a.scores_host = scores != nullptr ? reinterpret_cast<uint32_t*>(slot_dev + kPlHeadBytes + sums_bytes + final_bytes) : nullptr;
  a.flag = flag.p;
  a.G = G;
  count_launch(Chain::Plane);
  hipLaunchKernelGGL(plane_hypotheses_kernel, dim3(static_cast<unsigned>((H + kPlBlock - 1) / kPlBlock)), dim3(kPlBlock), 0, ctx->stream, a);
  count_launch(Chain::Plane);
  hipLaunchKernelGGL(plane_score_kernel, dim3(static_cast<unsigned>((n + kPlPointTile - 1) / kPlPointTile), static_cast<unsigned>((H + kPlHypTile - 1) / kPlHypTile)), dim3(kPlBlock), 0, ctx->stream, a);
  count_launch(Chain::Plane);
  hipLaunchKernelGGL(plane_select_kernel, dim3(1), dim3(kPlSelectThreads), 0, ctx->stream, a);
  count_launch(Chain::Plane);
  hipLaunchKernelGGL(plane_sums_kernel, dim3(G), dim3(kPlBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::PlaneWait);
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the first wait: the best word and the sums are in the slot
  const char* host = static_cast<const char*>(slot->host);
  const unsigned long long best = reinterpret_cast<const unsigned long long*>(host)[0];
  result->scored = reinterpret_cast<const unsigned long long*>(host)[1];
  if (scores) std::memcpy(scores, host + kPlHeadBytes + sums_bytes + final_bytes, H * sizeof(uint32_t));
  if (best == 0ull) return no_plane();  // every hypothesis was dropped
  result->best_hypothesis = 0xFFFFFFFFull - (best & 0xFFFFFFFFull);
  result->hypothesis_inliers = best >> 32;
  if (result->hypothesis_inliers < params->min_inliers) return no_plane();
  const double* head = reinterpret_cast<const double*>(host) + 2;  // nhat, a
  double sums[kPlSums];
  for (int c = 0; c < kPlSums; c++) sums[c] = 0.0;
  for (uint32_t g = 0; g < G; g++)
    for (int c = 0; c < kPlSums; c++) sums[c] += reinterpret_cast<const double*>(host + kPlHeadBytes)[static_cast<size_t>(kPlSums) * g + c];
  double count = sums[0], ssq = sums[10];
  for (int c = 0; c < 3; c++) a.fn[c] = head[c], a.fa[c] = head[3 + c];
  // the eigen-solve stays on the host: a wait costs about 10 us against the 10^8 point-plane tests before it, and a 3x3 Jacobi iteration
  // on the device would be one lane's work all the same
  if (params->refit != 0) {
    double normal[3], offset[3], values[3];
    if (plane_from_sums(static_cast<uint64_t>(count), sums + 1, sums + 4, normal, offset, values)) {
      Vec3 nf{normal[0], normal[1], normal[2]};
      if (plane_orient(nf, a.has_axis, a.ax, a.ay, a.az, a.axis_norm, a.cos_max)) {
        a.fn[0] = nf.x, a.fn[1] = nf.y, a.fn[2] = nf.z;
        for (int c = 0; c < 3; c++) a.fa[c] = head[3 + c] + offset[c];
        result->refit = 1;
      }
    }
  }
  sga_cloud* made = nullptr;
  if (result->refit != 0 || out) {  // the final inliers: of another plane, or wanted as flags
    count_launch(Chain::Plane);
    hipLaunchKernelGGL(plane_flags_kernel, dim3(G), dim3(kPlBlock), 0, ctx->stream, a);
    SGA_HIP(hipGetLastError());
    count_launch(Chain::PlaneWait);
    if (out) {
      CropStat cs{a.flag, nullptr, 0.5, Chain::Plane, true};
      SGA_TRY(cloud_crop_stat(ctx, cloud, cs, kept, &made));  // (its wait shows that everything above has run)
    } else {
      SGA_HIP(hipStreamSynchronize(ctx->stream));  // the second wait
    }
    count = ssq = 0.0;
    const double* fin = reinterpret_cast<const double*>(host + kPlHeadBytes + sums_bytes);
    for (uint32_t g = 0; g < G; g++) count += fin[2 * g], ssq += fin[2 * g + 1];
  }
  result->inliers = static_cast<uint64_t>(count);
  result->rmse = count > 0.0 ? std::sqrt(ssq / count) : 0.0;
  for (int c = 0; c < 3; c++) plane[c] = a.fn[c];
  plane[3] = -((a.fn[0] * (a.fa[0] + cloud->origin[0]) + a.fn[1] * (a.fa[1] + cloud->origin[1])) + a.fn[2] * (a.fa[2] + cloud->origin[2]));
  if (out) *out = made;
  return SGA_OK;
}

int sga_debug_segment_plane_launches(unsigned long long* launches) { return report_launches(Chain::Plane, launches); }
int sga_debug_segment_plane_waits(unsigned long long* waits) { return report_launches(Chain::PlaneWait, waits); }

int sga_debug_plane_from_sums(uint64_t k, const double sum_x[3], const double sum_xx6[6], double normal[3], double centroid_offset[3], double eigenvalues[3]) {
  if (!sum_x || !sum_xx6 || !normal || !centroid_offset || !eigenvalues) return 0;
  return plane_from_sums(k, sum_x, sum_xx6, normal, centroid_offset, eigenvalues) ? 1 : 0;
}

}  // extern "C"

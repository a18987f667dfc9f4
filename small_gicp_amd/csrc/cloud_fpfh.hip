// FPFH descriptors on the device: sga_cloud_fpfh and the sga_features handle.  Three launches: the neighbour
// lists (the exact k-NN of the cloud's own kd-tree, on the two routes of cloud_outliers.hip), the SPFH counts (integer atomics in LDS),
// the FPFH rows (a lane per bin, the weighted sum in the list's order).  Everything in double from the fp32 records; no floating-point
// atomics: two calls give the same bytes.
#include "cloud_ops.hpp"
#include "device_io.hpp"
#include "forest.hpp"
#include "knn_wave.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kFpBlock = 64;      // lane route: queries of a workgroup (one wave)
constexpr int kFpWindow = 128;    // ... and the kd positions around them that are scanned before the walk
constexpr int kFpMaxK = 63;       // the point and its k neighbours fill the 64 lanes of the wave route
constexpr int kFpDim = SGA_FPFH_DIM;
constexpr int kFpWaves = 4;       // points of a workgroup of the SPFH and FPFH kernels: one wave each
constexpr double kFpPi = 3.14159265358979323846;

struct FpfhArgs {
  KdView g;             // the tree over the cloud
  const float4* pts;    // the cloud's records and normals, its order
  const float4* nrm;
  uint32_t* nbr;        // n x kp original indices: the neighbours of point i (the cloud's order) at nbr[i * kp ..]
  double* spfh;         // n x 33
  float* rows;          // n x 33
  double vp[3];         // viewpoint - origin (the records' frame)
  uint32_t n;
  int k, kp;            // kp = min(k, n - 1) >= 1
  int has_vp;
};

__device__ __forceinline__ uint32_t fp_orig(const float4 p) { return __float_as_uint(p.w); }

struct FpNormal {
  double x, y, z;
};
// the normal of a record as the definition uses it: as stored, or negated where it points away from the viewpoint
__device__ __forceinline__ FpNormal fp_normal(const FpfhArgs& a, const float4 p, const float4 nn) {
  FpNormal r{static_cast<double>(nn.x), static_cast<double>(nn.y), static_cast<double>(nn.z)};
  if (a.has_vp) {
    const double s = r.x * (a.vp[0] - static_cast<double>(p.x)) + r.y * (a.vp[1] - static_cast<double>(p.y)) + r.z * (a.vp[2] - static_cast<double>(p.z));
    if (s < 0.0) r.x = -r.x, r.y = -r.y, r.z = -r.z;
  }
  return r;
}

__device__ __forceinline__ int fp_bin(double x) {  // 11 x, floored and clamped to 0 .. 10
  const int b = static_cast<int>(floor(x));
  return b < 0 ? 0 : (b > 10 ? 10 : b);
}

}  // namespace

// The neighbour list of every point: its kp nearest OTHER records, in the search's order, as original indices.  The search asks for
// k + 1 entries (the point itself is one of them at distance 0); the first entry that IS the query is left out — when coincident
// records pushed the query itself out of the list, the last entry is.
//   ROUTE 0 — one wave per query (knn_wave.hpp): lane j holds the j-th nearest.
//   ROUTE 1 — one lane per query: kd_knn with its list in LDS, unsorted, as outlier_stat_kernel<1> calls it.
template <int ROUTE>
__global__ __launch_bounds__(kFpBlock) void fpfh_neighbours_kernel(const FpfhArgs a) {
  const int lane = threadIdx.x;
  const int kp = a.kp;
  if constexpr (ROUTE == 0) {
    __shared__ uint32_t stack[2 * kKdMaxDepth + 2];
    const uint32_t i = blockIdx.x;  // < n: the grid is n workgroups
    float bd;
    int bid;
    knn_wave_query(a.g, i, a.k + 1, lane, stack, bd, bid);
    const unsigned long long self = __ballot(bid == static_cast<int>(i));
    const int self_lane = self != 0ull ? __ffsll(static_cast<long long>(self)) - 1 : kp;
    const int slot = lane - (lane > self_lane ? 1 : 0);
    if (lane != self_lane && lane <= kp && bid >= 0 && slot < kp) {
      const size_t row = static_cast<size_t>(fp_orig(a.g.pts[i])) * kp;
      a.nbr[row + slot] = fp_orig(a.g.pts[bid]);
    }
  } else {
    extern __shared__ float sh[];
    __shared__ float4 window[kFpWindow];
    const int kk = a.k + 1;
    const int kpad = (kk + 3) & ~3;  // kd_knn sweeps the list four slots at a time
    float* sd = sh;
    int* si = reinterpret_cast<int*>(sh + static_cast<size_t>(kpad) * kFpBlock);
    uint32_t* stack = reinterpret_cast<uint32_t*>(sh + 2 * static_cast<size_t>(kpad) * kFpBlock);
    const uint32_t base = blockIdx.x * kFpBlock;
    const uint32_t i = base + lane;
    for (int j = 0; j < kpad; j++) {
      sd[j * kFpBlock + lane] = INFINITY;
      si[j * kFpBlock + lane] = -1;
    }
    const uint32_t pre_first = base > (kFpWindow - kFpBlock) / 2 ? base - (kFpWindow - kFpBlock) / 2 : 0u;
    const uint32_t pre_end = min(pre_first + kFpWindow, a.n);
    for (uint32_t w = lane; w < pre_end - pre_first; w += kFpBlock) window[w] = a.g.pts[pre_first + w];
    __syncthreads();
    if (i >= a.n) return;
    const float4 p = a.g.pts[i];
    kd_knn<kFpBlock>(a.g, p.x, p.y, p.z, kk, INFINITY, sd, si, stack, lane, false, pre_first, pre_end, window, base, base + kFpBlock);
    const size_t row = static_cast<size_t>(fp_orig(p)) * kp;
    int w = 0;
    bool skipped = false;
    for (int j = 0; j < kk && w < kp; j++) {
      const int id = si[j * kFpBlock + lane];
      if (id < 0) continue;
      if (!skipped && id == static_cast<int>(i)) {
        skipped = true;
        continue;
      }
      a.nbr[row + w++] = fp_orig(a.g.pts[id]);
    }
  }
}

// SPFH_i: one wave per point, lane j takes the pair (i, j-th neighbour) and adds one to three bins of the point's counts in LDS (integer
// atomics); lanes 0 .. 32 then write the counts scaled by 100 / (pairs counted).
__global__ __launch_bounds__(kFpWaves * 64) void fpfh_spfh_kernel(const FpfhArgs a) {
  __shared__ unsigned hist[kFpWaves][kFpDim + 1];  // [33] = the pairs counted
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * kFpWaves + wv;
  if (lane <= kFpDim) hist[wv][lane] = 0u;
  __syncthreads();
  if (i < a.n && lane < a.kp) {
    const uint32_t j = min(a.nbr[static_cast<size_t>(i) * a.kp + lane], a.n - 1u);  // (every slot was written; the bound keeps a broken list inside the cloud)
    const float4 pi = a.pts[i], pj = a.pts[j];
    const FpNormal ni = fp_normal(a, pi, a.nrm[i]), nj = fp_normal(a, pj, a.nrm[j]);
    double dx = static_cast<double>(pj.x) - static_cast<double>(pi.x), dy = static_cast<double>(pj.y) - static_cast<double>(pi.y), dz = static_cast<double>(pj.z) - static_cast<double>(pi.z);
    const double len = sqrt(dx * dx + dy * dy + dz * dz);
    if (len > 0.0) {
      const double a1 = (ni.x * dx + ni.y * dy + ni.z * dz) / len, a2 = (nj.x * dx + nj.y * dy + nj.z * dz) / len;
      FpNormal n1 = ni, n2 = nj;
      double phi = a1;
      if (fabs(a1) < fabs(a2)) {
        n1 = nj, n2 = ni;
        dx = -dx, dy = -dy, dz = -dz;
        phi = -a2;
      }
      const double ux = dx / len, uy = dy / len, uz = dz / len;
      double vx = uy * n1.z - uz * n1.y, vy = uz * n1.x - ux * n1.z, vz = ux * n1.y - uy * n1.x;
      const double vn = sqrt(vx * vx + vy * vy + vz * vz);
      if (vn > 0.0) {
        vx /= vn, vy /= vn, vz /= vn;
        const double wx = n1.y * vz - n1.z * vy, wy = n1.z * vx - n1.x * vz, wz = n1.x * vy - n1.y * vx;
        const double alpha = vx * n2.x + vy * n2.y + vz * n2.z;
        const double theta = atan2(wx * n2.x + wy * n2.y + wz * n2.z, n1.x * n2.x + n1.y * n2.y + n1.z * n2.z);
        atomicAdd(&hist[wv][fp_bin(11.0 * (theta + kFpPi) / (2.0 * kFpPi))], 1u);
        atomicAdd(&hist[wv][11 + fp_bin(11.0 * (alpha + 1.0) / 2.0)], 1u);
        atomicAdd(&hist[wv][22 + fp_bin(11.0 * (phi + 1.0) / 2.0)], 1u);
        atomicAdd(&hist[wv][kFpDim], 1u);
      }
    }
  }
  __syncthreads();
  if (i < a.n && lane < kFpDim) {
    const unsigned c = hist[wv][kFpDim];
    a.spfh[static_cast<size_t>(i) * kFpDim + lane] = c > 0u ? static_cast<double>(hist[wv][lane]) * (100.0 / static_cast<double>(c)) : 0.0;
  }
}

// FPFH_i: one wave per point.  Lane j forms w_ij of the j-th neighbour; then lane b < 33 adds w_ij SPFH_j[b] over the list in its order
// (the 33 values of a neighbour are one coalesced load), the three sub-histograms are rescaled to 100 by sums every lane of a
// sub-histogram takes in the same order, and the row is rounded once to fp32.
__global__ __launch_bounds__(kFpWaves * 64) void fpfh_rows_kernel(const FpfhArgs a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t i = blockIdx.x * kFpWaves + wv;
  if (i >= a.n) return;  // (wave-uniform)
  uint32_t nb = 0u;
  double w = 0.0;
  if (lane < a.kp) {
    nb = min(a.nbr[static_cast<size_t>(i) * a.kp + lane], a.n - 1u);
    const float4 pi = a.pts[i], pj = a.pts[nb];
    const double dx = static_cast<double>(pj.x) - static_cast<double>(pi.x), dy = static_cast<double>(pj.y) - static_cast<double>(pi.y), dz = static_cast<double>(pj.z) - static_cast<double>(pi.z);
    const double d2 = dx * dx + dy * dy + dz * dz;
    w = d2 > 0.0 ? 1.0 / d2 : 0.0;
  }
  const int b = lane < kFpDim ? lane : 0;
  double acc = 0.0;
  for (int j = 0; j < a.kp; j++) {
    const double wj = __shfl(w, j);
    const uint32_t nj = __shfl(nb, j);
    acc += wj * a.spfh[static_cast<size_t>(nj) * kFpDim + b];
  }
  double v = a.spfh[static_cast<size_t>(i) * kFpDim + b] + acc / static_cast<double>(a.kp);
  const int first = 11 * min(lane / 11, 2);
  double total = 0.0;
#pragma unroll
  for (int t = 0; t < 11; t++) total += __shfl(v, first + t);
  if (total != 0.0) v *= 100.0 / total;
  if (lane < kFpDim) a.rows[static_cast<size_t>(i) * kFpDim + lane] = static_cast<float>(v);
}

// sga_features_select: value t of the output is value t % dim of row idx[t / dim] (a thread per value: the loads of a row are coalesced)
__global__ __launch_bounds__(256) void features_gather_kernel(const float* __restrict__ rows, const uint32_t* __restrict__ idx, uint32_t dim, unsigned long long total, float* __restrict__ out) {
  const unsigned long long t = blockIdx.x * 256ull + threadIdx.x;
  if (t >= total) return;
  const unsigned long long j = t / dim;
  out[t] = rows[static_cast<unsigned long long>(idx[j]) * dim + (t - j * dim)];
}

// sga_features_create_device / sga_features_export_device: value t of the handle's rows (row t / dim, column t % dim) from or to a caller's
// strided array of floats or doubles (a double is rounded to fp32 once; a float becomes the double it is)
template <typename T, bool kExport>
__global__ __launch_bounds__(256) void features_rows_kernel(float* __restrict__ rows, T* __restrict__ user, uint32_t dim, uint32_t stride, unsigned long long total) {
  const unsigned long long t = blockIdx.x * 256ull + threadIdx.x;
  if (t >= total) return;
  const unsigned long long j = t / dim;
  const unsigned long long u = j * stride + (t - j * dim);
  if constexpr (kExport) user[u] = static_cast<T>(rows[t]);
  else rows[t] = static_cast<float>(user[u]);
}

namespace {

struct IndexDestroy {
  void operator()(sga_index* i) const { (void)sga_index_destroy(i); }
};

int features_new(const sga_context* ctx, size_t n, int dim, std::unique_ptr<sga_features>* out) {
  std::unique_ptr<sga_features> f(new sga_features());
  f->device = ctx->device;
  f->n = n;
  f->dim = dim;
  SGA_TRY(f->rows.alloc(n * static_cast<size_t>(dim)));
  *out = std::move(f);
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

int sga_features_create(sga_context* ctx, const float* rows, size_t n, int dim, sga_features** out) {
  if (out) *out = nullptr;
  if (!ctx || !out || (n > 0 && !rows)) return fail(SGA_ERR_INVALID, "null argument");
  if (dim < 1 || dim > 128) return fail(SGA_ERR_INVALID, "features: dim must be in [1,128], got %d", dim);
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many rows (%zu; limit 2^31-1)", n);
  SGA_ENTER(ctx);
  std::unique_ptr<sga_features> f;
  SGA_TRY(features_new(ctx, n, dim, &f));
  if (n > 0) {  // through a slot of the staging ring: the caller's array is free when the call returns
    const size_t bytes = n * static_cast<size_t>(dim) * sizeof(float);
    sga_context::StageSlot* slot = nullptr;
    SGA_TRY(stage_acquire(ctx, bytes, &slot));
    std::memcpy(slot->host, rows, bytes);
    SGA_HIP(hipMemcpyAsync(f->rows.p, slot->host, bytes, hipMemcpyHostToDevice, ctx->stream));
    SGA_TRY(stage_release(ctx, slot));
    SGA_TRY(mark_ready(ctx, f->ready));
  }
  *out = f.release();
  return SGA_OK;
}

// the caller's array `a` of n rows against its allocation: the last row ends with its last column (a view of a wider array)
static int features_array_check(sga_context* ctx, const sga_device_array* a, size_t n, const char* host_entry) {
  const size_t elem = a->dtype == SGA_F64 ? 8 : 4;
  size_t span = 0;
  if (__builtin_mul_overflow(n - 1, static_cast<size_t>(a->stride) * elem, &span) || __builtin_add_overflow(span, static_cast<size_t>(a->cols) * elem, &span))
    return fail(SGA_ERR_INVALID, "rows: %zu rows of stride %d overflow the address space", n, a->stride);
  return check_device_range(ctx, a->data, span, elem, "rows", host_entry);
}
static int features_array_layout(const sga_device_array* a) {
  if (a->dtype != SGA_F32 && a->dtype != SGA_F64) return fail(SGA_ERR_INVALID, "rows: dtype %d is neither SGA_F32 nor SGA_F64", a->dtype);
  if (a->cols < 1 || a->cols > 128) return fail(SGA_ERR_INVALID, "features: dim must be in [1,128], got %d", a->cols);
  if (a->stride < a->cols) return fail(SGA_ERR_INVALID, "rows: stride %d < cols %d", a->stride, a->cols);
  return SGA_OK;
}

int sga_features_create_device(sga_context* ctx, const sga_device_array* rows, size_t n, void* user_stream, int flags, sga_features** out) {
  if (out) *out = nullptr;
  if (!ctx || !out || !rows) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(features_array_layout(rows));
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many rows (%zu; limit 2^31-1)", n);
  SGA_ENTER(ctx);
  if (n > 0) SGA_TRY(features_array_check(ctx, rows, n, "sga_features_create"));
  std::unique_ptr<sga_features> f;
  SGA_TRY(features_new(ctx, n, rows->cols, &f));
  if (n > 0) {
    IoOrder ord;
    SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
    const unsigned long long total = static_cast<unsigned long long>(n) * static_cast<unsigned long long>(rows->cols);
    const dim3 grid(static_cast<unsigned>((total + 255) / 256)), block(256);
    if (rows->dtype == SGA_F64)
      hipLaunchKernelGGL((features_rows_kernel<const double, false>), grid, block, 0, ctx->stream, f->rows.p, static_cast<const double*>(rows->data), static_cast<uint32_t>(rows->cols), static_cast<uint32_t>(rows->stride), total);
    else
      hipLaunchKernelGGL((features_rows_kernel<const float, false>), grid, block, 0, ctx->stream, f->rows.p, static_cast<const float*>(rows->data), static_cast<uint32_t>(rows->cols), static_cast<uint32_t>(rows->stride), total);
    SGA_HIP(hipGetLastError());
    SGA_TRY(io_end(ctx, ord));
    SGA_TRY(mark_ready(ctx, f->ready));
  }
  *out = f.release();
  return SGA_OK;
}

int sga_features_export_device(sga_context* ctx, const sga_features* features, const sga_device_array* rows, void* user_stream, int flags) {
  if (!ctx || !features || !rows) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(features_array_layout(rows));
  if (features->device != ctx->device) return fail(SGA_ERR_INVALID, "features live on another device");
  if (rows->cols != features->dim) return fail(SGA_ERR_INVALID, "rows: cols = %d, the features have dim %d", rows->cols, features->dim);
  if (features->n == 0) return SGA_OK;
  SGA_ENTER(ctx);
  SGA_TRY(features_array_check(ctx, rows, features->n, "sga_features_download"));
  SGA_TRY(wait_ready(ctx, features->ready));
  IoOrder ord;
  SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  const unsigned long long total = static_cast<unsigned long long>(features->n) * static_cast<unsigned long long>(features->dim);
  const dim3 grid(static_cast<unsigned>((total + 255) / 256)), block(256);
  void* data = const_cast<void*>(rows->data);  // (sga_device_array: written through by the export calls)
  if (rows->dtype == SGA_F64)
    hipLaunchKernelGGL((features_rows_kernel<double, true>), grid, block, 0, ctx->stream, features->rows.p, static_cast<double*>(data), static_cast<uint32_t>(rows->cols), static_cast<uint32_t>(rows->stride), total);
  else
    hipLaunchKernelGGL((features_rows_kernel<float, true>), grid, block, 0, ctx->stream, features->rows.p, static_cast<float*>(data), static_cast<uint32_t>(rows->cols), static_cast<uint32_t>(rows->stride), total);
  SGA_HIP(hipGetLastError());
  return io_end(ctx, ord);
}

int sga_features_size(const sga_features* features, size_t* n, int* dim) {
  if (!features) return fail(SGA_ERR_INVALID, "null argument");
  if (n) *n = features->n;
  if (dim) *dim = features->dim;
  return SGA_OK;
}

int sga_features_download(sga_context* ctx, const sga_features* features, float* rows) {
  if (!ctx || !features || (features->n > 0 && !rows)) return fail(SGA_ERR_INVALID, "null argument");
  if (features->device != ctx->device) return fail(SGA_ERR_INVALID, "features live on another device");
  if (features->n == 0) return SGA_OK;
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, features->ready));
  SGA_HIP(hipMemcpyAsync(rows, features->rows.p, features->n * static_cast<size_t>(features->dim) * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

int sga_features_destroy(sga_features* features) {
  delete features;
  return SGA_OK;
}

int sga_features_select(sga_context* ctx, const sga_features* features, const int64_t* indices, size_t m, sga_features** out) {
  if (out) *out = nullptr;
  if (!ctx || !features || !out || (m > 0 && !indices)) return fail(SGA_ERR_INVALID, "null argument");
  if (m >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many indices (%zu; limit 2^31-1)", m);
  if (features->device != ctx->device) return fail(SGA_ERR_INVALID, "features live on another device");
  for (size_t j = 0; j < m; j++)
    if (indices[j] < 0 || static_cast<unsigned long long>(indices[j]) >= features->n) return fail(SGA_ERR_INVALID, "indices[%zu] = %lld is outside the %zu rows", j, static_cast<long long>(indices[j]), features->n);
  SGA_ENTER(ctx);
  std::unique_ptr<sga_features> f;
  SGA_TRY(features_new(ctx, m, features->dim, &f));
  if (m > 0) {  // the indices go through a slot of the staging ring, which is reused only behind the kernel: no host wait
    SGA_TRY(wait_ready(ctx, features->ready));
    sga_context::StageSlot* slot = nullptr;
    SGA_TRY(stage_acquire(ctx, m * sizeof(uint32_t), &slot));
    uint32_t* host = static_cast<uint32_t*>(slot->host);
    for (size_t j = 0; j < m; j++) host[j] = static_cast<uint32_t>(indices[j]);
    const unsigned long long total = static_cast<unsigned long long>(m) * static_cast<unsigned long long>(features->dim);
    hipLaunchKernelGGL(features_gather_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), dim3(256), 0, ctx->stream, features->rows.p, static_cast<const uint32_t*>(slot->dev), static_cast<uint32_t>(features->dim), total,
                       f->rows.p);
    SGA_HIP(hipGetLastError());
    SGA_TRY(stage_release(ctx, slot));
    SGA_TRY(mark_ready(ctx, f->ready));
    if (!ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));  // a blocking context reports what its kernel met
  }
  *out = f.release();
  return SGA_OK;
}

int sga_cloud_fpfh(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree, int k, const double viewpoint[3], sga_features** out) {
  if (out) *out = nullptr;
  if (!ctx || !cloud || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (k < 2 || k > kFpMaxK) return fail(SGA_ERR_INVALID, "fpfh: k must be in [2,%d] (the point and its k neighbours fill the 64 lanes of a wave)", kFpMaxK);
  for (int a = 0; viewpoint != nullptr && a < 3; a++)
    if (!(viewpoint[a] - viewpoint[a] == 0.0)) return fail(SGA_ERR_INVALID, "fpfh: the viewpoint has a non-finite entry");
  // ---- (from here on the handles are read)
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (kdtree) {  // checked as sga_cloud_remove_outliers checks it
    if (kdtree->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "fpfh needs a kd-tree index, not a projective search");
    if (kdtree->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_INVALID, "a kd-tree index is required");
    if (kdtree->n != n) return fail(SGA_ERR_INVALID, "index was built over a cloud of %zu points, got %zu", kdtree->n, n);
    for (int a = 0; a < 3; a++)
      if (kdtree->origin[a] != cloud->origin[a]) return fail(SGA_ERR_INVALID, "the index was not built over this cloud (their device frames differ)");
  }
  if (n > 0 && !cloud->has_normals) return fail(SGA_ERR_INVALID, "fpfh needs a cloud with normals");
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", n);
  SGA_ENTER(ctx);
  std::unique_ptr<sga_features> f;
  SGA_TRY(features_new(ctx, n, kFpDim, &f));
  if (n == 0) {  // an empty handle; nothing is launched
    *out = f.release();
    return SGA_OK;
  }
  std::unique_ptr<sga_index, IndexDestroy> temp;
  const sga_index* index = kdtree;
  if (!index) {  // (refuses a cloud with a non-finite coordinate)
    sga_index* made = nullptr;
    SGA_TRY(sga_index_build_kdtree(ctx, cloud, &made));
    temp.reset(made);
    index = made;
  } else {
    SGA_TRY(wait_ready(ctx, index->ready));
  }
  SGA_TRY(wait_ready(ctx, cloud->ready));
  if (n == 1) {  // no neighbour: a zero row
    count_launch(Chain::Fpfh);
    SGA_HIP(hipMemsetAsync(f->rows.p, 0, kFpDim * sizeof(float), ctx->stream));
    SGA_TRY(mark_ready(ctx, f->ready));
    *out = f.release();
    return SGA_OK;
  }
  FpfhArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = static_cast<uint32_t>(n);
  a.k = k;
  a.kp = static_cast<int>(std::min<size_t>(static_cast<size_t>(k), n - 1));
  DevBuf<uint32_t> nbr;   // both live to the end of the call (then: the stream's free list)
  DevBuf<double> spfh;
  SGA_TRY(nbr.alloc(n * static_cast<size_t>(a.kp)));
  SGA_TRY(spfh.alloc(n * static_cast<size_t>(kFpDim)));
  a.g = make_kd_view(index);
  a.pts = cloud->pts.p;
  a.nrm = cloud->nrm.p;
  a.nbr = nbr.p;
  a.spfh = spfh.p;
  a.rows = f->rows.p;
  a.has_vp = viewpoint != nullptr ? 1 : 0;
  for (int c = 0; c < 3; c++) a.vp[c] = viewpoint != nullptr ? viewpoint[c] - cloud->origin[c] : 0.0;
  count_launch(Chain::Fpfh);
  if (n <= static_cast<size_t>(knn_wave_max_points())) {  // the rule of sga_cloud_remove_outliers: clouds that do not fill the chip
    hipLaunchKernelGGL((fpfh_neighbours_kernel<0>), dim3(static_cast<unsigned>(n)), dim3(kFpBlock), 0, ctx->stream, a);
  } else {
    const dim3 grid(static_cast<unsigned>((n + kFpBlock - 1) / kFpBlock));
    const size_t stack_bytes = static_cast<size_t>(kKdMaxDepth) * 4 * kFpBlock;
    hipLaunchKernelGGL((fpfh_neighbours_kernel<1>), grid, dim3(kFpBlock), static_cast<size_t>((k + 1 + 3) & ~3) * 8 * kFpBlock + stack_bytes, ctx->stream, a);
  }
  SGA_HIP(hipGetLastError());
  const dim3 per_wave(static_cast<unsigned>((n + kFpWaves - 1) / kFpWaves));
  count_launch(Chain::Fpfh);
  hipLaunchKernelGGL(fpfh_spfh_kernel, per_wave, dim3(kFpWaves * 64), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::Fpfh);
  hipLaunchKernelGGL(fpfh_rows_kernel, per_wave, dim3(kFpWaves * 64), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  SGA_TRY(mark_ready(ctx, f->ready));
  if (!ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));  // a blocking context reports what its kernels met
  *out = f.release();
  return SGA_OK;
}

int sga_debug_cloud_fpfh_launches(unsigned long long* launches) { return report_launches(Chain::Fpfh, launches); }

}  // extern "C"

// ProjectiveSearch (ann/projective_search.hpp) as a target index: the build of the equirectangular index image, the standalone kNN, the
// source order of a problem over it, and the C entry points.  The factor kernel's search is projective_nearest (projective.hpp) inside
// linearize_group<..., TARGET = 3> (factor_stage.hpp).
#include "common.hpp"

#include <algorithm>
#include <cmath>
#include <memory>
#include "device_math.hpp"
#include "projective.hpp"

namespace sga {

// UnsafeProjectiveSearch's constructor (projective_search.hpp:49-62): points in index order, a later point overwrites an earlier one in
// its pixel, i.e. the HIGHEST index owns a pixel.  One thread per point: atomicMax of index + 1 over an image cleared to 0 gives exactly
// that image whatever order the threads run in.  Out-of-range pixels (u == W when lon == pi) are skipped (:58-60); so are non-finite points.
__global__ void projective_build_kernel(const float4* __restrict__ pts, size_t n, int W, int H, double ox, double oy, double oz, uint32_t* __restrict__ img) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int u, v;
  if (!proj_pixel(proj_add(p.x, ox), proj_add(p.y, oy), proj_add(p.z, oz), W, H, u, v)) return;
  if (u < 0 || u >= W || v < 0 || v >= H) return;
  atomicMax(&img[static_cast<size_t>(u) * H + v], static_cast<uint32_t>(i) + 1u);
}

// standalone kNN: one lane per query; the lane's k-best list is its row of the output (queries in the index's device frame)
template <typename Real>
__global__ void projective_knn_kernel(const ProjView pv, const float4* __restrict__ pts, const Real* __restrict__ queries, size_t m, int k, Real max_sq, long long* __restrict__ out_idx, Real* __restrict__ out_d2) {
  const size_t qi = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (qi >= m) return;
  long long* idx = out_idx + qi * k;
  Real* d2 = out_d2 + qi * k;
  const Real worst = sizeof(Real) == 8 ? static_cast<Real>(DBL_MAX) : static_cast<Real>(FLT_MAX);
  for (int j = 0; j < k; j++) {
    idx[j] = -1;
    d2[j] = worst;
  }
  projective_knn<Real, long long>(pv, pts, queries[3 * qi], queries[3 * qi + 1], queries[3 * qi + 2], k, idx, d2);
  for (int j = 0; j < k; j++) {  // the caller's distance bound as a filter (reject iff d2 > max_sq), "none" = (-1, inf)
    const bool ok = idx[j] >= 0 && !(d2[j] > max_sq);
    if (!ok) {
      idx[j] = -1;
      d2[j] = static_cast<Real>(INFINITY);
    }
  }
}

// sort key of a problem's source point (problem.hip): the u-major pixel of init_T p, so that neighbouring lanes scan overlapping windows
__global__ void projective_source_keys_kernel(const float4* __restrict__ pts, size_t n, Rigid<double> T, const ProjView pv, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  double qx, qy, qz;
  transform_point<double>(T, p.x, p.y, p.z, qx, qy, qz);
  int u, v;
  unsigned long long key = ~0ull;
  if (proj_pixel(proj_add(qx, pv.org[0]), proj_add(qy, pv.org[1]), proj_add(qz, pv.org[2]), pv.W, pv.H, u, v)) {
    u = min(max(u, 0), pv.W - 1);
    v = min(max(v, 0), pv.H - 1);
    key = static_cast<unsigned long long>(u) * pv.H + v;
  }
  keys[i] = key;
  vals[i] = static_cast<uint32_t>(i);
}

ProjView make_proj_view(const sga_index* idx) {
  ProjView v{};
  v.img = idx->proj_img.p;
  v.W = idx->proj_w;
  v.H = idx->proj_h;
  v.wh = idx->proj_win_h;
  v.wv = idx->proj_win_v;
  v.repeat_h = idx->proj_repeat_h;
  v.repeat_v = idx->proj_repeat_v;
  for (int k = 0; k < 3; k++) v.org[k] = idx->origin[k];
  return v;
}

int projective_source_keys(sga_context* ctx, const sga_index* idx, const float4* pts, size_t n, const double T_dev[16], unsigned long long* keys, uint32_t* vals) {
  hipLaunchKernelGGL(projective_source_keys_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, pts, n, rigid_from_colmajor<double>(T_dev), make_proj_view(idx), keys, vals);
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// sga_index_knn / sga_index_knn_f64 over a projective index (problem.hip: index_knn_impl).  The queries move to the index's device frame in
// double; fp64 (queries64): double distances, the reference's; fp32 (queries): the fp32 query, float distances.
int projective_index_knn(sga_context* ctx, const sga_index* index, const float* queries, const double* queries64, size_t m, int k, double max_sq_dist, int64_t* idx, float* sq_dist, double* sq_dist64) {
  const bool f64 = queries64 != nullptr;
  const size_t qbytes = m * 3 * (f64 ? sizeof(double) : sizeof(float));
  std::vector<double> qd;
  std::vector<float> qf;
  if (f64)
    qd.resize(m * 3);
  else
    qf.resize(m * 3);
  for (size_t i = 0; i < m * 3; i++) {
    const double v = (f64 ? queries64[i] : static_cast<double>(queries[i])) - index->origin[i % 3];
    if (f64)
      qd[i] = v;
    else
      qf[i] = static_cast<float>(v);
  }
  DevBuf<uint8_t> d_q, d_d;
  DevBuf<long long> d_i;
  SGA_TRY(d_q.alloc(qbytes));
  SGA_TRY(d_d.alloc(m * k * (f64 ? sizeof(double) : sizeof(float))));
  SGA_TRY(d_i.alloc(m * k));
  SGA_HIP(hipMemcpyAsync(d_q.p, f64 ? static_cast<const void*>(qd.data()) : static_cast<const void*>(qf.data()), qbytes, hipMemcpyHostToDevice, ctx->stream));
  const ProjView pv = make_proj_view(index);
  const dim3 grid((m + 255) / 256), block(256);
  if (f64)
    hipLaunchKernelGGL(projective_knn_kernel<double>, grid, block, 0, ctx->stream, pv, index->pts.p, reinterpret_cast<const double*>(d_q.p), m, k, max_sq_dist < 0 ? static_cast<double>(INFINITY) : max_sq_dist, d_i.p,
                       reinterpret_cast<double*>(d_d.p));
  else
    hipLaunchKernelGGL(projective_knn_kernel<float>, grid, block, 0, ctx->stream, pv, index->pts.p, reinterpret_cast<const float*>(d_q.p), m, k, max_sq_dist < 0 ? INFINITY : static_cast<float>(max_sq_dist), d_i.p,
                       reinterpret_cast<float*>(d_d.p));
  SGA_HIP(hipGetLastError());
  SGA_HIP(hipMemcpyAsync(idx, d_i.p, m * k * sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
  std::vector<float> tf;
  std::vector<double> td;
  if (f64) {
    if (!sq_dist64) td.resize(m * k);
    SGA_HIP(hipMemcpyAsync(sq_dist64 ? sq_dist64 : td.data(), d_d.p, m * k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  } else {
    if (!sq_dist) tf.resize(m * k);
    SGA_HIP(hipMemcpyAsync(sq_dist ? sq_dist : tf.data(), d_d.p, m * k * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
  }
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  if (f64 && sq_dist)
    for (size_t i = 0; i < m * k; i++) sq_dist[i] = static_cast<float>(sq_dist64 ? sq_dist64[i] : td[i]);
  if (!f64 && sq_dist64)
    for (size_t i = 0; i < m * k; i++) sq_dist64[i] = sq_dist ? sq_dist[i] : tf[i];
  return SGA_OK;
}

static int projective_index(const sga_index* index) {
  if (!index) return fail(SGA_ERR_INVALID, "null argument");
  if (index->kind != SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_INVALID, "not a projective search index");
  return SGA_OK;
}

}  // namespace sga

using namespace sga;

extern "C" {

int sga_index_build_projective(sga_context* ctx, const sga_cloud* cloud, int width, int height, sga_index** out) {
  if (!ctx || !cloud || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (width < 1 || height < 1 || static_cast<long long>(width) * height > (1ll << 30)) return fail(SGA_ERR_INVALID, "index map of %d x %d pixels: width and height must be positive, at most 2^30 pixels", width, height);
  if (cloud->n >= 0xffffffffull) return fail(SGA_ERR_INVALID, "a projective index holds fewer than 2^32 - 1 points");
  *out = nullptr;
  SGA_ENTER(ctx);
  const size_t n = cloud->n;
  std::unique_ptr<sga_index> idx(new sga_index);
  idx->kind = SGA_INDEX_PROJECTIVE;
  idx->device = ctx->device;
  idx->n = n;
  for (int k = 0; k < 3; k++) idx->origin[k] = cloud->origin[k];  // the records keep their cloud's device frame
  idx->has_normals = cloud->has_normals;
  idx->has_covs = cloud->has_covs;
  idx->proj_w = width;
  idx->proj_h = height;
  SGA_TRY(wait_ready(ctx, cloud->ready));
  const size_t pixels = static_cast<size_t>(width) * height;
  SGA_TRY(idx->proj_img.alloc(pixels));
  SGA_HIP(hipMemsetAsync(idx->proj_img.p, 0, pixels * sizeof(uint32_t), ctx->stream));
  if (n > 0) {
    // the target in its original order: a correspondence is the caller's index as it is
    SGA_TRY(idx->pts.alloc(n));
    SGA_HIP(hipMemcpyAsync(idx->pts.p, cloud->pts.p, n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    if (cloud->has_normals) {
      SGA_TRY(idx->nrm.alloc(n));
      SGA_HIP(hipMemcpyAsync(idx->nrm.p, cloud->nrm.p, n * sizeof(float4), hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (cloud->has_covs) {
      SGA_TRY(idx->cov.alloc(n));
      SGA_HIP(hipMemcpyAsync(idx->cov.p, cloud->cov.p, n * sizeof(Cov8), hipMemcpyDeviceToDevice, ctx->stream));
    }
    hipLaunchKernelGGL(projective_build_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, idx->pts.p, n, width, height, idx->origin[0], idx->origin[1], idx->origin[2], idx->proj_img.p);
    SGA_HIP(hipGetLastError());
  }
  if (!ctx->stream_ordered) SGA_HIP(hipStreamSynchronize(ctx->stream));
  SGA_TRY(mark_ready(ctx, idx->ready));
  *out = idx.release();
  return SGA_OK;
}

int sga_projective_set_search_window(sga_index* index, int h, int v) {
  SGA_TRY(projective_index(index));
  if (h < 0 || v < 0 || h > 65535 || v > 65535) return fail(SGA_ERR_INVALID, "search window (%d, %d): each half-width must be in [0, 65535]", h, v);
  index->proj_win_h = h;
  index->proj_win_v = v;
  return SGA_OK;
}

int sga_projective_set_border_modes(sga_index* index, int repeat_h, int repeat_v) {
  SGA_TRY(projective_index(index));
  index->proj_repeat_h = repeat_h ? 1 : 0;
  index->proj_repeat_v = repeat_v ? 1 : 0;
  return SGA_OK;
}

int sga_projective_get_params(const sga_index* index, int out[6]) {
  SGA_TRY(projective_index(index));
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  const int v[6] = {index->proj_w, index->proj_h, index->proj_win_h, index->proj_win_v, index->proj_repeat_h, index->proj_repeat_v};
  std::copy(v, v + 6, out);
  return SGA_OK;
}

int sga_projective_download_map(sga_context* ctx, const sga_index* index, uint32_t* out) {
  SGA_TRY(projective_index(index));
  if (!ctx || !out) return fail(SGA_ERR_INVALID, "null argument");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, index->ready));
  const size_t W = index->proj_w, H = index->proj_h;
  std::vector<uint32_t> img(W * H);
  SGA_HIP(hipMemcpyAsync(img.data(), index->proj_img.p, W * H * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t u = 0; u < W; u++)  // u-major index + 1 -> the reference's index_map(v, u), 0xFFFFFFFF = invalid_index (:145)
    for (size_t v = 0; v < H; v++) out[v * W + u] = img[u * H + v] == 0u ? 0xffffffffu : img[u * H + v] - 1u;
  return SGA_OK;
}

}  // extern "C"

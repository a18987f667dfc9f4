// ISS keypoints on the device: sga_cloud_iss_keypoints — the saliency of every point from the scatter of its
// fixed-radius neighbourhood, then the non-maximum suppression over a second radius, both over the walk of kd_radius.hpp, and the crop's
// stable compaction (cloud_crop.hip: cloud_crop_stat) when a cloud is asked for.  Everything is in cloud indices and in double from the
// fp32 records, as differences from the query's own record.  One host wait; no floating-point atomic: two calls give the same bytes.
#include "cloud_ops.hpp"
#include "forest.hpp"
#include "kd_radius.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kIssBlock = 64;  // walk kernels: points of a workgroup, one lane each, one wave

// What the kernels receive (kernel arguments: read with scalar loads)
struct IssArgs {
  KdView g;                 // the tree over the cloud
  double salient_radius, non_max_radius;
  double gamma_21, gamma_32;
  uint32_t n;
  uint32_t min_neighbors;
  double* sal;              // n: the saliency of every point, the cloud's order
  double* sal_host;         // n behind the count in a slot of the staging ring; or null
  double* flag;             // n: 0.0 where the point is a keypoint, 1.0 where it is not (held against 0.5)
  unsigned long long* count_host;  // the slot's first word: the keypoints (iss_list_kernel)
  uint32_t* kept_host;      // n indices in the slot; or null
};

// The eigenvalues of the symmetric matrix {{xx, xy, xz}, {xy, yy, yz}, {xz, yz, zz}}, descending: cyclic Jacobi rotations until the
// off-diagonal entries are exactly zero (an entry below 2^-53 / 100 of both its diagonal neighbours is set to zero from the fourth
// sweep on).  Absolute error a few ulps of the largest eigenvalue, also next to a double root, where the trigonometric closed form of
// preprocess.hip (eigen_sym3) loses half its digits.
__device__ __forceinline__ void iss_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, int sweep) {
  if (apq == 0.0) return;
  const double g = 100.0 * fabs(apq);
  if (sweep > 3 && fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) {
    apq = 0.0;
    return;
  }
  const double h = aqq - app;
  double t;
  if (fabs(h) + g == fabs(h)) {
    t = apq / h;
  } else {
    const double theta = 0.5 * h / apq;
    t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
  app -= t * apq;
  aqq += t * apq;
  apq = 0.0;
  const double rp = arp, rq = arq;  // the third row's two entries
  arp = rp - s * (rq + rp * tau);
  arq = rq + s * (rp - rq * tau);
}
__device__ __forceinline__ void iss_eigenvalues(double xx, double xy, double xz, double yy, double yz, double zz, double& l1, double& l2, double& l3) {
#pragma unroll 1
  for (int sweep = 0; sweep < 16 && (xy != 0.0 || xz != 0.0 || yz != 0.0); sweep++) {
    iss_rotate(xx, yy, xy, xz, yz, sweep);
    iss_rotate(xx, zz, xz, xy, yz, sweep);
    iss_rotate(yy, zz, yz, xy, xz, sweep);
  }
  l1 = fmax(xx, fmax(yy, zz));
  l3 = fmin(xx, fmin(yy, zz));
  l2 = fmax(fmin(xx, yy), fmin(fmax(xx, yy), zz));  // the median itself, not a difference of sums
}

}  // namespace

// Lane i of the grid owns the record at kd position i (neighbouring lanes walk neighbouring paths) and acts for the cloud index in its w.
// RULES 1 - 3: the count, sum x and sum x x^T of the neighbourhood in ten registers, the covariance, its eigenvalues, the saliency.
__global__ __launch_bounds__(kIssBlock) void iss_saliency_kernel(const IssArgs a) {
  extern __shared__ uint32_t iss_stack[];  // [kKdMaxDepth][kIssBlock] words
  const int lane = threadIdx.x;
  const uint32_t pos = blockIdx.x * static_cast<uint32_t>(kIssBlock) + lane;
  if (pos >= a.n) return;  // (the walk has no wave-level step)
  const float4 p = a.g.pts[pos];
  const uint32_t i = __float_as_uint(p.w);
  uint32_t c = 0;
  double sx = 0.0, sy = 0.0, sz = 0.0, sxx = 0.0, sxy = 0.0, sxz = 0.0, syy = 0.0, syz = 0.0, szz = 0.0;
  auto add = [&](uint32_t, double, double dx, double dy, double dz) {
    c++;
    sx += dx, sy += dy, sz += dz;
    sxx += dx * dx, sxy += dx * dy, sxz += dx * dz, syy += dy * dy, syz += dy * dz, szz += dz * dz;
  };
  kd_radius_walk<kIssBlock>(a.g, static_cast<double>(p.x), static_cast<double>(p.y), static_cast<double>(p.z), a.salient_radius, iss_stack, lane, add);
  double sal = 0.0;
  if (c >= a.min_neighbors) {  // (c >= 1: the point itself)
    const double k = static_cast<double>(c);
    const double mx = sx / k, my = sy / k, mz = sz / k;
    double l1, l2, l3;
    iss_eigenvalues(sxx / k - mx * mx, sxy / k - mx * my, sxz / k - mx * mz, syy / k - my * my, syz / k - my * mz, szz / k - mz * mz, l1, l2, l3);
    if (l1 > 0.0 && l2 < a.gamma_21 * l1 && l3 < a.gamma_32 * l2 && l3 > 1e-9 * l1) sal = l3;
  }
  a.sal[i] = sal;
  if (a.sal_host != nullptr) {
    a.sal_host[i] = sal;
    __threadfence_system();
  }
}

// RULE 4: a salient point is a keypoint when its window holds min_neighbors records and none of them beats it (a greater saliency, or
// the same one at a lower index).  Every saliency is read: the launch behind iss_saliency_kernel's.
__global__ __launch_bounds__(kIssBlock) void iss_nms_kernel(const IssArgs a) {
  extern __shared__ uint32_t iss_stack[];
  const int lane = threadIdx.x;
  const uint32_t pos = blockIdx.x * static_cast<uint32_t>(kIssBlock) + lane;
  if (pos >= a.n) return;
  const float4 p = a.g.pts[pos];
  const uint32_t i = __float_as_uint(p.w);
  const double own = a.sal[i];
  if (own == 0.0) {
    a.flag[i] = 1.0;
    return;
  }
  uint32_t c = 0;
  bool beaten = false;
  auto window = [&](uint32_t j, double) {
    c++;
    const double s = a.sal[j];
    if (j != i && (s > own || (s == own && j < i))) beaten = true;
  };
  kd_radius_walk<kIssBlock>(a.g, static_cast<double>(p.x), static_cast<double>(p.y), static_cast<double>(p.z), a.non_max_radius, iss_stack, lane, window);
  a.flag[i] = !beaten && c >= a.min_neighbors ? 0.0 : 1.0;
}

// Without a cloud: the keypoints counted and, on request, listed in index order by ONE workgroup (kd_radius.hpp: one_block_prefix), into the slot.
__global__ __launch_bounds__(kRadScanThreads) void iss_list_kernel(const IssArgs a) {
  __shared__ unsigned long long sh[kRadScanThreads];
  uint32_t first, end;
  unsigned long long total;
  unsigned long long at = one_block_prefix(a.n, first, end, sh, total, [&](uint32_t v) { return a.flag[v] <= 0.5 ? 1ull : 0ull; });
  if (a.kept_host != nullptr)
    for (uint32_t v = first; v < end; v++)
      if (a.flag[v] <= 0.5) a.kept_host[at++] = v;  // (at < total <= n)
  if (threadIdx.x == 0) a.count_host[0] = total;
  __threadfence_system();
}

namespace {

// what sga_cloud_iss_keypoints refuses of its arguments (no handle is read)
int iss_check(const sga_iss_params& p, sga_cloud* const* out) {
  if (!(p.salient_radius - p.salient_radius == 0.0 && p.salient_radius > 0.0)) return fail(SGA_ERR_INVALID, "iss: salient_radius must be finite and > 0");
  if (!(p.non_max_radius - p.non_max_radius == 0.0 && p.non_max_radius > 0.0)) return fail(SGA_ERR_INVALID, "iss: non_max_radius must be finite and > 0");
  if (!(p.gamma_21 > 0.0 && p.gamma_21 <= 1.0)) return fail(SGA_ERR_INVALID, "iss: gamma_21 must be in (0, 1]");
  if (!(p.gamma_32 > 0.0 && p.gamma_32 <= 1.0)) return fail(SGA_ERR_INVALID, "iss: gamma_32 must be in (0, 1]");
  if (p.min_neighbors < 1) return fail(SGA_ERR_INVALID, "iss: min_neighbors %d is below 1", p.min_neighbors);
  if (p.keep < 0 || p.keep > 1) return fail(SGA_ERR_INVALID, "iss: keep %d is not 0 (no cloud) or 1 (the keypoints)", p.keep);
  if (p.keep == 0 && out != nullptr) return fail(SGA_ERR_INVALID, "iss: keep is 0 but an output cloud is asked for");
  if (p.keep != 0 && out == nullptr) return fail(SGA_ERR_INVALID, "iss: keep is %d but there is no place for the output cloud", p.keep);
  return SGA_OK;
}

struct IndexDestroy {
  void operator()(sga_index* i) const { (void)sga_index_destroy(i); }
};
struct CloudDestroy {
  void operator()(sga_cloud* c) const { (void)sga_cloud_destroy(c); }
};

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_iss_default(sga_iss_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->gamma_21 = 0.975;
  p->gamma_32 = 0.975;
  p->min_neighbors = 5;
}

int sga_cloud_iss_keypoints(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree, const sga_iss_params* params, double* saliency, int64_t* kept, size_t* count, sga_cloud** out) {
  if (out) *out = nullptr;
  if (count) *count = 0;
  if (!ctx || !cloud || !params || !count) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(iss_check(*params, out));
  // ---- (from here on the handles are read)
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (kdtree) {  // checked as sga_cloud_cluster checks it
    if (kdtree->kind == SGA_INDEX_PROJECTIVE) return fail(SGA_ERR_UNSUPPORTED, "iss keypoints need a kd-tree index, not a projective search");
    if (kdtree->kind != SGA_INDEX_KDTREE) return fail(SGA_ERR_INVALID, "a kd-tree index is required");
    if (kdtree->device != ctx->device) return fail(SGA_ERR_INVALID, "index lives on another device");
    if (kdtree->n != n) return fail(SGA_ERR_INVALID, "index was built over a cloud of %zu points, got %zu", kdtree->n, n);
    for (int a = 0; a < 3; a++)
      if (kdtree->origin[a] != cloud->origin[a]) return fail(SGA_ERR_INVALID, "the index was not built over this cloud (their device frames differ)");
  }
  CropStat cs{nullptr, nullptr, 0.5, Chain::Keypoints};
  if (n == 0) return out ? cloud_crop_stat(ctx, cloud, cs, kept, out) : SGA_OK;  // an empty cloud, no keypoints; nothing is launched
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", n);
  SGA_ENTER(ctx);
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
  DevBuf<double> work;  // the saliencies and the flags
  SGA_TRY(work.alloc(2 * n));
  // the count, the saliencies and — without a cloud — the indices leave through ONE slot of the staging ring, which the kernels write by its device address
  const bool list = out == nullptr;
  const size_t sal_bytes = saliency != nullptr ? n * sizeof(double) : 0;
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, 8 + sal_bytes + (list && kept != nullptr ? n * sizeof(uint32_t) : 0), &slot));
  char* slot_dev = static_cast<char*>(slot->dev);
  IssArgs a;
  std::memset(&a, 0, sizeof(a));
  a.g = make_kd_view(index);
  a.salient_radius = params->salient_radius, a.non_max_radius = params->non_max_radius;
  a.gamma_21 = params->gamma_21, a.gamma_32 = params->gamma_32;
  a.n = static_cast<uint32_t>(n);
  a.min_neighbors = static_cast<uint32_t>(params->min_neighbors);
  a.sal = work.p;
  a.flag = work.p + n;
  a.count_host = reinterpret_cast<unsigned long long*>(slot_dev);
  a.sal_host = saliency != nullptr ? reinterpret_cast<double*>(slot_dev + 8) : nullptr;
  a.kept_host = list && kept != nullptr ? reinterpret_cast<uint32_t*>(slot_dev + 8 + sal_bytes) : nullptr;
  const dim3 walk(static_cast<unsigned>((n + kIssBlock - 1) / kIssBlock));
  const size_t stack_bytes = static_cast<size_t>(kKdMaxDepth) * 4 * kIssBlock;
  count_launch(Chain::Keypoints);
  hipLaunchKernelGGL(iss_saliency_kernel, walk, dim3(kIssBlock), stack_bytes, ctx->stream, a);
  count_launch(Chain::Keypoints);
  hipLaunchKernelGGL(iss_nms_kernel, walk, dim3(kIssBlock), stack_bytes, ctx->stream, a);
  if (list) {
    count_launch(Chain::Keypoints);
    hipLaunchKernelGGL(iss_list_kernel, dim3(1), dim3(kRadScanThreads), 0, ctx->stream, a);
  }
  SGA_HIP(hipGetLastError());
  const char* host = static_cast<const char*>(slot->host);
  std::unique_ptr<sga_cloud, CloudDestroy> made;
  size_t m = 0;
  count_launch(Chain::KeypointsWait);
  if (!list) {
    sga_cloud* c = nullptr;
    cs.d = a.flag;
    SGA_TRY(cloud_crop_stat(ctx, cloud, cs, kept, &c));  // (its wait shows that everything above has run)
    made.reset(c);
    m = c->n;
  } else {
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait
    const unsigned long long counted = *reinterpret_cast<const unsigned long long*>(host);
    if (counted > n) return fail(SGA_ERR_HIP, "the device reported %llu keypoints among %zu points", counted, n);
    m = static_cast<size_t>(counted);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(host + 8 + sal_bytes);
    for (size_t j = 0; kept != nullptr && j < m; j++) kept[j] = static_cast<int64_t>(src[j]);
  }
  if (saliency) std::memcpy(saliency, host + 8, sal_bytes);
  *count = m;
  if (out) *out = made.release();
  return SGA_OK;
}

int sga_debug_iss_launches(unsigned long long* launches) { return report_launches(Chain::Keypoints, launches); }
int sga_debug_iss_waits(unsigned long long* waits) { return report_launches(Chain::KeypointsWait, waits); }

}  // extern "C"

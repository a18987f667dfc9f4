// The cloud handle itself (cloud_ops.hpp): the maker of output clouds, the preamble of the calls over many clouds, the box a cloud keeps
// and the getters.  Uploads and downloads: cloud_io.hip; merge and deskew: cloud_pose.hip; crop, select and slice: cloud_crop.hip.
#include "cloud_ops.hpp"

#include <cmath>

namespace sga {

int cloud_make(const sga_context* ctx, const double origin[3], size_t n, bool normals, bool covs, std::unique_ptr<sga_cloud>* out) {
  std::unique_ptr<sga_cloud> c(new sga_cloud);
  c->device = ctx->device;
  c->n = n;
  for (int k = 0; k < 3; k++) c->origin[k] = origin ? origin[k] : 0.0;
  c->has_normals = normals;
  c->has_covs = covs;
  SGA_TRY(c->pts.alloc(n));
  if (normals) SGA_TRY(c->nrm.alloc(n));
  if (covs) SGA_TRY(c->cov.alloc(n));
  *out = std::move(c);
  return SGA_OK;
}

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

int cloud_members_args(const sga_cloud* const* clouds, size_t count, const void* const* also, const char* also_name) {
  if (count > kCloudMaxMembers) return fail(SGA_ERR_INVALID, "too many members (%zu; limit %zu)", count, kCloudMaxMembers);
  for (size_t k = 0; k < count; k++) {
    if (!clouds[k]) return fail(SGA_ERR_INVALID, "null argument: clouds[%zu] is NULL", k);
    if (also != nullptr && !also[k]) return fail(SGA_ERR_INVALID, "null argument: %s[%zu] is NULL", also_name, k);
  }
  return SGA_OK;
}

int cloud_members(const sga_context* ctx, const sga_cloud* const* clouds, size_t count, size_t per_block, CloudMembers* m) {
  for (size_t k = 0; k < count; k++) {
    if (clouds[k]->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud %zu lives on another device", k);
    if (clouds[k]->n == 0) continue;
    m->live.push_back(k);
    m->points += clouds[k]->n;
    m->blocks += (clouds[k]->n + per_block - 1) / per_block;
    m->normals = m->normals && clouds[k]->has_normals;
    m->covs = m->covs && clouds[k]->has_covs;
  }
  return SGA_OK;
}

}  // namespace sga

using namespace sga;

extern "C" {

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

int sga_cloud_origin(const sga_cloud* cloud, double origin[3]) {
  if (!cloud || !origin) return fail(SGA_ERR_INVALID, "null argument");
  for (int k = 0; k < 3; k++) origin[k] = cloud->origin[k];
  return SGA_OK;
}

int sga_debug_cloud_box(const sga_cloud* cloud, int* has_box, float lo[3], float hi[3]) {
  if (!cloud || !has_box || !lo || !hi) return fail(SGA_ERR_INVALID, "null argument");
  *has_box = cloud->has_box ? 1 : 0;
  for (int k = 0; k < 3; k++) lo[k] = cloud->has_box ? cloud->box_lo[k] : 0.f, hi[k] = cloud->has_box ? cloud->box_hi[k] : 0.f;
  return SGA_OK;
}

}  // extern "C"

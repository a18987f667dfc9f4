// What the cloud translation units (cloud.hip, cloud_io.hip, cloud_pose.hip, cloud_crop.hip, cloud_outliers.hip, cloud_overlap.hip, cloud_visibility.hip) share on the host.
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"
#include "forest.hpp"

namespace sga {

// ---- cloud.hip --------------------------------------------------------------------------------------------------------------------
// A cloud on the context's device, in the device frame at `origin` (null: zero), with room for n records and the attributes chosen
int cloud_make(const sga_context* ctx, const double origin[3], size_t n, bool normals, bool covs, std::unique_ptr<sga_cloud>* out);
// ... in the frame of `in` and with its attributes; n == 0: an empty cloud without attributes (select, crop, deskew)
inline int cloud_make_like(const sga_context* ctx, const sga_cloud* in, size_t n, std::unique_ptr<sga_cloud>* out) { return cloud_make(ctx, in->origin, n, n > 0 && in->has_normals, n > 0 && in->has_covs, out); }
// what an entry point made for its members becomes the caller's
inline int hand_over(std::vector<std::unique_ptr<sga_cloud>>& made, sga_cloud** out) {
  for (size_t k = 0; k < made.size(); k++) out[k] = made[k].release();
  return SGA_OK;
}
// The box of the records (device frame) from the box of the inputs, when there is one (lo <= hi): fp32 of (box - origin) — relative: the
// inputs ARE the records — rounded outwards on request.
void cloud_set_box(sga_cloud* c, const double lo[3], const double hi[3], bool relative, bool outward);

// The preamble of a call over `count` clouds (merge, deskew, crop), in two steps: the checks of the call's other arguments go between
// them, so that everything that reads only arguments happens before any handle is read.
constexpr size_t kCloudMaxMembers = 1u << 15;
// 1. the member limit and the null members, named by number (also[k], when given, right behind clouds[k], under the name also_name)
int cloud_members_args(const sga_cloud* const* clouds, size_t count, const void* const* also = nullptr, const char* also_name = nullptr);
// 2. the handles: a member on another device is refused by number; live: the non-empty members (empty ones take no workgroups), their
// points, their workgroups of per_block points each, and whether all of them have an attribute
struct CloudMembers {
  std::vector<size_t> live;
  size_t points = 0, blocks = 0;
  bool normals = true, covs = true;
};
int cloud_members(const sga_context* ctx, const sga_cloud* const* clouds, size_t count, size_t per_block, CloudMembers* m);

// A member's slot of a deskew or a crop in the context's box block (cloud_box.hpp: MemberBoxes): the points kept (crop only), then the box (box_dec64)
constexpr size_t kBoxSlotWords = 8;
constexpr int kBoxSlotCount = 0, kBoxSlotLo = 1, kBoxSlotHi = 4;

// ---- cloud_io.hip -----------------------------------------------------------------------------------------------------------------
int ensure_box64(sga_context* ctx);  // the context's 64-bit box accumulator (d_box64), made on first use
// Is [p, p + bytes) pinned host memory a kernel of this device can read (hipHostMalloc / hipHostRegister / sga_host_alloc)?  -> its device
// address.  on_device (optional): set when p is device memory, which no host entry point takes
const void* pinned_device_view(const void* p, size_t bytes, bool* on_device = nullptr);

// ---- cloud_crop.hip, for sga_cloud_remove_outliers (cloud_outliers.hip) sga_cloud_overlap (cloud_overlap.hip, 3.22) sga_cloud_visibility (cloud_visibility.hip, 3.23) and sga_cloud_iss_keypoints (cloud_keypoints.hip, 3.28) ----
// The crop's compaction — its table, its ONE launch, its one wait, its output cloud — over the points i of `cloud` with d[i] <= the limit.
// d (the cloud's size, the cloud's order) and limit are device memory that launches enqueued earlier on the context's stream write;
// limit == nullptr: limit_value travels in the call's table; d == nullptr (with every_record): every point is kept.  The table copy and the launch are counted under `chain`.
struct CropStat {
  const double* d;
  const double* limit;
  double limit_value;
  Chain chain = Chain::Outliers;
  bool every_record = false;  // the statistic alone decides: records with a non-finite coordinate, which the crop's own predicate drops, pass it (cloud_plane.hip)
};
int cloud_crop_stat(sga_context* ctx, const sga_cloud* cloud, const CropStat& stat, int64_t* kept /* or null */, sga_cloud** out);

}  // namespace sga

// crop_clouds, PointCloud::cropped with kept and PointCloud::selected (include/small_gicp_amd.hpp: sga_cloud_crop_batch / sga_cloud_crop /
// sga_cloud_select) against a host loop: the predicate of small_gicp_amd.h in double per point, the survivors in the input's order.
// usage: test_cpp_cloud_crop points.f32   (raw float32 xyz triples)
// Members: slices of the file of different length, preprocessed by the header's own calls (normals and covariances), each under its own crop.
//   CROP   k kept <m> of <n> equal <0|1> close <c>   the batch's member: kept[] is the host loop's list, record j is input record kept[j] bit for
//                                                    bit (point, normal, covariance); c = points whose d2 lies within 64 eps64 of a bound (0: the
//                                                    comparison does not hang on one rounding)
//   LONE   k equal <0|1>                             cropped() of the member alone equals the batch's member, kept included
//   SELECT k equal <0|1>                             selected(indices) — a stride-7 walk with repeats — is input[indices] bit for bit
//   REFUSE equal <0|1>                               an index out of range throws and names its position
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

static const double kEps = 2.220446049250313e-16;

static bool finite3(const std::array<double, 4>& p) { return p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0; }

// the host loop: indices kept of `in` under `c` (the clouds of this test keep the origin zero: point(i) is the record); *close counts the
// points whose d2 a rounding could move across a bound
static std::vector<int64_t> host_crop(const PointCloud& in, const sga_crop& c, int* close) {
  std::vector<int64_t> kept;
  const double r2min = c.min_range * c.min_range, r2max = c.max_range * c.max_range;
  for (size_t i = 0; i < in.size(); i++) {
    const auto p = in.point(i);
    if (!finite3(p)) continue;
    const double x = p[0] - c.center[0], y = p[1] - c.center[1], z = p[2] - c.center[2];
    const double d2 = x * x + y * y + z * z;
    if (std::fabs(d2 - r2min) <= 64 * kEps * d2 || std::fabs(d2 - r2max) <= 64 * kEps * d2) (*close)++;
    bool keep = r2min <= d2 && d2 <= r2max;
    if (c.box_mode != 0) {
      const bool inside = c.box_lo[0] <= p[0] && p[0] <= c.box_hi[0] && c.box_lo[1] <= p[1] && p[1] <= c.box_hi[1] && c.box_lo[2] <= p[2] && p[2] <= c.box_hi[2];
      keep = keep && (inside == (c.box_mode == 1));
    }
    if (keep) kept.push_back(static_cast<int64_t>(i));
  }
  return kept;
}

// out record j == in record idx[j], attributes included
static bool gathered(const PointCloud& in, const std::vector<int64_t>& idx, const PointCloud& out) {
  bool ok = out.size() == idx.size();
  if (ok && !idx.empty()) ok = in.has_normals() == out.has_normals() && in.has_covs() == out.has_covs();
  for (size_t j = 0; ok && j < idx.size(); j++) {
    const size_t i = static_cast<size_t>(idx[j]);
    ok = in.point(i) == out.point(j) && in.normal(i) == out.normal(j) && in.cov(i) == out.cov(j);
  }
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);

    const size_t lengths[3] = {pts.size(), pts.size() / 2, pts.size() / 3};
    std::vector<std::shared_ptr<const PointCloud>> clouds;
    for (size_t len : lengths) {
      std::vector<std::array<float, 3>> part(pts.begin(), pts.begin() + len);
      auto [cloud, tree] = preprocess_points(part, 0.5, 10);
      clouds.push_back(cloud);
    }
    clouds.push_back(clouds[0]);  // one cloud twice, under two crops
    sga_context* ctx = clouds[0]->ctx;
    const size_t B = clouds.size();
    std::vector<Crop> crops = {Crop(5.0, 30.0), Crop().box({-6.0, -4.0, -3.0}, {6.0, 4.0, 3.0}, 2), Crop(0.0, 10.0).about({4.0, -2.0, 0.5}).box({-20.0, -20.0, -3.0}, {20.0, 20.0, 3.0}, 1), Crop(1e3, 2e3)};
    std::vector<std::vector<int64_t>> kept;
    const std::vector<PointCloud::Ptr> out = crop_clouds(ctx, clouds, crops, &kept);
    for (size_t k = 0; k < B; k++) {
      int close = 0;
      const std::vector<int64_t> want = host_crop(*clouds[k], crops[k], &close);
      const bool ok = kept[k] == want && gathered(*clouds[k], want, *out[k]);
      std::printf("CROP %zu kept %zu of %zu equal %d close %d\n", k, out[k]->size(), clouds[k]->size(), ok ? 1 : 0, close);
      std::vector<int64_t> lone_kept;
      const PointCloud::Ptr lone = clouds[k]->cropped(crops[k], &lone_kept);
      std::printf("LONE %zu equal %d\n", k, lone_kept == kept[k] && gathered(*clouds[k], lone_kept, *lone) ? 1 : 0);
      std::vector<int64_t> idx;
      const size_t n = clouds[k]->size();
      for (size_t j = 0; j < n + 5; j++) idx.push_back(static_cast<int64_t>((j * 7) % n));
      std::printf("SELECT %zu equal %d\n", k, gathered(*clouds[k], idx, *clouds[k]->selected(idx)) ? 1 : 0);
    }
    bool refused = false;
    try {
      clouds[1]->selected({0, 1, static_cast<int64_t>(clouds[1]->size())});
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "indices[2]") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

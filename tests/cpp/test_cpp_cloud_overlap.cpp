// PointCloud::overlap with Overlap (include/small_gicp_amd.hpp) against the C-ABI call it wraps (sga_cloud_overlap), on a kd-tree target
// and on a Gaussian voxel map.
// usage: test_cpp_cloud_overlap points.f32   (raw float32 xyz triples)
// The target is the preprocessed scan (the header's own call: voxel grid, tree, covariances) and the one-shot Gaussian map over it; the
// cloud is the same scan moved by a small rigid motion and preprocessed in the same way, the pose handed to the call its inverse.
//   OVERLAP <kd|map> keep <k> points <n> matched <m> stats <0|1> kept <0|1> arrays <0|1> cloud <0|1>
//       stats: the wrapper's statistics are the C call's, bit for bit, and fitness == matched / points; kept: the wrapper's kept[] is the
//       C call's, of the output's size and ascending; arrays: dist[] and nearest[] are the C call's and say "unmatched" together
//       (dist = +inf <=> nearest = -1) for exactly points - matched entries; cloud: record j of the output is record kept[j] of the input
//   REFUSE equal <0|1>   an output cloud's keep with a max_distance of 0 throws and names max_distance
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

static bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof(double)) == 0; }

static void run(const char* name, const PointCloud& cloud, const sga_index* target, const Isometry3d& T, Overlap::Keep keep, double max_distance) {
  const size_t n = cloud.size();
  const OverlapResult r = cloud.overlap(target, &T, Overlap(max_distance, keep), true, true, keep != Overlap::None);
  sga_overlap p;
  sga_overlap_default(&p);
  p.max_distance = max_distance, p.keep = static_cast<int>(keep);
  std::vector<double> dist(n);
  std::vector<int64_t> nearest(n), kept(n);
  sga_overlap_stats st;
  sga_cloud* made = nullptr;
  check(sga_cloud_overlap(cloud.ctx, cloud.h, target, T.data(), &p, dist.data(), nearest.data(), keep != Overlap::None ? kept.data() : nullptr, &st, keep != Overlap::None ? &made : nullptr), "sga_cloud_overlap");
  size_t m = 0;
  if (made) {
    sga_cloud_size(made, &m);
    sga_cloud_destroy(made);
  }
  kept.resize(m);
  const bool stats = r.stats.points == st.points && r.stats.matched == st.matched && same_bits(r.stats.fitness, st.fitness) && same_bits(r.stats.rmse, st.rmse) && same_bits(r.stats.mean_distance, st.mean_distance) &&
                     st.points == n && same_bits(st.fitness, static_cast<double>(st.matched) / static_cast<double>(n));
  const bool kept_ok = r.kept == kept && std::is_sorted(kept.begin(), kept.end()) && (keep == Overlap::None ? !r.cloud : (r.cloud && r.cloud->size() == m));
  size_t unmatched = 0;
  bool arrays = r.dist.size() == n && r.nearest == nearest && std::memcmp(r.dist.data(), dist.data(), n * sizeof(double)) == 0;
  for (size_t i = 0; i < n; i++) {
    const bool none = nearest[i] < 0;
    arrays = arrays && none == std::isinf(dist[i]) && (none || dist[i] <= max_distance);
    unmatched += none ? 1 : 0;
  }
  arrays = arrays && unmatched == st.points - st.matched;
  bool gathered = true;
  if (r.cloud) {
    gathered = m == (keep == Overlap::Matched ? st.matched : st.points - st.matched) && r.cloud->has_covs() == cloud.has_covs();
    for (size_t j = 0; gathered && j < m; j++) {
      const size_t i = static_cast<size_t>(kept[j]);
      gathered = (nearest[i] >= 0) == (keep == Overlap::Matched) && cloud.point(i) == r.cloud->point(j) && cloud.cov(i) == r.cloud->cov(j);
    }
  }
  std::printf("OVERLAP %s keep %d points %zu matched %zu stats %d kept %d arrays %d cloud %d\n", name, static_cast<int>(keep), st.points, st.matched, stats ? 1 : 0, kept_ok ? 1 : 0, arrays ? 1 : 0, gathered ? 1 : 0);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
    auto [target, tree] = preprocess_points(pts, 0.5, 10);
    const GaussianVoxelMap::Ptr map = create_gaussian_voxelmap(*target, 1.0);
    // the scan seen from a pose a little off: x' = R^T (x - t) with a yaw of 0.02 rad and t = (0.3, -0.2, 0.05)
    Isometry3d T;
    const double c = std::cos(0.02), s = std::sin(0.02);
    T(0, 0) = c, T(0, 1) = -s, T(1, 0) = s, T(1, 1) = c;
    T(0, 3) = 0.3, T(1, 3) = -0.2, T(2, 3) = 0.05;
    const Isometry3d Ti = T.inverse();
    std::vector<std::array<float, 3>> moved(pts.size());
    for (size_t i = 0; i < pts.size(); i++)
      for (int r = 0; r < 3; r++) moved[i][r] = static_cast<float>(Ti(r, 0) * pts[i][0] + Ti(r, 1) * pts[i][1] + Ti(r, 2) * pts[i][2] + Ti(r, 3));
    auto [cloud, cloud_tree] = preprocess_points(moved, 0.5, 10);
    (void)cloud_tree;
    for (Overlap::Keep keep : {Overlap::None, Overlap::Matched, Overlap::Unmatched}) {
      run("kd", *cloud, tree->h, T, keep, 0.25);
      run("map", *cloud, map->h, T, keep, 0.5);
    }
    bool refused = false;
    try {
      cloud->overlap(tree->h, &T, Overlap(0.0, Overlap::Matched));
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "max_distance") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

// PointCloud::visibility with Visibility (include/small_gicp_amd.hpp) against the C-ABI call it wraps (sga_cloud_visibility).
// usage: test_cpp_cloud_visibility points.f32   (raw float32 xyz triples, sensor frame: x forward, y left, z up)
// The map is the preprocessed scan (the header's own call: voxel grid, tree, covariances); the scan is the raw scan seen from a pose a
// little off, the pose handed to the call, with every return on the sensor's left (y > 0) half as far again: the map's points there have
// become free space.
//   VISIBILITY keep <k> points <n> seen <m> stats <0|1> kept <0|1> arrays <0|1> cloud <0|1>
//       stats: the wrapper's counts are the C call's and sum to points; kept: the wrapper's kept[] is the C call's, of the output's size and
//       ascending; arrays: state[], clearance[] and the range image are the C call's bit for bit, the states' counts are the statistics',
//       the clearance is NaN exactly where the state is 0; cloud: record j of the output is record kept[j] of the map, and the states
//       of the kept points are what keep asks for
//   REFUSE equal <0|1>   a window of 17 throws and names the window
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

static void run(const PointCloud& map, const PointCloud& scan, const Isometry3d& T, Visibility::Keep keep) {
  const size_t n = map.size();
  Visibility what(keep);
  what.width = 512, what.height = 32;
  const VisibilityResult r = map.visibility(scan, &T, what, true, true, true, keep != Visibility::None);
  const size_t cells = static_cast<size_t>(what.width) * what.height;
  std::vector<uint8_t> state(n);
  std::vector<double> clearance(n), image(cells);
  std::vector<int64_t> kept(n);
  sga_visibility_stats st;
  sga_cloud* made = nullptr;
  check(sga_cloud_visibility(map.ctx, map.h, scan.h, T.data(), &what, state.data(), clearance.data(), image.data(), keep != Visibility::None ? kept.data() : nullptr, &st, keep != Visibility::None ? &made : nullptr),
        "sga_cloud_visibility");
  size_t m = 0;
  if (made) {
    sga_cloud_size(made, &m);
    sga_cloud_destroy(made);
  }
  kept.resize(m);
  const bool stats = std::memcmp(&r.stats, &st, sizeof(st)) == 0 && st.points == n && st.unobserved + st.consistent + st.occluded + st.seen_through == n;
  const bool kept_ok = r.kept == kept && std::is_sorted(kept.begin(), kept.end()) && (keep == Visibility::None ? !r.cloud : (r.cloud && r.cloud->size() == m));
  size_t count[4] = {0, 0, 0, 0};
  bool arrays = r.state == state && r.clearance.size() == n && std::memcmp(r.clearance.data(), clearance.data(), n * sizeof(double)) == 0 && r.range_image.size() == cells &&
                std::memcmp(r.range_image.data(), image.data(), cells * sizeof(double)) == 0;
  for (size_t i = 0; i < n; i++) {
    arrays = arrays && state[i] <= 3 && (state[i] == Visibility::Unobserved) == std::isnan(clearance[i]);
    count[state[i] & 3]++;
  }
  arrays = arrays && count[0] == st.unobserved && count[1] == st.consistent && count[2] == st.occluded && count[3] == st.seen_through;
  size_t returns = 0;
  for (size_t c = 0; c < cells; c++) returns += std::isinf(image[c]) ? 0 : 1;
  arrays = arrays && returns > 0 && returns < cells;
  bool gathered = true;
  if (r.cloud) {
    gathered = m == (keep == Visibility::SeenThrough ? st.seen_through : st.points - st.seen_through) && (m == 0 || r.cloud->has_covs() == map.has_covs());
    for (size_t j = 0; gathered && j < m; j++) {
      const size_t i = static_cast<size_t>(kept[j]);
      gathered = (state[i] == Visibility::Seen) == (keep == Visibility::SeenThrough) && map.point(i) == r.cloud->point(j) && map.cov(i) == r.cloud->cov(j);
    }
  }
  std::printf("VISIBILITY keep %d points %zu seen %zu stats %d kept %d arrays %d cloud %d\n", static_cast<int>(keep), st.points, st.seen_through, stats ? 1 : 0, kept_ok ? 1 : 0, arrays ? 1 : 0, gathered ? 1 : 0);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
    auto [map, tree] = preprocess_points(pts, 0.5, 10);
    (void)tree;
    // the scan seen from a pose a little off: x' = R^T (x - t) with a yaw of 0.02 rad and t = (0.3, -0.2, 0.05)
    Isometry3d T;
    const double c = std::cos(0.02), s = std::sin(0.02);
    T(0, 0) = c, T(0, 1) = -s, T(1, 0) = s, T(1, 1) = c;
    T(0, 3) = 0.3, T(1, 3) = -0.2, T(2, 3) = 0.05;
    const Isometry3d Ti = T.inverse();
    std::vector<std::array<float, 3>> moved(pts.size());
    for (size_t i = 0; i < pts.size(); i++)
      for (int r = 0; r < 3; r++) moved[i][r] = static_cast<float>(Ti(r, 0) * pts[i][0] + Ti(r, 1) * pts[i][1] + Ti(r, 2) * pts[i][2] + Ti(r, 3));
    for (auto& p : moved)
      if (p[1] > 0.f) p = {1.5f * p[0], 1.5f * p[1], 1.5f * p[2]};
    const PointCloud scan(moved);
    for (Visibility::Keep keep : {Visibility::None, Visibility::SeenThrough, Visibility::Rest}) run(*map, scan, T, keep);
    bool refused = false;
    try {
      Visibility bad;
      bad.window_h = 17;
      map->visibility(scan, &T, bad);
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "window") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

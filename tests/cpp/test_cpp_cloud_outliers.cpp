// PointCloud::without_outliers with OutlierFilter (include/small_gicp_amd.hpp: sga_cloud_remove_outliers) against a host loop: brute-force
// distances in double over the cloud's points, the k + 1 smallest per point, and the definitions of small_gicp_amd.h.
// usage: test_cpp_cloud_outliers points.f32   (raw float32 xyz triples)
// The cloud is preprocessed by the header's own call (voxel grid, tree, covariances), then filtered with the caller's tree and with a
// temporary one.
//   OUTLIERS <mode> kept <m> of <n> equal <0|1> band <b> relerr <e> gathered <0|1> tree <0|1>
//       equal: kept[] is the host loop's list but for the b points whose statistic lies within 1e-5 of the threshold; relerr: the largest
//       relative error of stat[], mean, stddev and threshold; gathered: record j is input record kept[j] bit for bit (point, covariance);
//       tree: the call with a temporary tree gives the same kept[] and stat[]
//   REFUSE equal <0|1>   k = 64 throws and names the range
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

struct HostResult {
  std::vector<double> stat;
  double mean = 0, stddev = 0, threshold = 0;
  std::vector<int64_t> kept;
};

static HostResult host_filter(const PointCloud& in, const sga_outlier_filter& f) {
  const size_t n = in.size();
  HostResult r;
  r.stat.resize(n);
  std::vector<std::array<double, 4>> p(n);
  for (size_t i = 0; i < n; i++) p[i] = in.point(i);
  const size_t kp = std::min<size_t>(f.k, n - 1);
  std::vector<double> d(n);
  for (size_t i = 0; i < n; i++) {
    for (size_t j = 0; j < n; j++) {
      const double x = p[i][0] - p[j][0], y = p[i][1] - p[j][1], z = p[i][2] - p[j][2];
      d[j] = std::sqrt(x * x + y * y + z * z);
    }
    std::partial_sort(d.begin(), d.begin() + kp + 1, d.end());
    if (f.mode == 0) {
      double s = 0;
      for (size_t j = 0; j <= kp; j++) s += d[j];
      r.stat[i] = kp > 0 ? s / kp : 0.0;
    } else {
      r.stat[i] = n > static_cast<size_t>(f.k) ? d[f.k] : INFINITY;
    }
  }
  for (double v : r.stat) r.mean += v;
  r.mean /= n;
  double q = 0;
  for (double v : r.stat) q += (v - r.mean) * (v - r.mean);
  r.stddev = n > 1 ? std::sqrt(q / (n - 1)) : 0.0;
  r.threshold = f.mode == 0 ? r.mean + f.std_mul * r.stddev : f.radius;
  for (size_t i = 0; i < n; i++)
    if (r.stat[i] <= r.threshold) r.kept.push_back(static_cast<int64_t>(i));
  return r;
}

static double rel(double a, double b) { return std::fabs(a - b) / std::max(std::fabs(b), 1e-300); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
    auto [cloud, tree] = preprocess_points(pts, 0.5, 10);
    const OutlierFilter filters[2] = {OutlierFilter::statistical(10, 1.0), OutlierFilter::within_radius(4, 1.0)};
    for (const OutlierFilter& f : filters) {
      std::vector<int64_t> kept, kept2;
      std::vector<double> stat, stat2;
      sga_outlier_stats st;
      const PointCloud::Ptr out = cloud->without_outliers(f, tree->h, &kept, &stat, &st);
      const PointCloud::Ptr out2 = cloud->without_outliers(f, nullptr, &kept2, &stat2);
      const HostResult want = host_filter(*cloud, f);
      double err = std::max(rel(st.mean, want.mean), std::max(rel(st.stddev, want.stddev), rel(st.threshold, want.threshold)));
      for (size_t i = 0; i < stat.size(); i++) err = std::max(err, rel(stat[i], want.stat[i]));
      int band = 0;
      std::vector<char> got(cloud->size(), 0);
      for (int64_t i : kept) got[static_cast<size_t>(i)] = 1;
      bool equal = st.kept == kept.size() && out->size() == kept.size() && std::is_sorted(kept.begin(), kept.end());
      for (size_t i = 0; i < cloud->size(); i++) {
        const bool in_band = std::fabs(want.stat[i] - want.threshold) <= 1e-5 * want.threshold;
        band += in_band ? 1 : 0;
        if (!in_band && (got[i] != 0) != (want.stat[i] <= want.threshold)) equal = false;
      }
      bool gathered = out->has_covs() == cloud->has_covs();
      for (size_t j = 0; gathered && j < kept.size(); j++) {
        const size_t i = static_cast<size_t>(kept[j]);
        gathered = cloud->point(i) == out->point(j) && cloud->cov(i) == out->cov(j);
      }
      const bool same = kept2 == kept && stat2.size() == stat.size() && std::memcmp(stat2.data(), stat.data(), stat.size() * sizeof(double)) == 0 && out2->size() == out->size();
      std::printf("OUTLIERS %d kept %zu of %zu equal %d band %d relerr %.3e gathered %d tree %d\n", f.mode, out->size(), cloud->size(), equal ? 1 : 0, band, err, gathered ? 1 : 0, same ? 1 : 0);
    }
    bool refused = false;
    try {
      cloud->without_outliers(OutlierFilter::statistical(64));
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "[1,63]") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

// PointCloud::segment_plane with PlaneParams and segment_planes (include/small_gicp_amd.hpp: sga_cloud_segment_plane) on a file of points:
// the test holds what is printed here against the Python layer's answers on the same file (tests/test_cloud_plane_gpu.py).
// usage: test_cpp_cloud_plane points.f32   (raw float32 xyz triples)
//   PLANE best <h> hypothesis_inliers <k> inliers <i> scored <s> refit <r> plane <nx> <ny> <nz> <d> rmse <e>     (%.17g)
//   KEEP plane <points> rest <points> partition <0|1> scores <0|1>
//       partition: the two kept lists are ascending, disjoint and cover the cloud, the plane's cloud has `inliers` points and the kept
//       records are the cloud's, bit for bit; scores: the best hypothesis is the lowest h with the greatest score among those not dropped
//   PLANES count <c> sizes <n0> <n1> ... rest <m> labelled <0|1>      labelled: the labels' counts are the planes' inliers
//   REFUSE equal <0|1>   iterations = 0 throws and names it
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
    auto cloud = std::make_shared<PointCloud>(pts);
    const size_t n = cloud->size();
    PlaneParams q(0.05, 300, 7);
    const Plane got = cloud->segment_plane(q, true);
    std::printf("PLANE best %llu hypothesis_inliers %llu inliers %llu scored %llu refit %d plane %.17g %.17g %.17g %.17g rmse %.17g\n", static_cast<unsigned long long>(got.result.best_hypothesis),
                static_cast<unsigned long long>(got.result.hypothesis_inliers), static_cast<unsigned long long>(got.result.inliers), static_cast<unsigned long long>(got.result.scored), got.result.refit, got.coefficients[0],
                got.coefficients[1], got.coefficients[2], got.coefficients[3], got.result.rmse);
    {
      PlaneParams on = q, off = q;
      on.keep = PlaneParams::Plane, off.keep = PlaneParams::Rest;
      const Plane a = cloud->segment_plane(on), b = cloud->segment_plane(off);
      std::vector<int64_t> all(a.kept);
      all.insert(all.end(), b.kept.begin(), b.kept.end());
      std::sort(all.begin(), all.end());
      bool partition = std::is_sorted(a.kept.begin(), a.kept.end()) && std::is_sorted(b.kept.begin(), b.kept.end()) && all.size() == n && a.cloud->size() == got.result.inliers && a.kept.size() == a.cloud->size() &&
                       b.kept.size() == b.cloud->size() && a.coefficients == got.coefficients && b.coefficients == got.coefficients;
      for (size_t i = 0; partition && i < n; i++) partition = all[i] == static_cast<int64_t>(i);
      for (size_t j = 0; partition && j < a.kept.size(); j++) partition = cloud->point(static_cast<size_t>(a.kept[j])) == a.cloud->point(j);
      for (size_t j = 0; partition && j < b.kept.size(); j++) partition = cloud->point(static_cast<size_t>(b.kept[j])) == b.cloud->point(j);
      size_t best = got.scores.size();
      for (size_t h = 0; h < got.scores.size(); h++)
        if (got.scores[h] != 0xFFFFFFFFu && (best == got.scores.size() || got.scores[h] > got.scores[best])) best = h;
      const bool scores = got.scores.size() == q.iterations && best == got.result.best_hypothesis && got.scores[best] == got.result.hypothesis_inliers;
      std::printf("KEEP plane %zu rest %zu partition %d scores %d\n", a.cloud->size(), b.cloud->size(), partition ? 1 : 0, scores ? 1 : 0);
    }
    {
      PlaneParams many(0.05, 300, 7);
      many.min_inliers = 200;
      const Planes found = segment_planes(cloud, 6, many);
      std::printf("PLANES count %zu sizes", found.planes.size());
      bool labelled = found.labels.size() == n && found.rest && found.rest->size() == found.rest_indices.size();
      for (size_t r = 0; r < found.planes.size(); r++) {
        std::printf(" %llu", static_cast<unsigned long long>(found.planes[r].result.inliers));
        labelled = labelled && static_cast<uint64_t>(std::count(found.labels.begin(), found.labels.end(), static_cast<int32_t>(r))) == found.planes[r].result.inliers;
      }
      labelled = labelled && static_cast<size_t>(std::count(found.labels.begin(), found.labels.end(), -1)) == found.rest_indices.size();
      for (size_t j = 0; labelled && j < found.rest_indices.size(); j++) labelled = found.labels[static_cast<size_t>(found.rest_indices[j])] == -1;
      std::printf(" rest %zu labelled %d\n", found.rest_indices.size(), labelled ? 1 : 0);
    }
    bool refused = false;
    try {
      cloud->segment_plane(PlaneParams(0.05, 0));
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "iterations must be in [1, 2^20]") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

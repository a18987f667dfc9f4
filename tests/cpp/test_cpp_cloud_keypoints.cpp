// PointCloud::iss_keypoints with IssParams and Features::selected (include/small_gicp_amd.hpp: sga_cloud_iss_keypoints,
// sga_features_select) against host loops: rule 4 of small_gicp_amd.h over brute-force squared distances in double and the saliencies
// the call reports, and a gather of the downloaded rows.
// usage: test_cpp_cloud_keypoints points.f32 salient_radius non_max_radius   (raw float32 xyz triples)
// The cloud is preprocessed by the header's own call (voxel grid 0.25 m, tree, normals and covariances).
//   KEYPOINTS points <n> count <c> first <i> last <j> salient <s> nms <0|1> tree <0|1> keep <0|1>
//       salient: points with a saliency above zero; nms: the indices are those the host loop finds from the saliencies; tree: the call
//       with a temporary tree gives the same bytes; keep: the cloud holds exactly the keypoints, in order, bit for bit
//   SELECT rows <c> dim <d> equal <0|1>   the selected rows are the rows at the keypoints' indices, bit for bit; repeats too
//   REFUSE gamma <0|1> index <0|1>   gamma_21 = 0 and an index outside the rows throw and say so
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
    const double salient_radius = std::atof(argv[2]), non_max_radius = std::atof(argv[3]);
    auto [cloud, tree] = preprocess_points(pts, 0.25, 10);
    const size_t n = cloud->size();
    std::vector<std::array<double, 4>> p(n);
    for (size_t i = 0; i < n; i++) p[i] = cloud->point(i);
    const IssParams q(salient_radius, non_max_radius, true);
    const Keypoints got = cloud->iss_keypoints(q, tree->h, true), again = cloud->iss_keypoints(q, nullptr, true);
    const Keypoints bare = cloud->iss_keypoints(IssParams(salient_radius, non_max_radius), tree->h);
    // rule 4 on the host, from the saliencies the device reports
    const double r2 = non_max_radius * non_max_radius;
    std::vector<int64_t> want;
    size_t salient = 0;
    for (size_t i = 0; i < n; i++) {
      const double own = got.saliency[i];
      if (!(own > 0.0)) continue;
      salient++;
      int window = 0;
      bool beaten = false;
      for (size_t j = 0; j < n; j++) {
        const double x = p[i][0] - p[j][0], y = p[i][1] - p[j][1], z = p[i][2] - p[j][2];
        if (!(x * x + y * y + z * z <= r2)) continue;
        window++;
        if (j != i && (got.saliency[j] > own || (got.saliency[j] == own && j < i))) beaten = true;
      }
      if (!beaten && window >= q.min_neighbors) want.push_back(static_cast<int64_t>(i));
    }
    const bool nms = got.indices == want;
    const bool same = again.indices == got.indices && again.saliency.size() == n && std::memcmp(again.saliency.data(), got.saliency.data(), n * sizeof(double)) == 0 && bare.indices == got.indices && !bare.cloud &&
                      bare.saliency.empty();
    bool keep = got.cloud && got.cloud->size() == got.indices.size() && again.cloud && again.cloud->size() == got.indices.size() && got.cloud->has_covs() == cloud->has_covs();
    for (size_t j = 0; keep && j < got.indices.size(); j++) {
      const size_t i = static_cast<size_t>(got.indices[j]);
      keep = cloud->point(i) == got.cloud->point(j) && cloud->cov(i) == got.cloud->cov(j);
    }
    std::printf("KEYPOINTS points %zu count %zu first %lld last %lld salient %zu nms %d tree %d keep %d\n", n, got.indices.size(), got.indices.empty() ? -1ll : static_cast<long long>(got.indices.front()),
                got.indices.empty() ? -1ll : static_cast<long long>(got.indices.back()), salient, nms ? 1 : 0, same ? 1 : 0, keep ? 1 : 0);
    {
      const Features::Ptr all = cloud->fpfh(tree->h, 10);
      std::vector<int64_t> idx = got.indices;
      idx.insert(idx.end(), got.indices.begin(), got.indices.end());  // every keypoint twice: repeats are allowed
      const Features::Ptr some = all->selected(idx);
      const std::vector<float> rows = all->download(), sel = some->download();
      const size_t d = static_cast<size_t>(all->dim());
      bool equal = some->size() == idx.size() && some->dim() == all->dim() && sel.size() == idx.size() * d;
      for (size_t j = 0; equal && j < idx.size(); j++) equal = std::memcmp(&sel[j * d], &rows[static_cast<size_t>(idx[j]) * d], d * sizeof(float)) == 0;
      const Features::Ptr none = all->selected({});
      equal = equal && none->size() == 0 && none->dim() == all->dim();
      std::printf("SELECT rows %zu dim %d equal %d\n", some->size(), some->dim(), equal ? 1 : 0);
      bool gamma = false, index = false;
      try {
        IssParams bad(salient_radius, non_max_radius);
        bad.gamma_21 = 0.0;
        cloud->iss_keypoints(bad);
      } catch (const std::exception& e) {
        gamma = std::strstr(e.what(), "gamma_21 must be in (0, 1]") != nullptr;
      }
      try {
        all->selected({0, static_cast<int64_t>(n)});
      } catch (const std::exception& e) {
        index = std::strstr(e.what(), "indices[1]") != nullptr;
      }
      std::printf("REFUSE gamma %d index %d\n", gamma ? 1 : 0, index ? 1 : 0);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

// create_gaussian_voxelmaps (include/small_gicp_amd.hpp: sga_index_build_gaussian_voxelmap_batch) against create_gaussian_voxelmap and
// against the lone one-shot build, per member.
// usage: test_cpp_voxelmaps_batch points.f32   (raw float32 xyz triples)
// Members: slices of the file of different length, preprocessed by the header's own calls.  Per member one line
//   MEMBER k voxels <batch> <helper> <lone> exact <0|1> coords <0|1> mean_err <max |batch - helper| / scale> cov_err <max |batch - helper|>
// `exact`: every downloaded array of the batch-built map equals the lone sga_index_build_gaussian_voxelmap's bit for bit; `coords`: voxel
// coordinates and counts equal create_gaussian_voxelmap's (an incremental map after one insert: same voxels in the same order, fp64
// state exported as fp32 — the two may round a mean differently in its last bit, so the caller applies the tolerance).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

struct Voxels {
  std::vector<int32_t> coords;
  std::vector<float> means, cov6;
  std::vector<uint32_t> counts;
};

static Voxels download(sga_context* ctx, const sga_index* h) {
  size_t n = 0;
  check(sga_index_size(h, &n), "sga_index_size");
  Voxels v;
  v.coords.resize(3 * n), v.means.resize(3 * n), v.cov6.resize(6 * n), v.counts.resize(n);
  check(sga_index_voxelmap_download(ctx, h, v.coords.data(), v.means.data(), v.cov6.data(), v.counts.data()), "sga_index_voxelmap_download");
  return v;
}

template <typename T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);

    const size_t lengths[4] = {pts.size(), pts.size() / 2, 65, pts.size() / 3};
    std::vector<PointCloud::Ptr> keep;
    std::vector<std::shared_ptr<const PointCloud>> clouds;
    for (size_t len : lengths) {
      std::vector<std::array<float, 3>> part(pts.begin(), pts.begin() + len);
      auto [cloud, tree] = preprocess_points(part, 0.25, 10);
      keep.push_back(cloud);
      clouds.push_back(cloud);
    }
    sga_context* ctx = clouds[0]->ctx;
    const double leaf = 1.0;
    const auto maps = create_gaussian_voxelmaps(ctx, clouds, leaf);
    if (maps.size() != clouds.size()) throw std::runtime_error("create_gaussian_voxelmaps returned another number of maps");
    for (size_t k = 0; k < clouds.size(); k++) {
      const auto helper = create_gaussian_voxelmap(*clouds[k], leaf);
      sga_index* lone = nullptr;
      check(sga_index_build_gaussian_voxelmap(ctx, clouds[k]->h, leaf, &lone), "sga_index_build_gaussian_voxelmap");
      const Voxels b = download(ctx, maps[k]->h), h = download(ctx, helper->h), l = download(ctx, lone);
      size_t nl = 0;
      sga_index_size(lone, &nl);
      sga_index_destroy(lone);
      const bool exact = same_bits(b.coords, l.coords) && same_bits(b.means, l.means) && same_bits(b.cov6, l.cov6) && same_bits(b.counts, l.counts);
      const bool coords = same_bits(b.coords, h.coords) && same_bits(b.counts, h.counts);
      double mean_err = 0, cov_err = 0, scale = 1.0;
      if (coords) {
        for (float v : h.means) scale = std::fmax(scale, std::fabs(static_cast<double>(v)));
        for (size_t i = 0; i < b.means.size(); i++) mean_err = std::fmax(mean_err, std::fabs(static_cast<double>(b.means[i]) - h.means[i]));
        for (size_t i = 0; i < b.cov6.size(); i++) cov_err = std::fmax(cov_err, std::fabs(static_cast<double>(b.cov6[i]) - h.cov6[i]));
      }
      // the batch-built map serves a search like the helper's
      size_t ib = 0, ih = 0;
      double db = 0, dh = 0;
      const double q[3] = {b.means.empty() ? 0.0 : b.means[0], b.means.empty() ? 0.0 : b.means[1], b.means.empty() ? 0.0 : b.means[2]};
      const size_t fb = maps[k]->nearest_neighbor_search(q, &ib, &db), fh = helper->nearest_neighbor_search(q, &ih, &dh);
      std::printf("MEMBER %zu voxels %zu %zu %zu exact %d coords %d mean_err %.3e cov_err %.3e search %d\n", k, maps[k]->size(), helper->size(), nl, exact ? 1 : 0, coords ? 1 : 0, mean_err / scale, cov_err,
                  (fb == fh && ib == ih) ? 1 : 0);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}

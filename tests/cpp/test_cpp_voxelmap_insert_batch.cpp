// insert_batch (include/small_gicp_amd.hpp: sga_voxelmap_insert_batch) against GaussianVoxelMap::insert, per member.
// usage: test_cpp_voxelmap_insert_batch points.f32   (raw float32 xyz triples)
// Members: slices of the file of different length, preprocessed by the header's own calls; three rounds, each at another pose (rotation
// about z plus translation), the members' clouds rotated by one place per round.  Per member one line after the last round
//   MEMBER k voxels <batch> <lone> equal <0|1>
// `equal`: after EVERY round every downloaded array of the batch-inserted map equalled the lone-inserted twin's bit for bit.
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

static Isometry3d pose(double yaw, double x, double y, double z) {
  Isometry3d T;
  T(0, 0) = std::cos(yaw), T(0, 1) = -std::sin(yaw), T(1, 0) = std::sin(yaw), T(1, 1) = std::cos(yaw);
  T(0, 3) = x, T(1, 3) = y, T(2, 3) = z;
  return T;
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
    std::vector<std::shared_ptr<const PointCloud>> clouds;
    for (size_t len : lengths) {
      std::vector<std::array<float, 3>> part(pts.begin(), pts.begin() + len);
      auto [cloud, tree] = preprocess_points(part, 0.25, 10);
      clouds.push_back(cloud);
    }
    sga_context* ctx = clouds[0]->ctx;
    const size_t B = clouds.size();
    std::vector<GaussianVoxelMap::Ptr> batch, lone;
    for (size_t k = 0; k < B; k++) {
      batch.push_back(std::make_shared<GaussianVoxelMap>(k % 2 ? 0.5 : 1.0));
      lone.push_back(std::make_shared<GaussianVoxelMap>(k % 2 ? 0.5 : 1.0));
      batch[k]->lru_horizon = lone[k]->lru_horizon = 1;
      batch[k]->lru_clear_cycle = lone[k]->lru_clear_cycle = 2 + k % 2;  // some members sweep in round 2, some in round 3
    }
    std::vector<bool> equal(B, true);
    for (int round = 0; round < 3; round++) {
      std::vector<std::shared_ptr<const PointCloud>> now;
      std::vector<Isometry3d> Ts;
      for (size_t k = 0; k < B; k++) {
        now.push_back(clouds[(k + round) % B]);
        Ts.push_back(pose(0.03 * (round + 1) + 0.01 * k, 4.5 * round + 0.3, -2.0 * round + 0.1 * k, 0.05 * round));
      }
      insert_batch(ctx, batch, now, Ts);
      for (size_t k = 0; k < B; k++) {
        lone[k]->insert(*now[k], Ts[k]);
        const Voxels b = download(ctx, batch[k]->h), l = download(ctx, lone[k]->h);
        equal[k] = equal[k] && same_bits(b.coords, l.coords) && same_bits(b.means, l.means) && same_bits(b.cov6, l.cov6) && same_bits(b.counts, l.counts);
      }
    }
    for (size_t k = 0; k < B; k++) std::printf("MEMBER %zu voxels %zu %zu equal %d\n", k, batch[k]->size(), lone[k]->size(), equal[k] ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}

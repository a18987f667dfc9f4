// Features, PointCloud::fpfh, match_features and ransac_correspondences of include/small_gicp_amd.hpp, end to end:
// two clouds that share no initial guess are preprocessed by the header's own call, described, matched, registered coarsely and refined
// by align() from the coarse pose.
// usage: test_cpp_global_registration target.f32 source.f32 voxel seed   (raw float32 xyz triples)
//   FEATURES rows <n> dim <d> roundtrip <0|1> sums <0|1>
//       roundtrip: a Features made from the downloaded rows matches the original row for row at distance 0; sums: every sub-histogram
//       of every row sums to 100 within 33 fp32 ulps, or is zero
//   GLOBAL pairs <M> inliers <I> best <h> scored <s> refit <r> rmse <e>
//   COARSE <16 doubles, column-major>
//   REFINED converged <0|1> <16 doubles, column-major>
//   REFUSE k <0|1> pairs <0|1>   k = 1 and a pair outside the clouds throw and name the reason
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

static std::vector<std::array<float, 3>> read_points(const char* path) {
  std::ifstream ifs(path, std::ios::binary | std::ios::ate);
  if (!ifs) throw std::runtime_error("cannot open the points file");
  std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
  ifs.seekg(0);
  ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
  return pts;
}

static void print_pose(const Isometry3d& T) {
  for (int k = 0; k < 16; k++) std::printf(" %.17g", T.data()[k]);
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  try {
    const double voxel = std::atof(argv[3]);
    auto [target, target_tree] = preprocess_points(read_points(argv[1]), voxel, 20);
    auto [source, source_tree] = preprocess_points(read_points(argv[2]), voxel, 20);
    const std::array<double, 3> above{0.0, 0.0, 50.0};
    const Features::Ptr ft = target->fpfh(target_tree->h, 20, &above), fs = source->fpfh(source_tree->h, 20, &above);

    const std::vector<float> rows = fs->download();
    const Features copy(rows.data(), fs->size(), fs->dim());
    std::vector<double> dist;
    const auto self = match_features(*fs, copy, false, &dist);
    bool roundtrip = self.size() == fs->size() && fs->dim() == SGA_FPFH_DIM && fs->size() == source->size();
    for (size_t i = 0; roundtrip && i < self.size(); i++) roundtrip = dist[i] == 0.0 && std::memcmp(&rows[self[i][1] * SGA_FPFH_DIM], &rows[i * SGA_FPFH_DIM], SGA_FPFH_DIM * sizeof(float)) == 0;
    bool sums = true;
    for (size_t i = 0; i < fs->size(); i++)
      for (int g = 0; g < 3; g++) {
        double s = 0;
        for (int b = 0; b < 11; b++) s += rows[i * SGA_FPFH_DIM + 11 * g + b];
        sums = sums && (s == 0.0 || std::fabs(s - 100.0) <= 33 * 7.62939453125e-06);
      }
    std::printf("FEATURES rows %zu dim %d roundtrip %d sums %d\n", fs->size(), fs->dim(), roundtrip ? 1 : 0, sums ? 1 : 0);

    const auto pairs = match_features(*fs, *ft, true);
    Ransac params;
    params.max_distance = 1.5 * voxel;
    params.min_edge = 2.0 * voxel;
    params.seed = static_cast<uint64_t>(std::atoll(argv[4]));
    const RansacResult coarse = ransac_correspondences(*source, *target, pairs, params);
    std::printf("GLOBAL pairs %zu inliers %llu best %llu scored %llu refit %d rmse %.17g\n", pairs.size(), static_cast<unsigned long long>(coarse.inliers), static_cast<unsigned long long>(coarse.best_hypothesis),
                static_cast<unsigned long long>(coarse.scored), coarse.refit, coarse.inlier_rmse);
    std::printf("COARSE");
    print_pose(coarse.T_target_source);
    const RegistrationResult refined = align(*target, *source, *target_tree, coarse.T_target_source);
    std::printf("REFINED converged %d", refined.converged ? 1 : 0);
    print_pose(refined.T_target_source);

    bool refused_k = false, refused_pairs = false;
    try {
      source->fpfh(nullptr, 1);
    } catch (const std::exception& e) {
      refused_k = std::strstr(e.what(), "[2,63]") != nullptr;
    }
    try {
      ransac_correspondences(*source, *target, {{0, 0}, {1, 1}, {static_cast<int64_t>(source->size()), 2}});
    } catch (const std::exception& e) {
      refused_pairs = std::strstr(e.what(), "pairs[2] names source point") != nullptr;
    }
    std::printf("REFUSE k %d pairs %d\n", refused_k ? 1 : 0, refused_pairs ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

// Point-to-plane ICP against a ProjectiveSearch target through the header-only C++ layer: Registration<PointToPlaneICPFactor,
// ParallelReductionHIP>::align(target, source, ProjectiveSearch, init_T) with the public search window changed after construction
// (ann/projective_search.hpp:153-154), and the index's nearest_neighbor_search / knn_search.
// usage: test_cpp_projective target.f32 target_normals.f32 source.f32 init.f64   (raw float32 xyz triples; init: column-major 4x4)
//        -> "NN <index> <sq_dist>", "KNN <k found> <indices>", "POSE <iterations> <16 column-major entries>" on stdout
#include <cstdio>
#include <fstream>
#include <memory>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

template <typename T>
static std::vector<T> read_raw(const char* path) {
  std::ifstream ifs(path, std::ios::binary | std::ios::ate);
  if (!ifs) throw std::runtime_error(std::string("cannot open ") + path);
  const size_t bytes = ifs.tellg();
  std::vector<T> v(bytes / sizeof(T));
  ifs.seekg(0);
  ifs.read(reinterpret_cast<char*>(v.data()), v.size() * sizeof(T));
  return v;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  try {
    const auto tp = read_raw<float>(argv[1]);
    const auto tn = read_raw<float>(argv[2]);
    const auto sp = read_raw<float>(argv[3]);
    const auto init = read_raw<double>(argv[4]);
    if (tn.size() != tp.size() || init.size() != 16 || sp.size() < 3) return 2;
    auto target = std::make_shared<PointCloud>(tp.data(), tn.data(), nullptr, tp.size() / 3);
    PointCloud source(sp.data(), nullptr, nullptr, sp.size() / 3);
    ProjectiveSearch search(1024, 64, target);
    search.search_window_h = 8;
    search.search_window_v = 3;
    const double q[3] = {sp[0], sp[1], sp[2]};
    size_t idx[5];
    double d2[5];
    if (search.nearest_neighbor_search(q, idx, d2) == 1)
      std::printf("NN %zu %.17g\n", idx[0], d2[0]);
    else
      std::printf("NN -1 inf\n");
    const size_t found = search.knn_search(q, 5, idx, d2);
    std::printf("KNN %zu", found);
    for (size_t j = 0; j < found; j++) std::printf(" %zu", idx[j]);
    std::printf("\n");
    Isometry3d T0;
    for (int i = 0; i < 16; i++) T0.m[i] = init[i];
    Registration<PointToPlaneICPFactor, ParallelReductionHIP> reg;
    const RegistrationResult r = reg.align(*target, source, search, T0);
    std::printf("POSE %zu", r.iterations);
    for (int i = 0; i < 16; i++) std::printf(" %.17g", r.T_target_source.m[i]);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}

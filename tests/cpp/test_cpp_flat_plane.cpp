// Scan-to-model point-to-plane ICP through the header-only C++ layer: Registration<PointToPlaneICPFactor, ParallelReductionHIP> against
// IncrementalVoxelMap<FlatContainerNormal> (ann/flat_container.hpp:15-17: the linear iVox of Faster-LIO).
// usage: test_cpp_flat_plane target.f32 target_normals.f32 source.f32 init.f64   (raw float32 xyz triples; init: column-major 4x4)
//        -> "POSE <iterations> <16 column-major entries>" on stdout
#include <cstdio>
#include <fstream>
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
    if (tn.size() != tp.size() || init.size() != 16) return 2;
    PointCloud target(tp.data(), tn.data(), nullptr, tp.size() / 3);
    PointCloud source(sp.data(), nullptr, nullptr, sp.size() / 3);
    IncrementalVoxelMap<FlatContainerNormal> model(1.0);
    model.set_search_offsets(7);
    model.insert(target);
    Isometry3d T0;
    for (int i = 0; i < 16; i++) T0.m[i] = init[i];
    Registration<PointToPlaneICPFactor, ParallelReductionHIP> reg;
    const RegistrationResult r = reg.align(model, source, model, T0);
    std::printf("POSE %zu", r.iterations);
    for (int i = 0; i < 16; i++) std::printf(" %.17g", r.T_target_source.m[i]);
    std::printf("\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}

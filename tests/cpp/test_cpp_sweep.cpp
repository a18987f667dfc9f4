// align_sweep with SweepParams (include/small_gicp_amd.hpp) over the C-ABI call it wraps (sga_align_sweep): the pose and the twist of a
// raw sweep against a snapshot, from the identity and a zero twist.
// usage: test_cpp_sweep target.f32 source.f32 times.f32   (raw float32 xyz triples; one float32 time per source point)
// Both clouds are uploaded as they are and get covariances from 10 neighbours (the target with its tree).
//   POSE <16 doubles as hex floats, column-major>
//   TWIST <6 doubles as hex floats>
//   RESULT converged <0|1> iterations <i> inliers <n> symmetric <0|1>     symmetric: H is 12 x 12 and symmetric, bit for bit
//   PRIOR moved <0|1>   a stiff prior (information 1e12 I) centred on 0 keeps the twist within 1e-6 of 0, where the free twist is not
//   REFUSE times <0|1>  a times vector of another size throws
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

template <typename T>
static std::vector<T> read_all(const char* path) {
  std::ifstream ifs(path, std::ios::binary | std::ios::ate);
  if (!ifs) throw std::runtime_error(std::string("cannot open ") + path);
  std::vector<T> v(static_cast<size_t>(ifs.tellg()) / sizeof(T));
  ifs.seekg(0);
  ifs.read(reinterpret_cast<char*>(v.data()), v.size() * sizeof(T));
  return v;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  try {
    const auto tp = read_all<std::array<float, 3>>(argv[1]);
    const auto sp = read_all<std::array<float, 3>>(argv[2]);
    const auto times = read_all<float>(argv[3]);
    auto target = std::make_shared<PointCloud>(tp);
    auto source = std::make_shared<PointCloud>(sp);
    KdTree tree(target);
    estimate_covariances(*target, tree, 10);
    estimate_covariances(*source, 10);
    const SweepResult r = align_sweep(*target, *source, times, tree);
    std::printf("POSE");
    for (int k = 0; k < 16; k++) std::printf(" %a", r.T_target_source.data()[k]);
    std::printf("\nTWIST");
    for (int k = 0; k < 6; k++) std::printf(" %a", r.twist[k]);
    bool symmetric = true;
    for (int i = 0; i < 12; i++)
      for (int j = 0; j < 12; j++) symmetric = symmetric && std::memcmp(&r.H[12 * i + j], &r.H[12 * j + i], sizeof(double)) == 0;
    std::printf("\nRESULT converged %d iterations %zu inliers %zu symmetric %d\n", r.converged ? 1 : 0, r.iterations, r.num_inliers, symmetric ? 1 : 0);
    SweepParams stiff;
    for (int k = 0; k < 6; k++) stiff.twist_information[7 * k] = 1e12;
    const SweepResult held = align_sweep(*target, *source, times, tree, Isometry3d::Identity(), stiff);
    double free_norm = 0.0, held_norm = 0.0;
    for (int k = 0; k < 6; k++) free_norm += r.twist[k] * r.twist[k], held_norm += held.twist[k] * held.twist[k];
    std::printf("PRIOR moved %d\n", (std::sqrt(held_norm) < 1e-6 && std::sqrt(free_norm) > 1e-2) ? 1 : 0);
    bool refused = false;
    try {
      std::vector<float> fewer(times.begin(), times.end() - 1);
      align_sweep(*target, *source, fewer, tree);
    } catch (const std::exception&) {
      refused = true;
    }
    std::printf("REFUSE times %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

// create_problems (include/small_gicp_amd.hpp: sga_problem_create_batch) against sga_problem_create, per member.
// usage: test_cpp_problem_batch points.f32   (raw float32 xyz triples)
// Members: slices of the file of different length, preprocessed by the header's own calls, each at a pose of its own (rotation about z
// plus translation); even members against the kd-tree of the whole file, odd members against its 1 m Gaussian voxel map.  Per member
//   MEMBER k points <n> equal <0|1>
// `equal`: the engine's source order (sga_problem_get_sorted_points), one linearization (H, b, e, inliers) and the result of
// sga_align_problem equal the lone twin's bit for bit.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"
#include "small_gicp_amd_debug.h"

using namespace small_gicp_amd;

static Isometry3d pose(double yaw, double x, double y, double z) {
  Isometry3d T;
  T(0, 0) = std::cos(yaw), T(0, 1) = -std::sin(yaw), T(1, 0) = std::sin(yaw), T(1, 1) = std::cos(yaw);
  T(0, 3) = x, T(1, 3) = y, T(2, 3) = z;
  return T;
}

struct Outcome {
  std::vector<float> order;
  double H[36], b[6], e;
  uint64_t inliers;
  sga_result res;
};

static Outcome run(sga_context* ctx, sga_problem* pb, size_t n, const Isometry3d& T) {
  Outcome o;
  std::memset(&o.res, 0, sizeof(o.res));
  o.order.resize(4 * n);
  check(sga_problem_get_sorted_points(ctx, pb, o.order.data()), "sga_problem_get_sorted_points");
  sga_registration_setting s;
  sga_registration_setting_default(&s);
  check(sga_linearize(ctx, pb, &s.factor, T.data(), o.H, o.b, &o.e, &o.inliers), "sga_linearize");
  check(sga_align_problem(ctx, pb, T.data(), &s, &o.res), "sga_align_problem");
  return o;
}

static bool same(const Outcome& a, const Outcome& b) {
  return a.order.size() == b.order.size() && std::memcmp(a.order.data(), b.order.data(), a.order.size() * sizeof(float)) == 0 && std::memcmp(a.H, b.H, sizeof(a.H)) == 0 && std::memcmp(a.b, b.b, sizeof(a.b)) == 0 &&
         std::memcmp(&a.e, &b.e, sizeof(double)) == 0 && a.inliers == b.inliers && std::memcmp(a.res.T_target_source, b.res.T_target_source, sizeof(a.res.T_target_source)) == 0 && a.res.converged == b.res.converged &&
         a.res.iterations == b.res.iterations;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);

    auto [target, tree] = preprocess_points(pts, 0.25, 10);
    auto map = create_gaussian_voxelmap(*target, 1.0);
    sga_context* ctx = target->ctx;
    const size_t lengths[4] = {pts.size(), pts.size() / 2, 65 * 40, pts.size() / 3};
    std::vector<std::shared_ptr<const PointCloud>> sources;
    std::vector<const sga_index*> targets;
    std::vector<Isometry3d> Ts;
    for (size_t k = 0; k < 4; k++) {
      std::vector<std::array<float, 3>> part(pts.begin(), pts.begin() + lengths[k]);
      auto [cloud, unused] = preprocess_points(part, 0.25, 10);
      (void)unused;
      sources.push_back(cloud);
      targets.push_back(k % 2 ? map->h : tree->h);
      Ts.push_back(pose(0.01 * (k + 1), 0.05 * k, -0.03 * k, 0.01));
    }
    Problems batch = create_problems(ctx, targets, sources, Ts);
    for (size_t k = 0; k < batch.size(); k++) {
      sga_problem* lone = nullptr;
      check(sga_problem_create(ctx, targets[k], sources[k]->h, Ts[k].data(), &lone), "sga_problem_create");
      const size_t n = sources[k]->size();
      const Outcome a = run(ctx, batch[k], n, Ts[k]), b = run(ctx, lone, n, Ts[k]);
      sga_problem_destroy(lone);
      std::printf("MEMBER %zu points %zu equal %d\n", k, n, same(a, b) ? 1 : 0);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}

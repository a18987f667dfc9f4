// merge_clouds and PointCloud::transformed (include/small_gicp_amd.hpp: sga_cloud_merge / sga_cloud_transform) against the host loop they
// replace (src/test/registration_test.cpp:84: pt = T * pt over points; R n over normals, R C R^T over covs).
// usage: test_cpp_cloud_merge points.f32   (raw float32 xyz triples)
// Members: slices of the file of different length, preprocessed by the header's own calls (normals and covariances), one of them twice.
//   EXACT  k points <n> equal <0|1>    quarter turns about z with integer translations: the double arithmetic is exact, so every merged
//                                      point, normal and covariance equals the host loop's float(T * p), float(R n), float(R C R^T) bit for bit
//   POSED  k points <n> within <0|1>   general poses: |merged - (R r + t)| <= half a spacing of fp32 plus the double rounding of four terms
//   LONE   k equal <0|1>               transformed(T) of the member alone holds the merged cloud's stretch bit for bit
//   SHAPE  size <merged> <sum> normals <0|1> covs <0|1>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

static Isometry3d pose(double c, double s, double x, double y, double z) {
  Isometry3d T;
  T(0, 0) = c, T(0, 1) = -s, T(1, 0) = s, T(1, 1) = c;
  T(0, 3) = x, T(1, 3) = y, T(2, 3) = z;
  return T;
}

static double spacing32(double v) {
  const float f = std::fabs(static_cast<float>(v));
  return static_cast<double>(std::nextafter(f, INFINITY)) - static_cast<double>(f);
}

// member `in` under T against the stretch [off, off + n) of `out`: exact = bit equality with the host loop's rounded values
static bool member_matches(const PointCloud& in, const Isometry3d& T, const PointCloud& out, size_t off, bool exact) {
  const double eps = 2.220446049250313e-16;
  bool ok = true;
  for (size_t i = 0; i < in.size(); i++) {
    const auto p = in.point(i), n = in.normal(i), q = out.point(off + i), m = out.normal(off + i);
    const auto C = in.cov(i), D = out.cov(off + i);
    double RC[3][3];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) RC[a][b] = T(a, 0) * C[4 * b + 0] + T(a, 1) * C[4 * b + 1] + T(a, 2) * C[4 * b + 2];
    for (int a = 0; a < 3; a++) {
      const double rp = T(a, 0) * p[0] + T(a, 1) * p[1] + T(a, 2) * p[2] + T(a, 3);
      const double mag = std::fabs(T(a, 0) * p[0]) + std::fabs(T(a, 1) * p[1]) + std::fabs(T(a, 2) * p[2]) + std::fabs(T(a, 3));
      const double rn = T(a, 0) * n[0] + T(a, 1) * n[1] + T(a, 2) * n[2];
      if (exact) {
        ok = ok && static_cast<double>(static_cast<float>(rp)) == q[a] && static_cast<double>(static_cast<float>(rn)) == m[a];
      } else {
        ok = ok && std::fabs(q[a] - rp) <= 0.5 * spacing32(rp) + 64 * eps * mag && std::fabs(m[a] - rn) <= 0.5 * spacing32(rn) + 64 * eps * 3.0;
      }
      for (int b = 0; b < 3; b++) {
        const double rc = RC[a][0] * T(b, 0) + RC[a][1] * T(b, 1) + RC[a][2] * T(b, 2);
        double cmag = 0.0;
        for (int u = 0; u < 3; u++)
          for (int v = 0; v < 3; v++) cmag += std::fabs(T(a, u) * C[4 * v + u] * T(b, v));
        if (exact)
          ok = ok && static_cast<double>(static_cast<float>(rc)) == D[4 * b + a];
        else
          ok = ok && std::fabs(D[4 * b + a] - rc) <= 0.5 * spacing32(rc) + 64 * eps * cmag;
      }
    }
  }
  return ok;
}

static bool same_cloud(const PointCloud& a, const PointCloud& b, size_t off) {
  bool ok = true;
  for (size_t i = 0; i < a.size(); i++) ok = ok && a.point(i) == b.point(off + i) && a.normal(i) == b.normal(off + i) && a.cov(i) == b.cov(off + i);
  return ok;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);

    const size_t lengths[3] = {pts.size(), pts.size() / 2, pts.size() / 3};
    std::vector<std::shared_ptr<const PointCloud>> clouds;
    for (size_t len : lengths) {
      std::vector<std::array<float, 3>> part(pts.begin(), pts.begin() + len);
      auto [cloud, tree] = preprocess_points(part, 0.5, 10);
      clouds.push_back(cloud);
    }
    clouds.push_back(clouds[0]);  // one cloud twice, under two poses
    sga_context* ctx = clouds[0]->ctx;
    const size_t B = clouds.size();
    const double zero[3] = {0, 0, 0};
    const std::vector<Isometry3d> turns = {pose(1, 0, 0, 0, 0), pose(0, 1, 3, -2, 1), pose(-1, 0, -5, 4, 0), pose(0, -1, 7, 7, -2)};
    const std::vector<Isometry3d> posed = {pose(std::cos(0.3), std::sin(0.3), 1.25, -0.5, 0.1), pose(std::cos(-1.1), std::sin(-1.1), -3.0, 2.5, 0.0), pose(std::cos(2.0), std::sin(2.0), 0.0, 0.0, 0.7),
                                           pose(std::cos(0.01), std::sin(0.01), 10.0, 0.0, 0.0)};
    for (int mode = 0; mode < 2; mode++) {
      const std::vector<Isometry3d>& Ts = mode == 0 ? turns : posed;
      const PointCloud::Ptr merged = merge_clouds(ctx, clouds, Ts, zero);
      size_t off = 0;
      for (size_t k = 0; k < B; k++) {
        const bool ok = member_matches(*clouds[k], Ts[k], *merged, off, mode == 0);
        std::printf("%s %zu points %zu %s %d\n", mode == 0 ? "EXACT" : "POSED", k, clouds[k]->size(), mode == 0 ? "equal" : "within", ok ? 1 : 0);
        if (mode == 1) {
          const PointCloud::Ptr lone = clouds[k]->transformed(Ts[k], zero);
          std::printf("LONE %zu equal %d\n", k, lone->size() == clouds[k]->size() && same_cloud(*lone, *merged, off) ? 1 : 0);
        }
        off += clouds[k]->size();
      }
      if (mode == 0) std::printf("SHAPE size %zu %zu normals %d covs %d\n", merged->size(), off, merged->has_normals() ? 1 : 0, merged->has_covs() ? 1 : 0);
    }
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

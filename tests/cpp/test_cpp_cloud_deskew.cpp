// deskew_clouds, PointCloud::deskewed and se3_log (include/small_gicp_amd.hpp: sga_cloud_deskew_batch / sga_cloud_deskew / sga_se3_log)
// against a host loop: per point exp((s_i - ref) xi) in long double from the stable forms (sin, 2 sin^2(phi / 2), phi - sin phi by its
// series below 0.1), applied to the point, the normal and the covariance in double.
// usage: test_cpp_cloud_deskew points.f32   (raw float32 xyz triples)
// Members: slices of the file of different length, preprocessed by the header's own calls (normals and covariances), one of them twice.
//   DESKEW k points <n> within <0|1> worst <error / bound>   |out - ref| <= half a spacing of fp32 + 256 eps64 of the magnitudes
//   LONE   k equal <0|1>                                     deskewed() of the member alone equals the batch's member bit for bit
//   SAME   k equal <0|1>                                     a zero twist returns the input bit for bit
//   LOG    twists <n> within <0|1> worst <error / bound>     se3_exp(se3_log(T)) against T and se3_log(se3_exp(xi)) against xi
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <random>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;
typedef long double ld;

static const double kEps = 2.220446049250313e-16;

static double spacing32(double v) {
  const float f = std::fabs(static_cast<float>(v));
  return static_cast<double>(std::nextafter(f, INFINITY)) - static_cast<double>(f);
}

// (R, t) of exp(a xi), rotation first
static void exp_scaled(const std::array<double, 6>& xi, double a, double R[3][3], double t[3]) {
  const ld w[3] = {xi[0], xi[1], xi[2]}, v[3] = {xi[3], xi[4], xi[5]};
  const ld theta = sqrtl(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  ld k[3] = {0, 0, 0};
  if (theta > 0)
    for (int i = 0; i < 3; i++) k[i] = w[i] / theta;
  const ld phi = a * theta, sh = sinl(phi / 2), s1 = sinl(phi), c2 = 2 * sh * sh, q = phi * phi;
  const ld f3 = fabsl(phi) < 0.1L ? phi * q * (1 / 6.0L - q * (1 / 120.0L - q * (1 / 5040.0L - q * (1 / 362880.0L - q / 39916800.0L)))) : phi - s1;
  const ld K[3][3] = {{0, -k[2], k[1]}, {k[2], 0, -k[0]}, {-k[1], k[0], 0}};
  ld KK[3][3], kv[3], kkv[3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) KK[i][j] = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
  for (int i = 0; i < 3; i++) kv[i] = K[i][0] * v[0] + K[i][1] * v[1] + K[i][2] * v[2];
  for (int i = 0; i < 3; i++) kkv[i] = K[i][0] * kv[0] + K[i][1] * kv[1] + K[i][2] * kv[2];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[i][j] = static_cast<double>((i == j ? 1.0L : 0.0L) + s1 * K[i][j] + c2 * KK[i][j]);
    t[i] = static_cast<double>(a * v[i] + (theta > 0 ? (c2 * kv[i] + f3 * kkv[i]) / theta : 0.0L));
  }
}

static bool member_matches(const PointCloud& in, const std::vector<float>& times, const std::array<double, 6>& xi, double ref, const PointCloud& out, double* worst) {
  bool ok = in.size() == out.size() && in.has_normals() == out.has_normals() && in.has_covs() == out.has_covs();
  auto within = [&](double got, double want, double mag) {
    const double bound = 0.5 * spacing32(want) + 256 * kEps * mag;
    const double err = std::fabs(got - want);
    if (bound > 0 && err / bound > *worst) *worst = err / bound;
    return err <= bound;
  };
  for (size_t i = 0; ok && i < in.size(); i++) {
    double R[3][3], t[3];
    exp_scaled(xi, static_cast<double>(times[i]) - ref, R, t);
    const auto p = in.point(i), n = in.normal(i), q = out.point(i), m = out.normal(i);
    const auto C = in.cov(i), D = out.cov(i);
    double RC[3][3];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) RC[a][b] = R[a][0] * C[4 * b + 0] + R[a][1] * C[4 * b + 1] + R[a][2] * C[4 * b + 2];
    for (int a = 0; a < 3; a++) {
      const double rp = R[a][0] * p[0] + R[a][1] * p[1] + R[a][2] * p[2] + t[a];
      const double mag = std::fabs(R[a][0] * p[0]) + std::fabs(R[a][1] * p[1]) + std::fabs(R[a][2] * p[2]) + std::fabs(t[a]);
      const double rn = R[a][0] * n[0] + R[a][1] * n[1] + R[a][2] * n[2];
      const double nmag = std::fabs(R[a][0] * n[0]) + std::fabs(R[a][1] * n[1]) + std::fabs(R[a][2] * n[2]);
      ok = ok && within(q[a], rp, mag) && within(m[a], rn, nmag);
      for (int b = 0; b < 3; b++) {
        const double rc = RC[a][0] * R[b][0] + RC[a][1] * R[b][1] + RC[a][2] * R[b][2];
        double cmag = 0.0;
        for (int u = 0; u < 3; u++)
          for (int v = 0; v < 3; v++) cmag += std::fabs(R[a][u] * C[4 * v + u] * R[b][v]);
        ok = ok && within(D[4 * b + a], rc, cmag);
      }
    }
  }
  return ok;
}

static bool same_cloud(const PointCloud& a, const PointCloud& b) {
  bool ok = a.size() == b.size();
  for (size_t i = 0; ok && i < a.size(); i++) ok = a.point(i) == b.point(i) && a.normal(i) == b.normal(i) && a.cov(i) == b.cov(i);
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
    clouds.push_back(clouds[0]);  // one cloud twice, under two twists
    sga_context* ctx = clouds[0]->ctx;
    const size_t B = clouds.size();
    const std::vector<std::array<double, 6>> twists = {{0.0, 0.0, 0.0174, 1.0, 0.02, 0.0}, {6e-6, -8e-6, 0.0, -2.0, 1.0, 0.5}, {0.6, 0.0, -0.8, 0.5, -3.0, 0.25}, {1e-3, 2e-3, -2e-3, 0.0, 0.0, 3.0}};
    const std::vector<double> refs = {1.0, 0.5, 0.0, 1.0};
    std::vector<std::vector<float>> times(B);
    std::vector<const float*> tp;
    for (size_t k = 0; k < B; k++) {
      const size_t n = clouds[k]->size();
      times[k].resize(n);
      for (size_t i = 0; i < n; i++) times[k][i] = static_cast<float>((i * 7919 + k) % n) / static_cast<float>(n);
      tp.push_back(times[k].data());
    }
    const std::vector<PointCloud::Ptr> out = deskew_clouds(ctx, clouds, tp, twists, refs);
    for (size_t k = 0; k < B; k++) {
      double worst = 0.0;
      const bool ok = member_matches(*clouds[k], times[k], twists[k], refs[k], *out[k], &worst);
      std::printf("DESKEW %zu points %zu within %d worst %.3f\n", k, clouds[k]->size(), ok ? 1 : 0, worst);
      const PointCloud::Ptr lone = clouds[k]->deskewed(times[k].data(), twists[k], refs[k]);
      std::printf("LONE %zu equal %d\n", k, same_cloud(*lone, *out[k]) ? 1 : 0);
      const PointCloud::Ptr same = clouds[k]->deskewed(times[k].data(), {0, 0, 0, 0, 0, 0}, refs[k]);
      std::printf("SAME %zu equal %d\n", k, same_cloud(*same, *clouds[k]) ? 1 : 0);
    }

    // se3_log: the round trips, angles {0, 1e-12, 1e-8, 1e-5, 1e-3, 0.1, 1, 3} about random axes, translations up to 10 m
    const double angles[8] = {0.0, 1e-12, 1e-8, 1e-5, 1e-3, 0.1, 1.0, 3.0};
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    double worst = 0.0;
    const int count = 200;
    for (int j = 0; j < count; j++) {
      const double th = angles[j % 8];
      double ax[3], nrm = 0.0;
      do {
        for (double& a : ax) a = u(rng);
        nrm = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
      } while (nrm < 0.1 || nrm > 1.0);
      const std::array<double, 6> xi = {th * ax[0] / nrm, th * ax[1] / nrm, th * ax[2] / nrm, 10.0 * u(rng), 10.0 * u(rng), 10.0 * u(rng)};
      const Isometry3d T = se3_exp(xi);
      const std::array<double, 6> back = se3_log(T);
      const Isometry3d T2 = se3_exp(back);
      const double tn = std::sqrt(T(0, 3) * T(0, 3) + T(1, 3) * T(1, 3) + T(2, 3) * T(2, 3));
      const double bound = 256 * kEps * (1.0 + tn), xbound = th >= 3.0 ? bound / (M_PI - th) : bound;
      for (int e = 0; e < 16; e++) worst = std::fmax(worst, std::fabs(T2.m[e] - T.m[e]) / bound);
      for (int e = 0; e < 6; e++) worst = std::fmax(worst, std::fabs(back[e] - xi[e]) / xbound);
    }
    const std::array<double, 6> zero = se3_log(Isometry3d());
    bool zero_exact = true;
    for (double z : zero) zero_exact = zero_exact && z == 0.0;
    std::printf("LOG twists %d within %d worst %.4f\n", count, worst <= 1.0 && zero_exact ? 1 : 0, worst);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

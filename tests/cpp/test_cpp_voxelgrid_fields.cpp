// voxelgrid_sampling(cloud, fields, ops, leaf, want_counts, want_voxel_of) of include/small_gicp_amd.hpp (sga_voxelgrid_sampling_fields)
// on one small cloud, all five reductions, against a host loop over the same points: voxels in ascending (z, y, x) order, members in
// ascending index, the mean in double, the nearest member by its squared distance to the fp32 centroid the call returned.
// usage: test_cpp_voxelgrid_fields          (no arguments: the cloud is made here — coordinates on a 1/8 lattice, so sums are exact)
//   GRID   voxels <m> cloud <0|1> counts <0|1> voxel_of <0|1>   the cloud equals voxelgrid_sampling(cloud, leaf)'s; counts and rows as the loop's
//   COLUMN <c> <op> equal <0|1>                                  column c of every voxel equals the loop's value (MEAN: within one fp32 rounding)
//   MEMBERSHIP equal <0|1>                                       without fields: no features, the same counts and rows
//   DEFAULT equal <0|1>                                          empty ops: MEAN each
//   REFUSE equal <0|1>                                           a row count other than the cloud's size throws and names both numbers
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

int main() {
  try {
    const double leaf = 1.0;
    std::vector<std::array<float, 3>> pts;
    std::vector<float> rows;  // 5 columns per point
    const int dim = 5;
    // 40 points on a 1/8 lattice scattered over 3 x 2 x 2 voxels about the origin, one of them outside every other's voxel, two NaN
    for (int i = 0; i < 40; i++) {
      const int a = (i * 7) % 24, b = (i * 11) % 16, c = (i * 5) % 16;
      pts.push_back({-1.5f + 0.125f * a, -1.0f + 0.125f * b + 0.0625f, -1.0f + 0.125f * c + 0.03125f});
    }
    pts[13][1] = NAN;
    pts[29][0] = NAN;
    pts.push_back({7.25f, 7.25f, 7.25f});
    const size_t n = pts.size();
    for (size_t i = 0; i < n; i++) {
      const float t = static_cast<float>((i * 37) % 41) / 41.0f;
      const float v[5] = {t, 100.0f - 3.0f * static_cast<float>(i % 9), static_cast<float>((i * 13) % 17) - 8.0f, static_cast<float>(i % 4), t * 0.5f};
      rows.insert(rows.end(), v, v + 5);
    }
    PointCloud cloud(pts);
    Features fields(rows.data(), n, dim, cloud.ctx);
    const std::vector<Reduce> ops = {Reduce::Mean, Reduce::Min, Reduce::Max, Reduce::First, Reduce::Nearest};
    const GridFields g = voxelgrid_sampling(cloud, &fields, ops, leaf, true, true);
    const PointCloud::Ptr plain = voxelgrid_sampling(cloud, leaf);

    // the host loop
    std::map<std::tuple<long, long, long>, std::vector<size_t>> voxels;  // (z, y, x) -> members, ascending
    std::vector<bool> dropped(n, false);
    for (size_t i = 0; i < n; i++) {
      const auto p = cloud.point(i);
      if (!(p[0] - p[0] == 0.0 && p[1] - p[1] == 0.0 && p[2] - p[2] == 0.0)) {
        dropped[i] = true;
        continue;
      }
      voxels[{static_cast<long>(std::floor(p[2] * (1.0 / leaf))), static_cast<long>(std::floor(p[1] * (1.0 / leaf))), static_cast<long>(std::floor(p[0] * (1.0 / leaf)))}].push_back(i);
    }
    const size_t m = voxels.size();
    bool cloud_ok = g.cloud->size() == m && plain->size() == m, counts_ok = g.counts.size() == m, rows_ok = g.voxel_of.size() == n;
    for (size_t v = 0; cloud_ok && v < m; v++) cloud_ok = g.cloud->point(v) == plain->point(v);
    const std::vector<float> got = g.fields->download();
    bool col_ok[5] = {got.size() == m * dim, got.size() == m * dim, got.size() == m * dim, got.size() == m * dim, got.size() == m * dim};
    size_t v = 0;
    for (const auto& [key, mem] : voxels) {
      if (counts_ok) counts_ok = g.counts[v] == static_cast<int32_t>(mem.size());
      for (size_t i : mem) rows_ok = rows_ok && g.voxel_of[i] == static_cast<int64_t>(v);
      if (!col_ok[0] || !cloud_ok) break;
      const auto c = g.cloud->point(v);  // the fp32 centroid the call wrote (the origin is zero: point() is the record)
      double sum = 0.0, lo = INFINITY, hi = -INFINITY, best = INFINITY;
      size_t nearest = mem[0];
      for (size_t i : mem) {
        const float* f = &rows[i * dim];
        sum += f[0];
        lo = std::fmin(lo, f[1]);
        hi = std::fmax(hi, f[2]);
        const auto p = cloud.point(i);
        const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best) best = d2, nearest = i;
      }
      const float* o = &got[v * dim];
      const double mean = sum / static_cast<double>(mem.size());
      col_ok[0] = col_ok[0] && std::fabs(o[0] - mean) <= 6e-8 * std::fabs(mean) + 1e-30;
      col_ok[1] = col_ok[1] && o[1] == lo;
      col_ok[2] = col_ok[2] && o[2] == hi;
      col_ok[3] = col_ok[3] && std::memcmp(&o[3], &rows[mem[0] * dim + 3], 4) == 0;
      col_ok[4] = col_ok[4] && std::memcmp(&o[4], &rows[nearest * dim + 4], 4) == 0;
      v++;
    }
    for (size_t i = 0; i < n; i++)
      if (dropped[i]) rows_ok = rows_ok && g.voxel_of[i] == -1;
    std::printf("GRID voxels %zu cloud %d counts %d voxel_of %d\n", m, cloud_ok ? 1 : 0, counts_ok ? 1 : 0, rows_ok ? 1 : 0);
    const char* names[5] = {"mean", "min", "max", "first", "nearest"};
    for (int c = 0; c < 5; c++) std::printf("COLUMN %d %s equal %d\n", c, names[c], col_ok[c] ? 1 : 0);

    const GridFields only = voxelgrid_sampling(cloud, nullptr, {}, leaf, true, true);
    std::printf("MEMBERSHIP equal %d\n", !only.fields && only.counts == g.counts && only.voxel_of == g.voxel_of && only.cloud->size() == m ? 1 : 0);
    const GridFields means = voxelgrid_sampling(cloud, &fields, {}, leaf);
    const GridFields means2 = voxelgrid_sampling(cloud, &fields, std::vector<Reduce>(5, Reduce::Mean), leaf);
    const std::vector<float> a = means.fields->download(), b = means2.fields->download();
    std::printf("DEFAULT equal %d\n", a.size() == m * dim && std::memcmp(a.data(), b.data(), a.size() * 4) == 0 && means.counts.empty() && means.voxel_of.empty() ? 1 : 0);
    bool refused = false;
    try {
      Features fewer(rows.data(), n - 1, dim, cloud.ctx);
      voxelgrid_sampling(cloud, &fewer, ops, leaf);
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "40 rows") != nullptr && std::strstr(e.what(), "41 points") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

// PointCloud::clusters with ClusterParams and KdTree::radius_search (include/small_gicp_amd.hpp: sga_cloud_cluster,
// sga_index_radius_search) against a host loop: brute-force squared distances in double over the cloud's points, a plain union-find over
// the core points, the border rule, the size filter and the numbering of small_gicp_amd.h.
// usage: test_cpp_cloud_cluster points.f32   (raw float32 xyz triples)
// The cloud is preprocessed by the header's own call (voxel grid, tree, covariances), then clustered with the caller's tree and with a
// temporary one.
//   CLUSTER <min_points> clusters <c> noise <x> dropped <y> equal <0|1> table <0|1> tree <0|1> keep <0|1>
//       equal: labels and the three counts are the host loop's; table: seeds, sizes and boxes are; tree: the call with a temporary tree
//       gives the same labels; keep: the cloud of the clustered points holds exactly the points with a label, in order, bit for bit
//   RADIUS total <t> equal <0|1>   counts, offsets and the lists as sets are the host loop's
//   REFUSE equal <0|1>   min_points = 0 throws and names it
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <numeric>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

struct HostClusters {
  std::vector<int32_t> labels;
  uint64_t clusters = 0, noise = 0, dropped = 0;
  std::vector<sga_cluster_row> table;
};

static HostClusters host_clusters(const std::vector<std::array<double, 4>>& p, const sga_cluster_params& q) {
  const size_t n = p.size();
  const double r2 = q.radius * q.radius;
  auto d2 = [&](size_t i, size_t j) {
    const double x = p[i][0] - p[j][0], y = p[i][1] - p[j][1], z = p[i][2] - p[j][2];
    return x * x + y * y + z * z;
  };
  std::vector<char> core(n, 0);
  for (size_t i = 0; i < n; i++) {
    int c = 0;
    for (size_t j = 0; j < n; j++) c += d2(i, j) <= r2 ? 1 : 0;
    core[i] = c >= q.min_points;
  }
  std::vector<size_t> parent(n);
  std::iota(parent.begin(), parent.end(), size_t(0));
  auto find = [&](size_t v) {
    while (parent[v] != v) v = parent[v] = parent[parent[v]];
    return v;
  };
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; core[i] && j < i; j++)
      if (core[j] && d2(i, j) <= r2) {
        const size_t a = find(i), b = find(j);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
      }
  std::vector<long long> root(n, -1);
  for (size_t i = 0; i < n; i++)
    if (core[i]) root[i] = static_cast<long long>(find(i));
  for (size_t i = 0; i < n; i++) {
    if (core[i]) continue;
    double best = INFINITY;
    for (size_t j = 0; j < n; j++)
      if (core[j] && d2(i, j) <= r2 && d2(i, j) < best) best = d2(i, j), root[i] = root[j];  // (j ascending: a tie keeps the lower index)
  }
  std::vector<long long> size(n, 0);
  for (size_t i = 0; i < n; i++)
    if (root[i] >= 0) size[static_cast<size_t>(root[i])]++;
  HostClusters r;
  std::vector<int32_t> number(n, -1);
  for (size_t v = 0; v < n; v++) {
    if (root[v] != static_cast<long long>(v)) continue;
    if (size[v] < q.min_size || (q.max_size > 0 && size[v] > q.max_size)) {
      r.dropped += static_cast<uint64_t>(size[v]);
      continue;
    }
    number[v] = static_cast<int32_t>(r.clusters++);
    sga_cluster_row row{static_cast<int64_t>(v), size[v], {INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
    r.table.push_back(row);
  }
  r.labels.assign(n, -1);
  for (size_t i = 0; i < n; i++) {
    if (root[i] < 0) {
      r.noise++;
      continue;
    }
    const int32_t c = number[static_cast<size_t>(root[i])];
    r.labels[i] = c;
    for (int a = 0; c >= 0 && a < 3; a++) r.table[c].lo[a] = std::min(r.table[c].lo[a], p[i][a]), r.table[c].hi[a] = std::max(r.table[c].hi[a], p[i][a]);
  }
  return r;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  try {
    std::ifstream ifs(argv[1], std::ios::binary | std::ios::ate);
    if (!ifs) throw std::runtime_error("cannot open the points file");
    std::vector<std::array<float, 3>> pts(static_cast<size_t>(ifs.tellg()) / 12);
    ifs.seekg(0);
    ifs.read(reinterpret_cast<char*>(pts.data()), pts.size() * 12);
    auto [cloud, tree] = preprocess_points(pts, 0.5, 10);
    const size_t n = cloud->size();
    std::vector<std::array<double, 4>> p(n);
    for (size_t i = 0; i < n; i++) p[i] = cloud->point(i);
    const ClusterParams cases[2] = {ClusterParams(1.0, 1, 5, 0, ClusterParams::Clustered), ClusterParams(1.0, 4, 1, 400, ClusterParams::Clustered)};
    for (const ClusterParams& q : cases) {
      const Clusters got = cloud->clusters(q, tree->h, n), got2 = cloud->clusters(q, nullptr, n);
      const HostClusters want = host_clusters(p, q);
      const bool equal = got.labels == want.labels && got.counts.clusters == want.clusters && got.counts.noise == want.noise && got.counts.dropped == want.dropped;
      bool table = got.table.size() == want.table.size() && got.counts.rows == want.clusters;
      for (size_t c = 0; table && c < want.table.size(); c++) table = std::memcmp(&got.table[c], &want.table[c], sizeof(sga_cluster_row)) == 0;
      const bool same = got2.labels == got.labels && got2.kept == got.kept;
      std::vector<int64_t> with_label;
      for (size_t i = 0; i < n; i++)
        if (want.labels[i] >= 0) with_label.push_back(static_cast<int64_t>(i));
      bool keep = got.cloud && got.kept == with_label && got.cloud->size() == with_label.size() && got.cloud->has_covs() == cloud->has_covs();
      for (size_t j = 0; keep && j < with_label.size(); j++) keep = cloud->point(static_cast<size_t>(with_label[j])) == got.cloud->point(j) && cloud->cov(static_cast<size_t>(with_label[j])) == got.cloud->cov(j);
      std::printf("CLUSTER %d clusters %llu noise %llu dropped %llu equal %d table %d tree %d keep %d\n", q.min_points, static_cast<unsigned long long>(got.counts.clusters), static_cast<unsigned long long>(got.counts.noise),
                  static_cast<unsigned long long>(got.counts.dropped), equal ? 1 : 0, table ? 1 : 0, same ? 1 : 0, keep ? 1 : 0);
    }
    {
      const double radius = 1.0, r2 = radius * radius;
      const RadiusNeighbors got = tree->radius_search(*cloud, radius), counts_only = tree->radius_search(*cloud, radius, false);
      bool equal = got.counts.size() == n && got.offsets.size() == n + 1 && counts_only.counts == got.counts && counts_only.indices.empty();
      for (size_t i = 0; equal && i < n; i++) {
        std::vector<int64_t> want;
        for (size_t j = 0; j < n; j++) {
          const double x = p[i][0] - p[j][0], y = p[i][1] - p[j][1], z = p[i][2] - p[j][2];
          if (x * x + y * y + z * z <= r2) want.push_back(static_cast<int64_t>(j));
        }
        std::vector<int64_t> have(got.indices.begin() + got.offsets[i], got.indices.begin() + got.offsets[i + 1]);
        std::sort(have.begin(), have.end());
        equal = have == want && got.counts[i] == static_cast<int64_t>(want.size());
        for (int64_t e = got.offsets[i]; equal && e < got.offsets[i + 1]; e++) {
          const size_t j = static_cast<size_t>(got.indices[e]);
          const double x = p[i][0] - p[j][0], y = p[i][1] - p[j][1], z = p[i][2] - p[j][2];
          equal = std::fabs(got.sq_dists[e] - (x * x + y * y + z * z)) <= 1e-15 * r2;
        }
      }
      std::printf("RADIUS total %zu equal %d\n", got.indices.size(), equal ? 1 : 0);
    }
    bool refused = false;
    try {
      cloud->clusters(ClusterParams(1.0, 0));
    } catch (const std::exception& e) {
      refused = std::strstr(e.what(), "min_points 0 is below 1") != nullptr;
    }
    std::printf("REFUSE equal %d\n", refused ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

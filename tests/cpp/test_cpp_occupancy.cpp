// OccupancyParams and OccupancyGrid of include/small_gicp_amd.hpp, end to end: a scan is ray-cast into a grid
// at two poses, the grid is read back, a cloud is classified and cleaned, the occupied cells are exported.
// usage: test_cpp_occupancy scan.f32 ox oy oz leaf nx ny nz min_range max_range   (raw float32 xyz triples, sensor frame)
//   the poses: the identity, then a quarter turn about z with the translation (1, -2, 0.5)
//   SCAN <k> beams <b> ignored <i> hits <h> truncated <t> cells_hit <c> cells_freed <f>      one line per integration
//   STATS total <n> unknown <u> free <f> occupied <o> epoch <e>
//   ABI equal <0|1>        a second grid driven through the C calls, mode and all, holds the same bytes (sga_occupancy_download)
//   CLASSIFY mask <m> total <n> unknown <u> free <f> occupied <o> cloud <size> consistent <0|1>    for the masks 0, 5 and 2: the states'
//       counts are the counts, and kept lists exactly the points whose state's bit is set, ascending
//   EXPORT count <c> written <w> ascending <0|1> occupied <0|1> cloud <size> capped <0|1>
//       every exported cell is occupied in the downloaded arrays, its log-odds the array's; a capacity of 3 writes the first 3
//   CLEAR epoch <e> unknown <u>
//   REFUSE leaf <0|1> range <0|1>   a leaf of 0 and a max_range beyond 4096 cells throw and name the reason
#include <cmath>
#include <cstdio>
#include <cstdlib>
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

int main(int argc, char** argv) {
  if (argc < 11) return 2;
  try {
    const PointCloud scan(read_points(argv[1]));
    const OccupancyParams params({std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4])}, std::atof(argv[5]), {std::atoi(argv[6]), std::atoi(argv[7]), std::atoi(argv[8])});
    const double min_range = std::atof(argv[9]), max_range = std::atof(argv[10]);
    Isometry3d turn;
    turn.m = {0, 1, 0, 0, -1, 0, 0, 0, 0, 0, 1, 0, 1, -2, 0.5, 1};  // column-major
    OccupancyGrid grid(params);
    const sga_occupancy_scan_stats s0 = grid.integrate_with_stats(scan, nullptr, min_range, max_range);
    const sga_occupancy_scan_stats s1 = grid.integrate_with_stats(scan, &turn, min_range, max_range);
    for (const sga_occupancy_scan_stats* s : {&s0, &s1})
      std::printf("SCAN %d beams %zu ignored %zu hits %zu truncated %zu cells_hit %zu cells_freed %zu\n", s == &s0 ? 0 : 1, s->beams, s->ignored, s->hits, s->truncated, s->cells_hit, s->cells_freed);
    const sga_occupancy_counts st = grid.stats();
    std::printf("STATS total %zu unknown %zu free %zu occupied %zu epoch %llu\n", st.total, st.unknown, st.free, st.occupied, static_cast<unsigned long long>(st.epoch));
    std::vector<uint32_t> stamp;
    std::vector<float> L;
    grid.download(stamp, L);

    // the same through the C calls
    sga_occupancy* raw = nullptr;
    check(sga_occupancy_create(default_context(), &params, &raw), "sga_occupancy_create");
    check(sga_occupancy_integrate(default_context(), raw, scan.h, nullptr, min_range, max_range, 0, nullptr), "sga_occupancy_integrate");
    check(sga_occupancy_integrate(default_context(), raw, scan.h, turn.data(), min_range, max_range, 0, nullptr), "sga_occupancy_integrate");
    std::vector<uint32_t> stamp2(grid.cells());
    std::vector<float> L2(grid.cells());
    check(sga_occupancy_download(default_context(), raw, stamp2.data(), L2.data()), "sga_occupancy_download");
    sga_occupancy_destroy(raw);
    const bool equal = stamp.size() == grid.cells() && std::memcmp(stamp.data(), stamp2.data(), stamp.size() * 4) == 0 && std::memcmp(L.data(), L2.data(), L.size() * 4) == 0 && grid.epoch() == 2;
    std::printf("ABI equal %d\n", equal ? 1 : 0);

    for (int mask : {0, 5, 2}) {
      const OccupancyClassified c = grid.classify(scan, &turn, 0.0, mask, true, mask != 0);
      size_t per[3] = {0, 0, 0};
      std::vector<int64_t> want;
      bool consistent = c.state.size() == scan.size();
      for (size_t i = 0; consistent && i < c.state.size(); i++) {
        consistent = c.state[i] <= 2;
        if (!consistent) break;
        per[c.state[i]]++;
        if ((mask >> c.state[i]) & 1) want.push_back(static_cast<int64_t>(i));
      }
      consistent = consistent && per[0] == c.counts.unknown && per[1] == c.counts.free && per[2] == c.counts.occupied && c.counts.total == scan.size() && c.counts.epoch == 2;
      if (mask == 0) consistent = consistent && !c.cloud && c.kept.empty();
      else consistent = consistent && c.cloud && c.cloud->size() == want.size() && c.kept == want;
      std::printf("CLASSIFY mask %d total %zu unknown %zu free %zu occupied %zu cloud %zu consistent %d\n", mask, c.counts.total, c.counts.unknown, c.counts.free, c.counts.occupied, c.cloud ? c.cloud->size() : 0, consistent ? 1 : 0);
    }

    const OccupancyCells cells = grid.export_cells();
    bool ascending = true, occupied = cells.indices.size() == cells.count && cells.log_odds.size() == cells.count;
    for (size_t j = 0; j < cells.indices.size(); j++) {
      if (j > 0 && cells.indices[j] <= cells.indices[j - 1]) ascending = false;
      const size_t i = static_cast<size_t>(cells.indices[j]);
      if (i >= stamp.size() || stamp[i] == 0 || !(L[i] >= 0.f) || std::memcmp(&L[i], &cells.log_odds[j], 4) != 0) occupied = false;
    }
    const OccupancyCells few = grid.export_cells(0.0, OccupancyGrid::OccupiedBit, 3);
    const bool capped = few.count == cells.count && few.indices.size() == (cells.count < 3 ? cells.count : 3) && std::equal(few.indices.begin(), few.indices.end(), cells.indices.begin()) && few.cloud->size() == few.indices.size();
    std::printf("EXPORT count %zu written %zu ascending %d occupied %d cloud %zu capped %d\n", cells.count, cells.indices.size(), ascending ? 1 : 0, occupied ? 1 : 0, grid.occupied_cloud()->size(), capped ? 1 : 0);

    grid.clear();
    std::printf("CLEAR epoch %llu unknown %zu\n", static_cast<unsigned long long>(grid.epoch()), grid.stats().unknown);

    bool refused_leaf = false, refused_range = false;
    try {
      OccupancyParams bad = params;
      bad.leaf = 0.0;
      OccupancyGrid none(bad);
    } catch (const std::exception& e) {
      refused_leaf = std::strstr(e.what(), "leaf must be finite and > 0") != nullptr;
    }
    try {
      grid.integrate(scan, nullptr, 0.0, 4097.0 * params.leaf);
    } catch (const std::exception& e) {
      refused_range = std::strstr(e.what(), "more than 4096 cells") != nullptr;
    }
    std::printf("REFUSE leaf %d range %d\n", refused_leaf ? 1 : 0, refused_range ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

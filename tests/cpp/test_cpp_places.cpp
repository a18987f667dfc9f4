// PlaceParams, Places and PointCloud::scan_context of include/small_gicp_amd.hpp, end to end: keyframes are
// added to a database, a revisit is looked up by cloud and by image, and an entry travels to the host and back.
// usage: test_cpp_places rings sectors k query.f32 keyframe0.f32 keyframe1.f32 ...   (raw float32 xyz triples)
//   PLACES size <n> cells <c>
//   MATCH <index> <shift> <distance>          one line per result of the query by cloud, in order
//   IMAGE same <0|1> descriptor <0|1> reloaded <0|1>
//       same: the query by the revisit's own scan_context image gives the same results bit for bit; descriptor: entry 0 as downloaded
//       is keyframe 0's scan_context; reloaded: entry 0 added again by add_descriptor comes back bytewise equal, and a query by that
//       image finds entry 0 before its copy at equal distance
//   REFUSE k <0|1> image <0|1>   k = 33 and an image with a negative value throw and name the reason
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
  if (argc < 6) return 2;
  try {
    PlaceParams params;
    params.rings = std::atoi(argv[1]);
    params.sectors = std::atoi(argv[2]);
    const int k = std::atoi(argv[3]);
    const PointCloud revisit(read_points(argv[4]));
    Places places(params);
    std::vector<std::shared_ptr<PointCloud>> keyframes;
    for (int a = 5; a < argc; a++) {
      keyframes.push_back(std::make_shared<PointCloud>(read_points(argv[a])));
      if (places.add(*keyframes.back()) != static_cast<size_t>(a - 5)) throw std::runtime_error("add returned another index");
    }
    std::printf("PLACES size %zu cells %zu\n", places.size(), places.cells());

    const std::vector<PlaceMatch> found = places.query(revisit, k);
    for (const PlaceMatch& m : found) std::printf("MATCH %lld %d %.17g\n", static_cast<long long>(m.index), m.shift, m.distance);

    const std::vector<PlaceMatch> by_image = places.query(revisit.scan_context(params), k);
    bool same = by_image.size() == found.size();
    for (size_t t = 0; same && t < found.size(); t++) same = by_image[t].index == found[t].index && by_image[t].shift == found[t].shift && std::memcmp(&by_image[t].distance, &found[t].distance, sizeof(double)) == 0;
    const std::vector<float> entry0 = places.download(0, 1), image0 = keyframes[0]->scan_context(params);
    const bool descriptor = entry0.size() == places.cells() && std::memcmp(entry0.data(), image0.data(), entry0.size() * sizeof(float)) == 0;
    const size_t copy = places.add_descriptor(entry0);
    const std::vector<float> back = places.download(copy, 1);
    bool reloaded = copy + 1 == places.size() && std::memcmp(back.data(), entry0.data(), back.size() * sizeof(float)) == 0;
    const std::vector<PlaceMatch> twins = places.query(entry0, 2);
    reloaded = reloaded && twins.size() == 2 && twins[0].index == 0 && twins[1].index == static_cast<int64_t>(copy) && std::memcmp(&twins[0].distance, &twins[1].distance, sizeof(double)) == 0 && twins[0].shift == twins[1].shift;
    std::printf("IMAGE same %d descriptor %d reloaded %d\n", same ? 1 : 0, descriptor ? 1 : 0, reloaded ? 1 : 0);

    bool refused_k = false, refused_image = false;
    try {
      places.query(revisit, 33);
    } catch (const std::exception& e) {
      refused_k = std::strstr(e.what(), "k 33 outside [1, 32]") != nullptr;
    }
    try {
      std::vector<float> bad = entry0;
      bad[places.cells() - 1] = -1.f;
      places.add_descriptor(bad);
    } catch (const std::exception& e) {
      char want[64];
      std::snprintf(want, sizeof(want), "image value %zu ", places.cells() - 1);
      refused_image = std::strstr(e.what(), want) != nullptr;
    }
    std::printf("REFUSE k %d image %d\n", refused_k ? 1 : 0, refused_image ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
}

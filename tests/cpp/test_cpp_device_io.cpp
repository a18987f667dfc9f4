// PointCloud::from_device / export_device and knn_device (include/small_gicp_amd.hpp: the sga_*_device calls) over hipMalloc'd memory,
// against the host entry points on the same values.  usage: test_cpp_device_io   (no arguments; the points are made here)
// A synthetic N x 4 float scan (x y z intensity) and its double twin shifted far from the origin go to the device with hipMemcpy; then
//   EQUAL <what> <0|1>
// for: the float cloud (records, origin), the double cloud (records, origin), the export back into an N x 4 device array (the fourth
// column untouched), kNN against a kd-tree (indices and float distances of sga_index_knn), and the refusal of a host pointer.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "small_gicp_amd.hpp"

using namespace small_gicp_amd;

static void hip(hipError_t e, const char* what) {
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

template <typename T>
struct DeviceBlock {
  T* p = nullptr;
  explicit DeviceBlock(size_t count) { hip(hipMalloc(reinterpret_cast<void**>(&p), count * sizeof(T)), "hipMalloc"); }
  DeviceBlock(const std::vector<T>& host) : DeviceBlock(host.size()) { hip(hipMemcpy(p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy"); }
  ~DeviceBlock() { (void)hipFree(p); }
  std::vector<T> host(size_t count) const {
    std::vector<T> v(count);
    hip(hipMemcpy(v.data(), p, count * sizeof(T), hipMemcpyDeviceToHost), "hipMemcpy");
    return v;
  }
};

struct Download {
  std::vector<float> xyz;
  double origin[3];
};
static Download download(const PointCloud& c) {
  Download d;
  d.xyz.resize(3 * c.size());
  check(sga_cloud_download(c.ctx, c.h, d.xyz.data(), nullptr, nullptr), "sga_cloud_download");
  check(sga_cloud_origin(c.h, d.origin), "sga_cloud_origin");
  return d;
}
static bool same(const Download& a, const Download& b) { return a.xyz.size() == b.xyz.size() && std::memcmp(a.xyz.data(), b.xyz.data(), a.xyz.size() * sizeof(float)) == 0 && std::memcmp(a.origin, b.origin, sizeof(a.origin)) == 0; }

int main() {
  try {
    const size_t n = 1000, m = 257;
    const int k = 5;
    sga_context* ctx = default_context();
    // a deterministic scan: a lattice with a twist, fourth column = intensity
    std::vector<float> scan(4 * n), xyz(3 * n);
    std::vector<double> far4(4 * n);
    unsigned s = 12345u;
    auto next = [&s]() {
      s = s * 1664525u + 1013904223u;
      return static_cast<float>(s >> 8) / 16777216.0f * 40.0f - 20.0f;
    };
    for (size_t i = 0; i < n; i++) {
      for (int a = 0; a < 3; a++) {
        scan[4 * i + a] = xyz[3 * i + a] = next();
        far4[4 * i + a] = static_cast<double>(scan[4 * i + a]) * 1.000001 + (a == 0 ? 5e5 : a == 1 ? -3e5 : 120.0);
      }
      scan[4 * i + 3] = 7777.f;
      far4[4 * i + 3] = 1.0;
    }
    DeviceBlock<float> d_scan(scan);
    DeviceBlock<double> d_far(far4);

    // 1. float rows of stride 4 against sga_cloud_create_f32 on the packed copy
    const sga_device_array pa{d_scan.p, SGA_F32, 3, 4};
    auto dev32 = PointCloud::from_device(ctx, pa, n);
    PointCloud host32(xyz.data(), nullptr, nullptr, n, ctx);
    std::printf("EQUAL float_cloud %d\n", same(download(*dev32), download(host32)) ? 1 : 0);

    // 2. double rows of stride 4, far from the origin, against sga_cloud_create_f64
    const sga_device_array pd{d_far.p, SGA_F64, 3, 4};
    auto dev64 = PointCloud::from_device(ctx, pd, n);
    sga_cloud* h64 = nullptr;
    check(sga_cloud_create_f64(ctx, far4.data(), nullptr, nullptr, n, &h64), "sga_cloud_create_f64");
    PointCloud host64(h64, ctx);
    const Download a64 = download(*dev64), b64 = download(host64);
    std::printf("EQUAL double_cloud %d\n", same(a64, b64) && a64.origin[0] != 0.0 ? 1 : 0);

    // 3. export into an N x 4 device array: the points of sga_cloud_download, the fourth column untouched
    DeviceBlock<float> d_out(std::vector<float>(4 * n, -1.f));
    const sga_device_array oa{d_out.p, SGA_F32, 3, 4};
    dev64->export_device(&oa);
    const std::vector<float> out = d_out.host(4 * n);
    bool ok = true;
    for (size_t i = 0; i < n; i++) ok = ok && std::memcmp(&out[4 * i], &b64.xyz[3 * i], 12) == 0 && out[4 * i + 3] == -1.f;
    std::printf("EQUAL export %d\n", ok ? 1 : 0);

    // 4. kNN: the first m rows of the scan as queries, against sga_index_knn on the same floats
    auto cloud = std::make_shared<PointCloud>(xyz.data(), nullptr, nullptr, n, ctx);
    KdTree tree(cloud);
    DeviceBlock<int64_t> d_idx(m * k);
    DeviceBlock<float> d_d2(m * k);
    knn_device(ctx, tree.h, pa, m, k, d_idx.p, d_d2.p);
    std::vector<float> q(3 * m), hd(m * k);
    for (size_t i = 0; i < m; i++)
      for (int a = 0; a < 3; a++) q[3 * i + a] = scan[4 * i + a];
    std::vector<int64_t> hi(m * k);
    check(sga_index_knn(ctx, tree.h, q.data(), m, k, -1.0, hi.data(), hd.data()), "sga_index_knn");
    const std::vector<int64_t> gi = d_idx.host(m * k);
    const std::vector<float> gd = d_d2.host(m * k);
    std::printf("EQUAL knn %d\n", std::memcmp(gi.data(), hi.data(), hi.size() * sizeof(int64_t)) == 0 && std::memcmp(gd.data(), hd.data(), hd.size() * sizeof(float)) == 0 && gi[0] == 0 ? 1 : 0);

    // 5. a host pointer is refused with a message that names the host entry point
    const sga_device_array bad{xyz.data(), SGA_F32, 3, 3};
    sga_cloud* none = nullptr;
    const int rc = sga_cloud_create_device(ctx, &bad, nullptr, nullptr, n, nullptr, nullptr, 0, &none);
    std::printf("EQUAL refusal %d\n", rc == SGA_ERR_INVALID && none == nullptr && std::strstr(sga_last_error(), "sga_cloud_create_f32") != nullptr ? 1 : 0);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
}

// small_gicp_amd.hpp — header-only C++17 host layer over the C-ABI (small_gicp_amd.h) that mirrors the reference's C++ surface
// for the registration hot path, name for name and default for default (reference tree /root/reference, koide3/small_gicp v1.0.1):
//
//   Registration<PointFactor, Reduction, GeneralFactor, CorrespondenceRejector, Optimizer>::align   registration/registration.hpp:17-54
//   ICPFactor / PointToPlaneICPFactor / GICPFactor / RobustFactor<Huber|Cauchy, F>                   factors/*.hpp
//   DistanceRejector / NullRejector, TerminationCriteria, NullFactor / RestrictDoFFactor             registration/rejector.hpp, termination_criteria.hpp, factors/general_factor.hpp
//   LevenbergMarquardtOptimizer / GaussNewtonOptimizer (fields)                                      registration/optimizer.hpp:24-149
//   RegistrationResult, RegistrationSetting, preprocess_points, create_gaussian_voxelmap, align x3    registration_result.hpp, registration_helper.hpp:37-90
//   PointCloud, KdTree, GaussianVoxelMap, voxelgrid_sampling, estimate_{normals,covariances,...}      points/point_cloud.hpp, ann/*.hpp, util/*.hpp
//
// The one new name is the reduction policy `ParallelReductionHIP` (the slot SerialReduction / ParallelReductionOMP / ...TBB fill
// in the reference): with it the whole align() runs on the GPU and only the 6x6 solve stays on the host.
// Eigen is not required (it is absent from this image); fixed-size values are plain column-major double arrays, and thin
// adaptors are enabled when <Eigen/Core> is on the include path.
#pragma once
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <type_traits>
#include <string>
#include <utility>
#include <vector>

#include "small_gicp_amd.h"

#if __has_include(<Eigen/Core>)
#include <Eigen/Core>
#include <Eigen/Geometry>
#define SMALL_GICP_AMD_HAS_EIGEN 1
#endif

namespace small_gicp_amd {

inline void check(int rc, const char* what) {
  if (rc != SGA_OK) throw std::runtime_error(std::string(what) + ": " + sga_last_error());
}

/// 4x4 rigid transform, column-major like Eigen::Isometry3d::matrix().data().
struct Isometry3d {
  std::array<double, 16> m{{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  static Isometry3d Identity() { return Isometry3d(); }
  double& operator()(int r, int c) { return m[4 * c + r]; }
  double operator()(int r, int c) const { return m[4 * c + r]; }
  const double* data() const { return m.data(); }
  Isometry3d operator*(const Isometry3d& o) const {
    Isometry3d r;
    for (int c = 0; c < 4; c++)
      for (int i = 0; i < 4; i++) {
        double s = 0;
        for (int k = 0; k < 4; k++) s += (*this)(i, k) * o(k, c);
        r(i, c) = s;
      }
    return r;
  }
  Isometry3d inverse() const {
    Isometry3d r;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) r(i, j) = (*this)(j, i);
      r(i, 3) = 0;
    }
    for (int i = 0; i < 3; i++)
      for (int k = 0; k < 3; k++) r(i, 3) -= (*this)(k, i) * (*this)(k, 3);
    return r;
  }
#ifdef SMALL_GICP_AMD_HAS_EIGEN
  Isometry3d(const Eigen::Isometry3d& T) { std::memcpy(m.data(), T.matrix().data(), sizeof(double) * 16); }
  operator Eigen::Isometry3d() const {
    Eigen::Isometry3d T;
    std::memcpy(T.matrix().data(), m.data(), sizeof(double) * 16);
    return T;
  }
  Isometry3d() = default;
#endif
};

/// The pose of a twist [rx ry rz tx ty tz] (sga_se3_exp) and the twist of a pose whose rotation angle is below pi (sga_se3_log): host
/// functions, evaluated without cancellation at small angles.
inline Isometry3d se3_exp(const std::array<double, 6>& twist) {
  Isometry3d T;
  sga_se3_exp(twist.data(), T.m.data());
  return T;
}
inline std::array<double, 6> se3_log(const Isometry3d& T) {
  std::array<double, 6> twist{};
  sga_se3_log(T.data(), twist.data());
  return twist;
}

/// One context (GPU + stream) per device, shared by the objects of this header.
inline sga_context* default_context(int device = 0) {
  static std::array<sga_context*, 16> ctxs{};
  if (device < 0 || device >= 16) throw std::runtime_error("device out of range");
  if (!ctxs[device]) check(sga_context_create(device, &ctxs[device]), "sga_context_create");
  return ctxs[device];
}

/// The predicate of PointCloud::cropped / crop_clouds (sga_crop with its defaults: every finite point is kept).  A point p of the caller's
/// frame is kept when it is finite, min_range <= |p - center| <= max_range, and — box_mode 1 — it lies inside the closed box [box_lo,
/// box_hi] or — box_mode 2, an ego-vehicle box — it does not.
struct Crop : sga_crop {
  Crop() { sga_crop_default(this); }
  Crop(double min_r, double max_r) {
    sga_crop_default(this);
    min_range = min_r, max_range = max_r;
  }
  Crop& box(const std::array<double, 3>& lo, const std::array<double, 3>& hi, int mode = 1) {
    for (int a = 0; a < 3; a++) box_lo[a] = lo[a], box_hi[a] = hi[a];
    box_mode = mode;
    return *this;
  }
  Crop& about(const std::array<double, 3>& c) {
    for (int a = 0; a < 3; a++) center[a] = c[a];
    return *this;
  }
};

/// The filter of PointCloud::without_outliers (sga_outlier_filter with its defaults: statistical, k = 10, std_mul = 1).  Statistical: a
/// point is kept when the mean distance to its k nearest neighbours is at most mean + std_mul * stddev of that figure over the cloud;
/// radius: when at least k other points lie within `radius`.
struct OutlierFilter : sga_outlier_filter {
  OutlierFilter() { sga_outlier_filter_default(this); }
  static OutlierFilter statistical(int k_ = 10, double std_mul_ = 1.0) {
    OutlierFilter f;
    f.k = k_, f.std_mul = std_mul_;
    return f;
  }
  static OutlierFilter within_radius(int min_neighbors, double radius_) {
    OutlierFilter f;
    f.mode = 1, f.k = min_neighbors, f.radius = radius_;
    return f;
  }
};

/// What PointCloud::clusters asks for (sga_cluster_params with its defaults: radius 0.5, min_points 1, min_size 1, no max_size, no cloud):
/// DBSCAN with a deterministic border rule (small_gicp_amd.h).  keep says which points the output cloud holds.
struct ClusterParams : sga_cluster_params {
  enum Keep { None = 0, Clustered = 1, Rest = 2 };
  ClusterParams() { sga_cluster_params_default(this); }
  explicit ClusterParams(double radius_, int min_points_ = 1, int64_t min_size_ = 1, int64_t max_size_ = 0, Keep keep_ = None) {
    sga_cluster_params_default(this);
    radius = radius_, min_points = min_points_, min_size = min_size_, max_size = max_size_, keep = static_cast<int>(keep_);
  }
};
struct PointCloud;
/// What PointCloud::clusters found: a label per point (-1: noise or a dropped cluster), the counts, a row per kept cluster (seed, size,
/// box; the first table_capacity of them), and the cloud of the clustered or the other points with their indices (keep other than None).
struct Clusters {
  std::vector<int32_t> labels;
  sga_cluster_result counts{};
  std::vector<sga_cluster_row> table;
  std::shared_ptr<PointCloud> cloud;
  std::vector<int64_t> kept;
};
/// What PointCloud::iss_keypoints asks for (sga_iss_params with its defaults: gamma_21 = gamma_32 = 0.975, min_neighbors 5, no cloud; the
/// two radii have none): Intrinsic Shape Signatures (small_gicp_amd.h).
struct IssParams : sga_iss_params {
  IssParams(double salient_radius_, double non_max_radius_, bool keep_ = false) {
    sga_iss_default(this);
    salient_radius = salient_radius_, non_max_radius = non_max_radius_, keep = keep_ ? 1 : 0;
  }
};
/// What PointCloud::iss_keypoints found: the keypoints' indices (ascending), the saliency of every point when asked for, and the cloud of
/// the keypoints (null unless params.keep).
struct Keypoints {
  std::vector<int64_t> indices;
  std::vector<double> saliency;
  std::shared_ptr<PointCloud> cloud;
};
/// What PointCloud::segment_plane asks for (sga_plane_params with its defaults: threshold 0.1, 1000 hypotheses, seed 0, no axis, at least
/// 3 inliers, refit, no cloud): RANSAC over triples of records (small_gicp_amd.h).  keep says which points the output cloud holds.
struct PlaneParams : sga_plane_params {
  enum Keep { None = 0, Plane = 1, Rest = 2 };
  PlaneParams() { sga_plane_default(this); }
  explicit PlaneParams(double distance_threshold_, uint64_t iterations_ = 1000, uint64_t seed_ = 0, Keep keep_ = None) {
    sga_plane_default(this);
    distance_threshold = distance_threshold_, iterations = iterations_, seed = seed_, keep = static_cast<int>(keep_);
  }
  /// only planes whose normal lies within max_angle_ (radians) of +-axis, the normal turned towards the axis
  PlaneParams& along(double x, double y, double z, double max_angle_) {
    axis[0] = x, axis[1] = y, axis[2] = z, max_angle = max_angle_;
    return *this;
  }
};
/// What PointCloud::segment_plane found: coefficients = (n, d) with n . p + d = 0 in the caller's frame (zeros and result.inliers 0: no
/// plane), the counts, the score of every hypothesis when asked for, and the cloud of the plane's or of the other points with their indices.
struct Plane {
  std::array<double, 4> coefficients{};
  sga_plane_result result{};
  std::vector<uint32_t> scores;
  std::shared_ptr<PointCloud> cloud;
  std::vector<int64_t> kept;
  bool found() const { return result.inliers > 0; }
};
/// What segment_planes found: the planes in the order found, a label per point of the original cloud (the plane's number, -1 for none),
/// the cloud left over and its points' indices in the original cloud.
struct Planes {
  std::vector<Plane> planes;
  std::vector<int32_t> labels;
  std::shared_ptr<PointCloud> rest;
  std::vector<int64_t> rest_indices;
};
/// What KdTree::radius_search found: the number of neighbours per query and, when asked for, their CSR lists.
struct RadiusNeighbors {
  std::vector<int64_t> counts, offsets, indices;
  std::vector<double> sq_dists;
};

/// What PointCloud::overlap asks for (sga_overlap with its defaults: max_distance 1, statistics only).  A point is matched when its
/// nearest target record lies within max_distance; keep says which points the output cloud holds.
struct Overlap {
  enum Keep { None = 0, Matched = 1, Unmatched = 2 };
  double max_distance = 1.0;
  Keep keep = None;
  Overlap() = default;
  Overlap(double max_distance_, Keep keep_ = None) : max_distance(max_distance_), keep(keep_) {}
};
struct PointCloud;
/// What PointCloud::overlap found: the statistics (points, matched, fitness = matched / points, rmse and mean_distance over the matched),
/// the cloud of the matched or the unmatched points (null when keep is None) and — where asked for — the distance per point (+inf where
/// unmatched), the winner per point (the target point's index, the voxel id, voxel * 16 + slot for a flat map; -1 where unmatched) and
/// the indices of the output cloud's points, ascending.
struct OverlapResult {
  sga_overlap_stats stats{};
  std::shared_ptr<PointCloud> cloud;
  std::vector<double> dist;
  std::vector<int64_t> nearest, kept;
};

/// What PointCloud::visibility asks for (sga_visibility with its defaults: 1024 x 64 over [-25, +3] degrees, ranges 0.5 .. 60 m, margin
/// 0.2 m + 1 % of the range, window 1 x 1, statistics only).  keep says which points the output cloud holds.
struct Visibility : sga_visibility {
  enum Keep { None = 0, SeenThrough = 1, Rest = 2 };
  enum State : uint8_t { Unobserved = 0, Consistent = 1, Occluded = 2, Seen = 3 };
  Visibility() { sga_visibility_default(this); }
  explicit Visibility(Keep keep_) {
    sga_visibility_default(this);
    keep = static_cast<int>(keep_);
  }
};
/// What PointCloud::visibility found: the counts per state, the cloud of the seen-through points or of all the others (null when keep is
/// None) and — where asked for — the state and the clearance per point (NaN where unobserved), the scan's range image ([v * width + u],
/// +inf where empty) and the indices of the output cloud's points, ascending.
struct VisibilityResult {
  sga_visibility_stats stats{};
  std::shared_ptr<PointCloud> cloud;
  std::vector<uint8_t> state;
  std::vector<double> clearance, range_image;
  std::vector<int64_t> kept;
};

/// n rows of dim floats on the device (sga_features): the FPFH descriptors of PointCloud::fpfh, or a caller's own (1 <= dim <= 128).
struct Features {
  using Ptr = std::shared_ptr<Features>;
  Features(sga_features* handle, sga_context* context) : ctx(context), h(handle) {}
  /// rows: n * dim floats, row-major
  Features(const float* rows, size_t n, int dim, sga_context* context = default_context()) : ctx(context) { check(sga_features_create(ctx, rows, n, dim, &h), "sga_features_create"); }
  Features(const Features&) = delete;
  Features& operator=(const Features&) = delete;
  ~Features() { sga_features_destroy(h); }
  size_t size() const {
    size_t n = 0;
    sga_features_size(h, &n, nullptr);
    return n;
  }
  int dim() const {
    int d = 0;
    sga_features_size(h, nullptr, &d);
    return d;
  }
  /// the rows on the host, row-major
  std::vector<float> download() const {
    std::vector<float> rows(size() * static_cast<size_t>(dim()));
    check(sga_features_download(ctx, h, rows.empty() ? nullptr : rows.data()), "sga_features_download");
    return rows;
  }
  /// New features whose row j is this one's row indices[j] (sga_features_select: one launch); repeats are allowed
  Ptr selected(const std::vector<int64_t>& indices) const {
    sga_features* made = nullptr;
    check(sga_features_select(ctx, h, indices.empty() ? nullptr : indices.data(), indices.size(), &made), "sga_features_select");
    return std::make_shared<Features>(made, ctx);
  }
  /// Features from rows that live in device memory of the context's device (sga_features_create_device): float or double, cols = dim,
  /// any stride >= cols; a double is rounded to float once.  stream: as PointCloud::from_device.
  static Ptr from_device(sga_context* context, const sga_device_array& rows, size_t n, void* stream = nullptr, int flags = 0) {
    sga_features* made = nullptr;
    check(sga_features_create_device(context, &rows, n, stream, flags, &made), "sga_features_create_device");
    return std::make_shared<Features>(made, context);
  }
  /// The rows into a device array of the caller's, cols = dim (sga_features_export_device)
  void export_device(const sga_device_array& rows, void* stream = nullptr, int flags = 0) const { check(sga_features_export_device(ctx, h, &rows, stream, flags), "sga_features_export_device"); }
  sga_context* ctx = default_context();
  sga_features* h = nullptr;
};

/// For every row of `source` the nearest row of `target` in squared L2 distance (sga_features_match; ties to the lowest index); mutual:
/// only the pairs that are each other's nearest.  Returns the pairs (source row, target row), ascending in the source row; dist
/// (optional): their distances.
inline std::vector<std::array<int64_t, 2>> match_features(const Features& source, const Features& target, bool mutual = true, std::vector<double>* dist = nullptr) {
  const size_t n = source.size();
  std::vector<int64_t> match(n);
  std::vector<double> d(dist ? n : 0);
  size_t matched = 0;
  int64_t none = -1;
  check(sga_features_match(source.ctx, source.h, target.h, mutual ? 1 : 0, n > 0 ? match.data() : &none, d.empty() ? nullptr : d.data(), &matched), "sga_features_match");
  std::vector<std::array<int64_t, 2>> pairs;
  pairs.reserve(matched);
  if (dist) dist->clear();
  for (size_t i = 0; i < n; i++)
    if (match[i] >= 0) {
      pairs.push_back({static_cast<int64_t>(i), match[i]});
      if (dist) dist->push_back(d[i]);
    }
  return pairs;
}

/// The parameters of ransac_correspondences (sga_ransac with its defaults: max_distance 1, 20000 hypotheses, seed 0, edge_similarity 0.9,
/// min_edge 0) and what it found: the pose, source -> target, with the inliers and their RMSE under the best hypothesis, that hypothesis'
/// number, the hypotheses that passed the edge and degeneracy tests, and whether the pose is the least-squares refit over the inliers.
struct Ransac : sga_ransac {
  Ransac() { sga_ransac_default(this); }
};
struct RansacResult : sga_ransac_result {
  Isometry3d T_target_source;
};

/// The parameters of a Scan Context descriptor (sga_place_params with its defaults: 20 rings x 60 sectors out to 80 m, heights
/// measured from 2 m below the sensor) and one result of a query: the entry, its best column shift, its distance.
struct PlaceParams : sga_place_params {
  PlaceParams() { sga_place_params_default(this); }
};
using PlaceMatch = sga_place_match;

/// points/point_cloud.hpp:15-71 — device-resident; host copies on demand (points(i) etc. read a cached download).
struct PointCloud {
  using Ptr = std::shared_ptr<PointCloud>;
  using ConstPtr = std::shared_ptr<const PointCloud>;

  PointCloud() { check(sga_cloud_create_f32(ctx, nullptr, nullptr, nullptr, 0, &h), "sga_cloud_create_f32"); }
  template <typename T, size_t D>
  explicit PointCloud(const std::vector<std::array<T, D>>& pts, int device = 0) : ctx(default_context(device)) {
    static_assert(D == 3 || D == 4, "points must be 3- or 4-vectors");
    // double points may lie kilometres from the origin (points/point_cloud.hpp:69-71): the cloud's origin is subtracted in double before the
    // cast (small_gicp_amd.h: device frames); float points are what they are and go through the library's own recentring
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, origin[3] = {0, 0, 0};
    for (size_t i = 0; i < pts.size(); i++)
      for (int k = 0; k < 3; k++) {
        const double v = static_cast<double>(pts[i][k]);
        if (v - v == 0.0) lo[k] = v < lo[k] ? v : lo[k], hi[k] = v > hi[k] ? v : hi[k];
      }
    sga_choose_origin(lo, hi, origin);
    std::vector<float> xyz(pts.size() * 3);
    for (size_t i = 0; i < pts.size(); i++)
      for (int k = 0; k < 3; k++) xyz[3 * i + k] = static_cast<float>(static_cast<double>(pts[i][k]) - origin[k]);
    check(sga_cloud_create_f32_origin(ctx, xyz.data(), nullptr, nullptr, pts.size(), origin, &h), "sga_cloud_create_f32_origin");
  }
  /// xyz n*3 floats [+ normals n*3] [+ cov6 n*6 (xx,xy,xz,yy,yz,zz)]
  PointCloud(const float* xyz, const float* normals, const float* cov6, size_t n, int device = 0) : ctx(default_context(device)) { check(sga_cloud_create_f32(ctx, xyz, normals, cov6, n, &h), "sga_cloud_create_f32"); }
  explicit PointCloud(sga_cloud* handle, int device = 0) : ctx(default_context(device)), h(handle) {}
  /// On a context of the caller's (sga_context_create: its own HIP stream) instead of the device's default one — the stages of a
  /// pipeline that run side by side take one each (examples/odometry_benchmark_flow.cpp).
  PointCloud(const float* xyz, const float* normals, const float* cov6, size_t n, sga_context* context) : ctx(context) { check(sga_cloud_create_f32(ctx, xyz, normals, cov6, n, &h), "sga_cloud_create_f32"); }
  PointCloud(sga_cloud* handle, sga_context* context) : ctx(context), h(handle) {}
  PointCloud(const PointCloud&) = delete;
  PointCloud& operator=(const PointCloud&) = delete;
  ~PointCloud() { sga_cloud_destroy(h); }

  /// A cloud from arrays that live in device memory of the context's device (sga_cloud_create_device: hipMalloc'd memory, a tensor's
  /// data pointer), read where they are: rows of `stride` elements, float or double.  origin NULL: chosen by the library; given: the
  /// points are recentred about it (with SGA_IO_RELATIVE in flags: they are relative to it already).  stream: the hipStream_t the arrays
  /// were written on; the library orders itself behind it and the stream's later work behind its reads (small_gicp_amd.h).
  static Ptr from_device(sga_context* context, const sga_device_array& points, size_t n, const sga_device_array* normals = nullptr, const sga_device_array* covs = nullptr, const double* origin = nullptr, void* stream = nullptr,
                         int flags = 0) {
    sga_cloud* made = nullptr;
    if (n == 0)
      check(sga_cloud_create_f32(context, nullptr, nullptr, nullptr, 0, &made), "sga_cloud_create_f32");
    else
      check(sga_cloud_create_device(context, &points, normals, covs, n, origin, stream, flags, &made), "sga_cloud_create_device");
    return std::make_shared<PointCloud>(made, context);
  }
  /// The cloud into device arrays of the caller's (sga_cloud_export_device; any may be NULL): points in the caller's frame, normals, covariances.
  void export_device(const sga_device_array* points, const sga_device_array* normals = nullptr, const sga_device_array* covs = nullptr, void* stream = nullptr, int flags = 0) const {
    check(sga_cloud_export_device(ctx, h, points, normals, covs, stream, flags), "sga_cloud_export_device");
  }

  /// This cloud posed by T as a new cloud on the device (sga_cloud_transform: points T * p, normals R n, covariances R C R^T — the loop of
  /// src/test/registration_test.cpp:84 over points, normals and covs); origin: the new cloud's device-frame origin (NULL: chosen by the library).
  Ptr transformed(const Isometry3d& T, const double* origin = nullptr) const {
    sga_cloud* made = nullptr;
    check(sga_cloud_transform(ctx, h, T.data(), origin, &made), "sga_cloud_transform");
    return std::make_shared<PointCloud>(made, ctx);
  }

  /// This raw sweep with the sensor's motion undone, as a new cloud on the device (sga_cloud_deskew): point i, measured at times[i] in the
  /// sensor frame of that instant, becomes exp((times[i] - ref_time) twist) p_i; twist = the motion per unit of time (se3_log of the
  /// sweep's relative pose when the times run from 0 to 1).  times: size() values in host memory, the cloud's order.
  Ptr deskewed(const float* times, const std::array<double, 6>& twist, double ref_time = 1.0) const {
    sga_cloud* made = nullptr;
    check(sga_cloud_deskew(ctx, h, times, twist.data(), ref_time, &made), "sga_cloud_deskew");
    return std::make_shared<PointCloud>(made, ctx);
  }
  /// The same with the times in device memory of the context's device (sga_cloud_deskew_device: float or double, cols = 1, any stride).
  Ptr deskewed(const sga_device_array& times, const std::array<double, 6>& twist, double ref_time = 1.0, void* stream = nullptr, int flags = 0) const {
    sga_cloud* made = nullptr;
    check(sga_cloud_deskew_device(ctx, h, &times, twist.data(), ref_time, stream, flags, &made), "sga_cloud_deskew_device");
    return std::make_shared<PointCloud>(made, ctx);
  }

  /// This cloud without the points the crop drops, as a new cloud on the device (sga_cloud_crop): the order, the normals, the covariances
  /// and the origin are kept.  kept (optional): receives the indices kept, ascending — what keeps a sweep's times aligned.
  Ptr cropped(const Crop& crop, std::vector<int64_t>* kept = nullptr) const {
    sga_cloud* made = nullptr;
    if (kept) kept->resize(size());
    check(sga_cloud_crop(ctx, h, &crop, kept && !kept->empty() ? kept->data() : nullptr, &made), "sga_cloud_crop");
    Ptr out = std::make_shared<PointCloud>(made, ctx);
    if (kept) kept->resize(out->size());
    return out;
  }
  /// This cloud without its isolated returns, as a new cloud on the device (sga_cloud_remove_outliers): the order, the normals, the
  /// covariances and the origin are kept.  kdtree: the handle of the KdTree over this cloud (KdTree::h), or null: a temporary one is
  /// built.  kept / stat / stats (optional): the indices kept, ascending; the statistic of every point in this cloud's order; its mean,
  /// stddev and threshold.  A cloud with a non-finite coordinate is refused: crop first.
  Ptr without_outliers(const OutlierFilter& filter = OutlierFilter(), const sga_index* kdtree = nullptr, std::vector<int64_t>* kept = nullptr, std::vector<double>* stat = nullptr, sga_outlier_stats* stats = nullptr) const {
    sga_cloud* made = nullptr;
    if (kept) kept->resize(size());
    if (stat) stat->resize(size());
    check(sga_cloud_remove_outliers(ctx, h, kdtree, &filter, kept && !kept->empty() ? kept->data() : nullptr, stat && !stat->empty() ? stat->data() : nullptr, stats, &made), "sga_cloud_remove_outliers");
    Ptr out = std::make_shared<PointCloud>(made, ctx);
    if (kept) kept->resize(out->size());
    return out;
  }
  /// How much of this cloud, posed by T (cloud -> target; null: the identity), the target already explains, and which points are new
  /// (sga_cloud_overlap).  target: the handle of a KdTree, a GaussianVoxelMap or a flat map (their member h).  with_dist / with_nearest /
  /// with_kept: also fill OverlapResult's per-point arrays (kept needs a keep other than None).
  OverlapResult overlap(const sga_index* target, const Isometry3d* T = nullptr, const Overlap& what = Overlap(), bool with_dist = false, bool with_nearest = false, bool with_kept = false) const {
    OverlapResult r;
    sga_overlap p;
    sga_overlap_default(&p);
    p.max_distance = what.max_distance, p.keep = static_cast<int>(what.keep);
    const size_t n = size();
    if (with_dist) r.dist.resize(n);
    if (with_nearest) r.nearest.resize(n);
    if (with_kept) r.kept.resize(n);
    sga_cloud* made = nullptr;
    check(sga_cloud_overlap(ctx, h, target, T ? T->data() : nullptr, &p, r.dist.empty() ? nullptr : r.dist.data(), r.nearest.empty() ? nullptr : r.nearest.data(), r.kept.empty() ? nullptr : r.kept.data(), &r.stats,
                            p.keep != 0 ? &made : nullptr),
          "sga_cloud_overlap");
    if (p.keep != 0) {
      r.cloud = std::make_shared<PointCloud>(made, ctx);
      r.kept.resize(with_kept ? r.cloud->size() : 0);
    }
    return r;
  }
  /// The free-space check with this cloud as the map (sga_cloud_visibility): which of its points does `scan`, posed by T (the scan's sensor
  /// frame — x forward, y left, z up — into this cloud's frame; null: the identity), see through?  with_state / with_clearance /
  /// with_image / with_kept: also fill VisibilityResult's arrays (kept needs a keep other than None).
  VisibilityResult visibility(const PointCloud& scan, const Isometry3d* T = nullptr, const Visibility& what = Visibility(), bool with_state = false, bool with_clearance = false, bool with_image = false,
                              bool with_kept = false) const {
    VisibilityResult r;
    const size_t n = size();
    if (with_state) r.state.resize(n);
    if (with_clearance) r.clearance.resize(n);
    if (with_image) r.range_image.resize(static_cast<size_t>(what.width > 0 ? what.width : 0) * static_cast<size_t>(what.height > 0 ? what.height : 0));
    if (with_kept) r.kept.resize(n);
    sga_cloud* made = nullptr;
    check(sga_cloud_visibility(ctx, h, scan.h, T ? T->data() : nullptr, &what, r.state.empty() ? nullptr : r.state.data(), r.clearance.empty() ? nullptr : r.clearance.data(),
                               r.range_image.empty() ? nullptr : r.range_image.data(), r.kept.empty() ? nullptr : r.kept.data(), &r.stats, what.keep != 0 ? &made : nullptr),
          "sga_cloud_visibility");
    if (what.keep != 0) {
      r.cloud = std::make_shared<PointCloud>(made, ctx);
      r.kept.resize(with_kept ? r.cloud->size() : 0);
    }
    return r;
  }
  /// The objects of this cloud (sga_cloud_cluster): labels, counts and a table of up to table_capacity clusters.  kdtree: the handle of
  /// the KdTree over this cloud, or null: a temporary one is built.  A cloud with a non-finite coordinate is refused: crop first.
  Clusters clusters(const ClusterParams& params = ClusterParams(), const sga_index* kdtree = nullptr, size_t table_capacity = 1024) const {
    Clusters r;
    const size_t n = size();
    r.labels.resize(n);
    r.table.resize(table_capacity);
    if (params.keep != 0) r.kept.resize(n);
    sga_cloud* made = nullptr;
    check(sga_cloud_cluster(ctx, h, kdtree, &params, r.labels.empty() ? nullptr : r.labels.data(), r.table.empty() ? nullptr : r.table.data(), table_capacity, r.kept.empty() ? nullptr : r.kept.data(), &r.counts,
                            params.keep != 0 ? &made : nullptr),
          "sga_cloud_cluster");
    r.table.resize(static_cast<size_t>(r.counts.rows));
    if (params.keep != 0) {
      r.cloud = std::make_shared<PointCloud>(made, ctx);
      r.kept.resize(r.cloud->size());
    }
    return r;
  }
  /// The dominant plane of this cloud (sga_cloud_segment_plane): a function of the records, the parameters and the seed alone.
  /// with_scores: also the score of every hypothesis (0xFFFFFFFF: dropped); with a keep other than None the cloud and its indices.
  Plane segment_plane(const PlaneParams& params = PlaneParams(), bool with_scores = false) const {
    Plane r;
    if (with_scores) r.scores.resize(params.iterations >= 1 && params.iterations <= (1ull << 20) ? static_cast<size_t>(params.iterations) : 1);
    if (params.keep != 0) r.kept.resize(size());
    sga_cloud* made = nullptr;
    check(sga_cloud_segment_plane(ctx, h, &params, r.coefficients.data(), r.scores.empty() ? nullptr : r.scores.data(), r.kept.empty() ? nullptr : r.kept.data(), params.keep != 0 ? &made : nullptr, &r.result),
          "sga_cloud_segment_plane");
    if (params.keep != 0) {
      r.cloud = std::make_shared<PointCloud>(made, ctx);
      r.kept.resize(r.cloud->size());
    }
    return r;
  }
  /// The salient points of this cloud (sga_cloud_iss_keypoints): a function of the records, the tree and the parameters alone.
  /// kdtree: the handle of the KdTree over this cloud, or null: a temporary one is built.  with_saliency: also the saliency per point.
  Keypoints iss_keypoints(const IssParams& params, const sga_index* kdtree = nullptr, bool with_saliency = false) const {
    Keypoints r;
    const size_t n = size();
    r.indices.resize(n);
    if (with_saliency) r.saliency.resize(n);
    size_t count = 0;
    sga_cloud* made = nullptr;
    check(sga_cloud_iss_keypoints(ctx, h, kdtree, &params, r.saliency.empty() ? nullptr : r.saliency.data(), r.indices.empty() ? nullptr : r.indices.data(), &count, params.keep != 0 ? &made : nullptr),
          "sga_cloud_iss_keypoints");
    r.indices.resize(count);
    if (params.keep != 0) r.cloud = std::make_shared<PointCloud>(made, ctx);
    return r;
  }
  /// One 33-bin Fast Point Feature Histogram per point (sga_cloud_fpfh); the cloud needs normals.  kdtree: the handle of the KdTree over
  /// this cloud, or null: a temporary one is built.  viewpoint (optional, the caller's frame): the normals are turned towards it for
  /// the descriptor; nothing is written back.
  Features::Ptr fpfh(const sga_index* kdtree = nullptr, int k = 20, const std::array<double, 3>* viewpoint = nullptr) const {
    sga_features* made = nullptr;
    check(sga_cloud_fpfh(ctx, h, kdtree, k, viewpoint ? viewpoint->data() : nullptr, &made), "sga_cloud_fpfh");
    return std::make_shared<Features>(made, ctx);
  }
  /// The Scan Context descriptor of this cloud (sga_cloud_scan_context): rings x sectors floats, row-major.  center (optional): the
  /// sensor's position in the cloud's coordinates.
  std::vector<float> scan_context(const PlaceParams& params = PlaceParams(), const std::array<double, 3>* center = nullptr) const {
    std::vector<float> image(params.rings > 0 && params.sectors > 0 ? static_cast<size_t>(params.rings) * static_cast<size_t>(params.sectors) : 1);
    check(sga_cloud_scan_context(ctx, h, &params, center ? center->data() : nullptr, image.data()), "sga_cloud_scan_context");
    return image;
  }
  /// A new cloud whose point j is this cloud's point indices[j] with its normal and covariance (sga_cloud_select: one launch); repeats
  /// are allowed, the order is as given.
  Ptr selected(const std::vector<int64_t>& indices) const {
    sga_cloud* made = nullptr;
    check(sga_cloud_select(ctx, h, indices.data(), indices.size(), &made), "sga_cloud_select");
    return std::make_shared<PointCloud>(made, ctx);
  }

  size_t size() const {
    size_t n = 0;
    sga_cloud_size(h, &n);
    return n;
  }
  bool empty() const { return size() == 0; }
  bool has_normals() const {
    int a = 0, b = 0;
    sga_cloud_has(h, &a, &b);
    return a != 0;
  }
  bool has_covs() const {
    int a = 0, b = 0;
    sga_cloud_has(h, &a, &b);
    return b != 0;
  }
  /// (x, y, z, 1) of point i
  std::array<double, 4> point(size_t i) const {
    sync_host();
    return {host_xyz[3 * i], host_xyz[3 * i + 1], host_xyz[3 * i + 2], 1.0};
  }
  std::array<double, 4> normal(size_t i) const {
    sync_host();
    if (host_nrm.empty()) return {0, 0, 0, 0};
    return {host_nrm[3 * i], host_nrm[3 * i + 1], host_nrm[3 * i + 2], 0.0};
  }
  /// 4x4 covariance (3x3 block + zero padding), column-major
  std::array<double, 16> cov(size_t i) const {
    sync_host();
    std::array<double, 16> c{};
    if (host_cov.empty()) return c;
    const float* s = &host_cov[6 * i];
    c[0] = s[0], c[1] = s[1], c[2] = s[2], c[4] = s[1], c[5] = s[3], c[6] = s[4], c[8] = s[2], c[9] = s[4], c[10] = s[5];
    return c;
  }
  void invalidate_host() const { host_valid = false; }

  sga_context* ctx = default_context();
  sga_cloud* h = nullptr;

private:
  void sync_host() const {
    if (host_valid) return;
    const size_t n = size();
    host_xyz.assign(3 * n, 0.0);
    host_nrm.assign(has_normals() ? 3 * n : 0, 0.f);
    host_cov.assign(has_covs() ? 6 * n : 0, 0.f);
    check(sga_cloud_download_f64(ctx, h, host_xyz.data(), host_nrm.empty() ? nullptr : host_nrm.data(), host_cov.empty() ? nullptr : host_cov.data()), "sga_cloud_download_f64");  // device record + origin, in double
    host_valid = true;
  }
  mutable bool host_valid = false;
  mutable std::vector<double> host_xyz;
  mutable std::vector<float> host_nrm, host_cov;
};

/// Place recognition (sga_places_*): the Scan Context descriptors of keyframes on the device, searched exhaustively at every column
/// shift.  add() forms a descriptor on the device, where it stays; query() returns the k nearest entries by ascending (distance, index),
/// each with the shift that aligns it: the yaw between the two visits is shift * 2 pi / sectors.
struct Places {
  explicit Places(const PlaceParams& params_ = PlaceParams(), sga_context* context = default_context()) : ctx(context), params(params_) { check(sga_places_create(ctx, &params, &h), "sga_places_create"); }
  Places(const Places&) = delete;
  Places& operator=(const Places&) = delete;
  ~Places() { sga_places_destroy(h); }
  size_t size() const {
    size_t n = 0;
    sga_places_size(h, &n);
    return n;
  }
  size_t cells() const { return static_cast<size_t>(params.rings) * static_cast<size_t>(params.sectors); }
  /// the descriptor of `cloud` becomes the next entry; returns its index
  size_t add(const PointCloud& cloud, const std::array<double, 3>* center = nullptr) {
    size_t index = 0;
    check(sga_places_add(ctx, h, cloud.h, center ? center->data() : nullptr, &index), "sga_places_add");
    return index;
  }
  /// an image of rings x sectors finite values >= 0 becomes the next entry
  size_t add_descriptor(const std::vector<float>& image) {
    if (image.size() != cells()) throw std::runtime_error("Places::add_descriptor: the image must hold rings x sectors values");
    size_t index = 0;
    check(sga_places_add_descriptor(ctx, h, image.data(), &index), "sga_places_add_descriptor");
    return index;
  }
  /// the images of the entries [first, first + count), row-major
  std::vector<float> download(size_t first, size_t count) const {
    std::vector<float> images(count * cells());
    check(sga_places_download(ctx, h, first, count, images.empty() ? nullptr : images.data()), "sga_places_download");
    return images;
  }
  /// the k best of the entries [first, first + count) (count == SIZE_MAX: to the end) for a cloud ...
  std::vector<PlaceMatch> query(const PointCloud& cloud, int k = 1, size_t first = 0, size_t count = SIZE_MAX, const std::array<double, 3>* center = nullptr) const {
    std::vector<PlaceMatch> out(k > 0 ? static_cast<size_t>(k) : 1);
    size_t found = 0;
    check(sga_places_query(ctx, h, cloud.h, center ? center->data() : nullptr, first, span(first, count), k, out.data(), &found, nullptr, nullptr), "sga_places_query");
    out.resize(found);
    return out;
  }
  /// ... or for an image
  std::vector<PlaceMatch> query(const std::vector<float>& image, int k = 1, size_t first = 0, size_t count = SIZE_MAX) const {
    if (image.size() != cells()) throw std::runtime_error("Places::query: the image must hold rings x sectors values");
    std::vector<PlaceMatch> out(k > 0 ? static_cast<size_t>(k) : 1);
    size_t found = 0;
    check(sga_places_query_descriptor(ctx, h, image.data(), first, span(first, count), k, out.data(), &found, nullptr, nullptr), "sga_places_query_descriptor");
    out.resize(found);
    return out;
  }
  /// the rotation about z by shift * 2 pi / sectors: the initial guess T_entry^-1 T_query a shift stands for
  Isometry3d yaw_guess(int shift) const {
    const double a = static_cast<double>(shift) * (2.0 * M_PI / static_cast<double>(params.sectors));
    Isometry3d T;
    T.m = {std::cos(a), std::sin(a), 0, 0, -std::sin(a), std::cos(a), 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    return T;
  }

  sga_context* ctx = default_context();
  PlaceParams params;
  sga_places* h = nullptr;

private:
  size_t span(size_t first, size_t count) const {
    const size_t n = size();
    return count == SIZE_MAX ? (first < n ? n - first : 0) : count;
  }
};

/// Where an OccupancyGrid lies and how it weighs evidence (sga_occupancy_params: the box's minimum corner, the leaf, the dims; the
/// log-odds of a hit and a miss and their clamps, OctoMap's by default).
struct OccupancyParams : sga_occupancy_params {
  OccupancyParams() { sga_occupancy_params_default(this); }
  OccupancyParams(const std::array<double, 3>& origin_, double leaf_, const std::array<int, 3>& dims_) {
    sga_occupancy_params_default(this);
    for (int k = 0; k < 3; k++) origin[k] = origin_[k], dims[k] = dims_[k];
    leaf = leaf_;
  }
};
/// What OccupancyGrid::classify found: the points per state with the epoch, the cloud of the kept points (null when keep_mask is 0)
/// and — where asked for — the state per point and the indices of the output cloud's points, ascending.
struct OccupancyClassified {
  sga_occupancy_counts counts{};
  std::shared_ptr<PointCloud> cloud;
  std::vector<uint8_t> state;
  std::vector<int64_t> kept;
};
/// What OccupancyGrid::export_cells found: the number of selected cells (whatever the capacity), the first of them in ascending linear
/// index (z * ny + y) * nx + x with their log-odds, and the cloud of their centres.
struct OccupancyCells {
  size_t count = 0;
  std::vector<int64_t> indices;
  std::vector<float> log_odds;
  std::shared_ptr<PointCloud> cloud;
};
/// A dense occupancy grid on the device (sga_occupancy_*): posed scans are ray-cast into it — free space along every beam, an endpoint
/// at every return within range — and it answers unknown / free / occupied for points and cells.
class OccupancyGrid {
public:
  enum State : uint8_t { Unknown = 0, Free = 1, Occupied = 2 };
  enum Mask { UnknownBit = 1, FreeBit = 2, OccupiedBit = 4 };
  explicit OccupancyGrid(const OccupancyParams& params_, sga_context* context = default_context()) : ctx(context), params(params_) { check(sga_occupancy_create(ctx, &params, &h), "sga_occupancy_create"); }
  OccupancyGrid(const OccupancyGrid&) = delete;
  OccupancyGrid& operator=(const OccupancyGrid&) = delete;
  ~OccupancyGrid() { sga_occupancy_destroy(h); }
  size_t cells() const { return static_cast<size_t>(params.dims[0]) * static_cast<size_t>(params.dims[1]) * static_cast<size_t>(params.dims[2]); }
  uint64_t epoch() const {
    uint64_t e = 0;
    check(sga_occupancy_get(h, nullptr, &e), "sga_occupancy_get");
    return e;
  }
  void clear() { check(sga_occupancy_clear(ctx, h), "sga_occupancy_clear"); }
  /// Ray-cast `scan` (sensor frame; T: sensor frame -> world, null: the identity).  mode 1: the endpoints only.  No host wait.
  void integrate(const PointCloud& scan, const Isometry3d* T = nullptr, double min_range = 0.5, double max_range = 60.0, int mode = 0) {
    check(sga_occupancy_integrate(ctx, h, scan.h, T ? T->data() : nullptr, min_range, max_range, mode, nullptr), "sga_occupancy_integrate");
  }
  /// ... and wait once for the scan's statistics
  sga_occupancy_scan_stats integrate_with_stats(const PointCloud& scan, const Isometry3d* T = nullptr, double min_range = 0.5, double max_range = 60.0, int mode = 0) {
    sga_occupancy_scan_stats st{};
    check(sga_occupancy_integrate(ctx, h, scan.h, T ? T->data() : nullptr, min_range, max_range, mode, &st), "sga_occupancy_integrate");
    return st;
  }
  /// The state of every point of `cloud` posed by T; keep_mask (Mask bits) other than 0: also the cloud of the points in those states.
  OccupancyClassified classify(const PointCloud& cloud, const Isometry3d* T = nullptr, double threshold = 0.0, int keep_mask = 0, bool with_state = false, bool with_kept = false) const {
    OccupancyClassified r;
    const size_t n = cloud.size();
    if (with_state) r.state.resize(n);
    if (with_kept) r.kept.resize(n);
    sga_cloud* made = nullptr;
    check(sga_occupancy_classify(ctx, h, cloud.h, T ? T->data() : nullptr, threshold, keep_mask, r.state.empty() ? nullptr : r.state.data(), r.kept.empty() ? nullptr : r.kept.data(), &r.counts, keep_mask != 0 ? &made : nullptr),
          "sga_occupancy_classify");
    if (keep_mask != 0) {
      r.cloud = std::make_shared<PointCloud>(made, ctx);
      r.kept.resize(with_kept ? r.cloud->size() : 0);
    }
    return r;
  }
  sga_occupancy_counts stats(double threshold = 0.0) const {
    sga_occupancy_counts c{};
    check(sga_occupancy_stats(ctx, h, threshold, &c), "sga_occupancy_stats");
    return c;
  }
  /// The cells in the states of which_mask, at most `capacity` of them (SIZE_MAX: the cells)
  OccupancyCells export_cells(double threshold = 0.0, int which_mask = OccupiedBit, size_t capacity = SIZE_MAX, bool with_cloud = true) const {
    OccupancyCells r;
    const size_t cap = capacity == SIZE_MAX ? cells() : capacity;
    r.indices.resize(cap);
    r.log_odds.resize(cap);
    sga_cloud* made = nullptr;
    check(sga_occupancy_export(ctx, h, threshold, which_mask, cap, cap ? r.indices.data() : nullptr, cap ? r.log_odds.data() : nullptr, &r.count, with_cloud ? &made : nullptr), "sga_occupancy_export");
    r.indices.resize(r.count < cap ? r.count : cap);
    r.log_odds.resize(r.indices.size());
    if (with_cloud) r.cloud = std::make_shared<PointCloud>(made, ctx);
    return r;
  }
  /// the centres of the occupied cells
  std::shared_ptr<PointCloud> occupied_cloud(double threshold = 0.0) const {
    size_t count = 0;
    sga_cloud* made = nullptr;
    check(sga_occupancy_export(ctx, h, threshold, OccupiedBit, cells(), nullptr, nullptr, &count, &made), "sga_occupancy_export");
    return std::make_shared<PointCloud>(made, ctx);
  }
  /// the raw arrays, cell (x, y, z) at (z * ny + y) * nx + x
  void download(std::vector<uint32_t>& stamp, std::vector<float>& log_odds) const {
    stamp.resize(cells());
    log_odds.resize(cells());
    check(sga_occupancy_download(ctx, h, stamp.data(), log_odds.data()), "sga_occupancy_download");
  }

  sga_context* ctx = default_context();
  OccupancyParams params;
  sga_occupancy* h = nullptr;
};

/// The rigid motion most of the index pairs (source point, target point) agree on (sga_ransac_correspondences): hypotheses from three
/// pairs each, scored by the pairs within max_distance, the best refitted over its inliers.  Fewer than three pairs, or no hypothesis
/// that passed the tests: inliers 0 and the identity.
inline RansacResult ransac_correspondences(const PointCloud& source, const PointCloud& target, const std::vector<std::array<int64_t, 2>>& pairs, const Ransac& params = Ransac()) {
  RansacResult r;
  check(sga_ransac_correspondences(source.ctx, source.h, target.h, pairs.empty() ? nullptr : pairs.data()->data(), pairs.size(), &params, r.T_target_source.m.data(), &r), "sga_ransac_correspondences");
  return r;
}

/// Up to max_planes planes of a cloud, one after the other (a host loop over PointCloud::segment_plane): round r runs with seed + r and
/// keep Rest on what round r - 1 left, and stops at the first round that finds fewer than min_inliers points.
inline Planes segment_planes(const std::shared_ptr<const PointCloud>& cloud, size_t max_planes, PlaneParams params = PlaneParams()) {
  Planes out;
  const size_t n = cloud->size();
  out.labels.assign(n, -1);
  out.rest_indices.resize(n);
  for (size_t i = 0; i < n; i++) out.rest_indices[i] = static_cast<int64_t>(i);
  std::shared_ptr<const PointCloud> rest = cloud;
  params.keep = PlaneParams::Rest;
  const uint64_t seed = params.seed;
  for (size_t r = 0; r < max_planes; r++) {
    params.seed = seed + r;
    Plane p = rest->segment_plane(params);
    if (p.result.inliers < params.min_inliers) break;
    std::vector<int64_t> index(p.kept.size());
    size_t k = 0;
    for (size_t i = 0; i < out.rest_indices.size(); i++) {
      if (k < p.kept.size() && p.kept[k] == static_cast<int64_t>(i))
        index[k++] = out.rest_indices[i];
      else
        out.labels[static_cast<size_t>(out.rest_indices[i])] = static_cast<int32_t>(r);
    }
    out.rest_indices.swap(index);
    rest = p.cloud;
    p.cloud.reset();
    p.kept.clear();
    out.planes.push_back(std::move(p));
  }
  out.rest = std::const_pointer_cast<PointCloud>(rest);
  return out;
}

/// kNN for m queries in device memory against a kd-tree, a Gaussian or a flat voxel map (sga_index_knn_device): d_idx m*k int64 and
/// d_sq_dist m*k floats are device memory of the caller's; -1 / inf = none.
inline void knn_device(sga_context* ctx, const sga_index* index, const sga_device_array& queries, size_t m, int k, int64_t* d_idx, float* d_sq_dist, double max_sq_dist = -1.0, void* stream = nullptr, int flags = 0) {
  check(sga_index_knn_device(ctx, index, &queries, m, k, max_sq_dist, d_idx, d_sq_dist, stream, flags), "sga_index_knn_device");
}

/// ann/kdtree.hpp:248-291 KdTree<PointCloud>: exact nearest-neighbour index over a cloud (GPU kd-tree).
struct KdTree {
  using Ptr = std::shared_ptr<KdTree>;
  explicit KdTree(std::shared_ptr<const PointCloud> pts) : points(std::move(pts)) { check(sga_index_build_kdtree(points->ctx, points->h, &h), "sga_index_build_kdtree"); }
  /// takes over an index built over `pts` (build_kdtrees)
  KdTree(std::shared_ptr<const PointCloud> pts, sga_index* built) : points(std::move(pts)), h(built) {}
  KdTree(const KdTree&) = delete;
  KdTree& operator=(const KdTree&) = delete;
  ~KdTree() { sga_index_destroy(h); }
  /// traits::knn_search (ann/traits.hpp:22-25) for one query (x, y, z[, 1]); returns the number of neighbours found
  size_t knn_search(const double* pt, size_t k, size_t* k_indices, double* k_sq_dists) const {
    const float q[3] = {static_cast<float>(pt[0]), static_cast<float>(pt[1]), static_cast<float>(pt[2])};
    std::vector<int64_t> idx(k);
    std::vector<float> d2(k);
    check(sga_index_knn(points->ctx, h, q, 1, static_cast<int>(k), -1.0, idx.data(), d2.data()), "sga_index_knn");
    size_t found = 0;
    for (size_t j = 0; j < k; j++)
      if (idx[j] >= 0) {
        k_indices[found] = static_cast<size_t>(idx[j]);
        k_sq_dists[found] = d2[j];
        found++;
      }
    return found;
  }
  size_t nearest_neighbor_search(const double* pt, size_t* k_index, double* k_sq_dist) const { return knn_search(pt, 1, k_index, k_sq_dist); }
  /// The indexed points within radius of every point of `queries` (sga_index_radius_search; d2 <= radius^2 in double): the counts and,
  /// with_lists, the CSR lists (indices into the indexed cloud, squared distances), in the walk's order within a list.
  RadiusNeighbors radius_search(const PointCloud& queries, double radius, bool with_lists = true) const {
    RadiusNeighbors r;
    const size_t m = queries.size();
    r.counts.resize(m + 1);  // (never empty: the library wants a place for the counts)
    sga_radius_result res{};
    check(sga_index_radius_search(points->ctx, h, queries.h, radius, 0, r.counts.data(), nullptr, nullptr, nullptr, &res), "sga_index_radius_search");
    if (with_lists) {
      r.offsets.resize(m + 1);
      r.indices.resize(static_cast<size_t>(res.total) + 1);
      r.sq_dists.resize(static_cast<size_t>(res.total) + 1);
      check(sga_index_radius_search(points->ctx, h, queries.h, radius, static_cast<size_t>(res.total), r.counts.data(), r.offsets.data(), r.indices.data(), r.sq_dists.data(), &res), "sga_index_radius_search");
      r.indices.resize(static_cast<size_t>(res.total));
      r.sq_dists.resize(static_cast<size_t>(res.total));
    }
    r.counts.resize(m);
    return r;
  }

  std::shared_ptr<const PointCloud> points;
  sga_index* h = nullptr;
};

/// ann/projective_search.hpp:158-183 ProjectiveSearch<PointCloud>(width, height, points): the equirectangular index image of the points
/// (y down, z forward), searched over the (2 h + 1) x (2 v + 1) window around the query's pixel, BorderRepeat horizontally and
/// BorderClamp vertically.  search_window_h / search_window_v are public as in the reference (:153-154) and honoured at every search
/// and align.  Indices are the cloud's own; distances are double (sga_index_knn_f64).
struct ProjectiveSearch {
  using Ptr = std::shared_ptr<ProjectiveSearch>;
  using ConstPtr = std::shared_ptr<const ProjectiveSearch>;
  ProjectiveSearch(int width, int height, std::shared_ptr<const PointCloud> pts) : points(std::move(pts)) {
    check(sga_index_build_projective(points->ctx, points->h, width, height, &h), "sga_index_build_projective");
  }
  ProjectiveSearch(const ProjectiveSearch&) = delete;
  ProjectiveSearch& operator=(const ProjectiveSearch&) = delete;
  ~ProjectiveSearch() { sga_index_destroy(h); }
  /// the public window, pushed to the index before it is used
  void sync() const { check(sga_projective_set_search_window(h, search_window_h, search_window_v), "sga_projective_set_search_window"); }
  size_t knn_search(const double* pt, size_t k, size_t* k_indices, double* k_sq_dists) const {
    sync();
    std::vector<int64_t> idx(k);
    std::vector<double> d2(k);
    check(sga_index_knn_f64(points->ctx, h, pt, 1, static_cast<int>(k), -1.0, idx.data(), d2.data()), "sga_index_knn_f64");
    size_t found = 0;
    for (size_t j = 0; j < k; j++)
      if (idx[j] >= 0) {
        k_indices[found] = static_cast<size_t>(idx[j]);
        k_sq_dists[found] = d2[j];
        found++;
      }
    return found;
  }
  size_t nearest_neighbor_search(const double* pt, size_t* k_index, double* k_sq_dist) const { return knn_search(pt, 1, k_index, k_sq_dist); }

  std::shared_ptr<const PointCloud> points;
  sga_index* h = nullptr;
  int search_window_h = 10;
  int search_window_v = 5;
};

/// traits::knn_search / nearest_neighbor_search of a voxel map (ann/incremental_voxelmap.hpp:99-149) for one query: global indices
/// (voxel_id << 32) | point_id, squared distances ascending; returns the number found
inline size_t voxelmap_knn_search(sga_context* ctx, const sga_index* h, const double* pt, size_t k, size_t* k_indices, double* k_sq_dists) {
  if (!h) return 0;
  std::vector<int64_t> idx(k);
  std::vector<double> d2(k);
  check(sga_index_knn_f64(ctx, h, pt, 1, static_cast<int>(k), -1.0, idx.data(), d2.data()), "sga_index_knn_f64");
  size_t found = 0;
  for (size_t j = 0; j < k; j++)
    if (idx[j] >= 0) {
      k_indices[found] = static_cast<size_t>(idx[j]);
      k_sq_dists[found] = d2[j];
      found++;
    }
  return found;
}

/// ann/gaussian_voxelmap.hpp + incremental_voxelmap.hpp: one-shot Gaussian voxel map (VGICP target).
struct GaussianVoxelMap {
  using Ptr = std::shared_ptr<GaussianVoxelMap>;
  explicit GaussianVoxelMap(double leaf_size) : leaf(leaf_size) {}
  GaussianVoxelMap(const GaussianVoxelMap&) = delete;
  GaussianVoxelMap& operator=(const GaussianVoxelMap&) = delete;
  ~GaussianVoxelMap() { sga_index_destroy(h); }
  // ann/incremental_voxelmap.hpp:55-92: any number of inserts, each with a pose; LRU removal of voxels not touched recently
  void insert(const PointCloud& points, const Isometry3d& T = Isometry3d::Identity()) {
    if (!h) {
      ctx = points.ctx;
      check(sga_voxelmap_create(ctx, leaf, &h), "sga_voxelmap_create");
      check(sga_voxelmap_set_lru(h, static_cast<uint32_t>(lru_horizon), static_cast<uint32_t>(lru_clear_cycle)), "sga_voxelmap_set_lru");
    }
    check(sga_voxelmap_insert(ctx, h, points.h, T.data()), "sga_voxelmap_insert");
  }
  size_t lru_horizon = 100, lru_clear_cycle = 10;  // set before the first insert (incremental_voxelmap.hpp:46)
  size_t size() const {
    size_t n = 0;
    if (h) sga_index_size(h, &n);
    return n;
  }
  size_t knn_search(const double* pt, size_t k, size_t* k_indices, double* k_sq_dists) const { return voxelmap_knn_search(ctx, h, pt, k, k_indices, k_sq_dists); }
  size_t nearest_neighbor_search(const double* pt, size_t* k_index, double* k_sq_dist) const { return knn_search(pt, 1, k_index, k_sq_dist); }
  static size_t voxel_id(size_t i) { return i >> 32; }          // incremental_voxelmap.hpp:153-154
  static size_t point_id(size_t i) { return i & 0xffffffffull; }
  double leaf;
  sga_context* ctx = nullptr;
  sga_index* h = nullptr;
};

// ann/flat_container.hpp + ann/incremental_voxelmap.hpp: IncrementalVoxelMap<FlatContainer<HasNormals, HasCovs>>, the scan-to-model
// targets (flat_container.hpp:18-58 and its aliases FlatContainerPoints / Normal / Cov / NormalCov).  `contents` selects what the device
// map keeps next to the points (sga_flatmap_create_contents); an insert needs exactly those attributes.  Points: ICP; Normal: ICP and
// PLANE_ICP (Faster-LIO's linear iVox); Cov: ICP and GICP (odometry_benchmark_small_gicp_model_omp.cpp); NormalCov: all three.
template <int Contents>
struct FlatContainer {
  static constexpr int contents = Contents;
  struct Setting {
    double min_sq_dist_in_cell = 0.1 * 0.1;
    size_t max_num_points_in_cell = 10;
  };
};
using FlatContainerPoints = FlatContainer<0>;
using FlatContainerNormal = FlatContainer<SGA_FLAT_NORMALS>;
using FlatContainerCov = FlatContainer<SGA_FLAT_COVS>;
using FlatContainerNormalCov = FlatContainer<SGA_FLAT_NORMALS | SGA_FLAT_COVS>;
template <typename VoxelContents>
struct IncrementalVoxelMap {
  using Ptr = std::shared_ptr<IncrementalVoxelMap>;
  explicit IncrementalVoxelMap(double leaf_size) : leaf(leaf_size) {}
  IncrementalVoxelMap(const IncrementalVoxelMap&) = delete;
  IncrementalVoxelMap& operator=(const IncrementalVoxelMap&) = delete;
  ~IncrementalVoxelMap() { sga_index_destroy(h); }
  void insert(const PointCloud& points, const Isometry3d& T = Isometry3d::Identity()) {
    if (!h) {
      ctx = points.ctx;
      check(sga_flatmap_create_contents(ctx, leaf, VoxelContents::contents, &h), "sga_flatmap_create_contents");
      check(sga_flatmap_set_setting(h, voxel_setting.min_sq_dist_in_cell, static_cast<uint32_t>(voxel_setting.max_num_points_in_cell)), "sga_flatmap_set_setting");
      check(sga_voxelmap_set_lru(h, static_cast<uint32_t>(lru_horizon), static_cast<uint32_t>(lru_clear_cycle)), "sga_voxelmap_set_lru");
      check(sga_voxelmap_set_search_offsets(h, num_search_offsets), "sga_voxelmap_set_search_offsets");
    }
    check(sga_voxelmap_insert(ctx, h, points.h, T.data()), "sga_voxelmap_insert");
  }
  void set_search_offsets(int num_offsets) {
    num_search_offsets = num_offsets;
    if (h) check(sga_voxelmap_set_search_offsets(h, num_offsets), "sga_voxelmap_set_search_offsets");
  }
  size_t size() const {
    size_t n = 0;
    if (h) sga_index_size(h, &n);
    return n;
  }
  size_t knn_search(const double* pt, size_t k, size_t* k_indices, double* k_sq_dists) const { return voxelmap_knn_search(ctx, h, pt, k, k_indices, k_sq_dists); }
  size_t nearest_neighbor_search(const double* pt, size_t* k_index, double* k_sq_dist) const { return knn_search(pt, 1, k_index, k_sq_dist); }
  static size_t voxel_id(size_t i) { return i >> 32; }          // incremental_voxelmap.hpp:153-154
  static size_t point_id(size_t i) { return i & 0xffffffffull; }
  double leaf;
  size_t lru_horizon = 100, lru_clear_cycle = 10;  // set before the first insert
  typename VoxelContents::Setting voxel_setting;    // set before the first insert
  int num_search_offsets = 1;
  sga_context* ctx = nullptr;
  sga_index* h = nullptr;
};

// ---- util/downsampling.hpp, util/normal_estimation.hpp ------------------------------------------------------------------------
inline PointCloud::Ptr voxelgrid_sampling(const PointCloud& points, double leaf_size) {
  sga_cloud* out = nullptr;
  check(sga_voxelgrid_sampling(points.ctx, points.h, leaf_size, &out), "sga_voxelgrid_sampling");
  return std::make_shared<PointCloud>(out, points.ctx);
}
/// How voxelgrid_sampling reduces a column of per-point fields over the members of a voxel (SGA_REDUCE_*): Nearest is the value of the
/// member nearest the voxel's centroid — one real return's, for a time or a label.
enum class Reduce : int { Mean = SGA_REDUCE_MEAN, Min = SGA_REDUCE_MIN, Max = SGA_REDUCE_MAX, First = SGA_REDUCE_FIRST, Nearest = SGA_REDUCE_NEAREST };
/// What the voxel grid that carries fields returns: the cloud voxelgrid_sampling(cloud, leaf) makes, row v of `fields` the reduced
/// columns of voxel v (null without input fields), counts[v] its members, voxel_of[i] the row of input point i (-1: dropped).
struct GridFields {
  PointCloud::Ptr cloud;
  Features::Ptr fields;
  std::vector<int32_t> counts;
  std::vector<int64_t> voxel_of;
};
/// sga_voxelgrid_sampling_fields: fields one row per point (or null: membership only), ops one per column (empty: Mean each)
inline GridFields voxelgrid_sampling(const PointCloud& cloud, const Features* fields, const std::vector<Reduce>& ops, double leaf_size, bool want_counts = false, bool want_voxel_of = false) {
  GridFields r;
  const size_t n = cloud.size();
  std::vector<int> op(ops.size());
  for (size_t c = 0; c < ops.size(); c++) op[c] = static_cast<int>(ops[c]);
  if (fields != nullptr && !op.empty() && op.size() != static_cast<size_t>(fields->dim())) throw std::invalid_argument("voxelgrid_sampling: one reduction per column of the fields");
  std::vector<int32_t> counts(want_counts ? n : 0);
  r.voxel_of.resize(want_voxel_of ? n : 0);
  sga_cloud* out = nullptr;
  sga_features* reduced = nullptr;
  check(sga_voxelgrid_sampling_fields(cloud.ctx, cloud.h, fields ? fields->h : nullptr, op.empty() ? nullptr : op.data(), leaf_size, &out, fields ? &reduced : nullptr, counts.empty() ? nullptr : counts.data(),
                                      r.voxel_of.empty() ? nullptr : r.voxel_of.data()),
        "sga_voxelgrid_sampling_fields");
  r.cloud = std::make_shared<PointCloud>(out, cloud.ctx);
  if (fields) r.fields = std::make_shared<Features>(reduced, cloud.ctx);
  if (want_counts) r.counts.assign(counts.begin(), counts.begin() + static_cast<std::ptrdiff_t>(r.cloud->size()));
  return r;
}
inline void estimate_normals(PointCloud& cloud, int num_neighbors = 20) {
  check(sga_estimate_normals_covariances(cloud.ctx, cloud.h, nullptr, num_neighbors, 1), "estimate_normals");
  cloud.invalidate_host();
}
inline void estimate_covariances(PointCloud& cloud, int num_neighbors = 20) {
  check(sga_estimate_normals_covariances(cloud.ctx, cloud.h, nullptr, num_neighbors, 2), "estimate_covariances");
  cloud.invalidate_host();
}
inline void estimate_normals_covariances(PointCloud& cloud, int num_neighbors = 20) {
  check(sga_estimate_normals_covariances(cloud.ctx, cloud.h, nullptr, num_neighbors, 3), "estimate_normals_covariances");
  cloud.invalidate_host();
}
inline void estimate_normals_covariances(PointCloud& cloud, KdTree& tree, int num_neighbors = 20) {
  check(sga_estimate_normals_covariances(cloud.ctx, cloud.h, tree.h, num_neighbors, 3), "estimate_normals_covariances");
  cloud.invalidate_host();
}
/// util/normal_estimation_omp.hpp estimate_covariances_omp(points, tree, k, threads): with the cloud's own tree (which then also holds
/// the covariances in its kd order: ready to be a registration target, or a source by its index)
inline void estimate_covariances(PointCloud& cloud, KdTree& tree, int num_neighbors = 20) {
  check(sga_estimate_normals_covariances(cloud.ctx, cloud.h, tree.h, num_neighbors, 2), "estimate_covariances");
  cloud.invalidate_host();
}
inline void estimate_normals(PointCloud& cloud, KdTree& tree, int num_neighbors = 20) {
  check(sga_estimate_normals_covariances(cloud.ctx, cloud.h, tree.h, num_neighbors, 1), "estimate_normals");
  cloud.invalidate_host();
}
/// sga_voxelgrid_sampling_batch: the voxel grids of several clouds of one context in one chain of launches (each bit-identical to voxelgrid_sampling(cloud))
inline std::vector<PointCloud::Ptr> voxelgrid_sampling_batch(sga_context* ctx, const std::vector<std::shared_ptr<const PointCloud>>& clouds, double leaf_size) {
  std::vector<const sga_cloud*> hs;
  for (const auto& c : clouds) hs.push_back(c->h);
  std::vector<sga_cloud*> out(clouds.size(), nullptr);
  check(sga_voxelgrid_sampling_batch(ctx, hs.data(), hs.size(), leaf_size, out.data()), "sga_voxelgrid_sampling_batch");
  std::vector<PointCloud::Ptr> down;
  for (size_t k = 0; k < clouds.size(); k++) down.push_back(std::make_shared<PointCloud>(out[k], ctx));
  return down;
}
/// sga_index_build_kdtree_batch: the kd-trees of several clouds of one context in one chain of launches (each bit-identical to KdTree(cloud))
inline std::vector<KdTree::Ptr> build_kdtrees(sga_context* ctx, const std::vector<std::shared_ptr<const PointCloud>>& clouds) {
  std::vector<const sga_cloud*> hs;
  for (const auto& c : clouds) hs.push_back(c->h);
  std::vector<sga_index*> out(clouds.size(), nullptr);
  check(sga_index_build_kdtree_batch(ctx, hs.data(), hs.size(), out.data()), "sga_index_build_kdtree_batch");
  std::vector<KdTree::Ptr> trees;
  for (size_t k = 0; k < clouds.size(); k++) trees.push_back(std::make_shared<KdTree>(clouds[k], out[k]));
  return trees;
}
/// sga_estimate_normals_covariances_batch (covariances): trees[k] must have been built over clouds[k]
inline void estimate_covariances(sga_context* ctx, const std::vector<std::shared_ptr<PointCloud>>& clouds, const std::vector<KdTree::Ptr>& trees, int num_neighbors = 20) {
  std::vector<sga_cloud*> cs;
  std::vector<sga_index*> ts;
  for (const auto& c : clouds) cs.push_back(c->h);
  for (const auto& t : trees) ts.push_back(t->h);
  if (cs.size() != ts.size()) throw std::runtime_error("estimate_covariances: as many trees as clouds");
  check(sga_estimate_normals_covariances_batch(ctx, cs.data(), ts.data(), cs.size(), num_neighbors, 2), "sga_estimate_normals_covariances_batch");
  for (const auto& c : clouds) c->invalidate_host();
}

// ---- factors (factors/*.hpp): tag types, the per-point state lives on the device ----------------------------------------------------
struct ICPFactor {
  struct Setting {};
  static constexpr int kind = SGA_ICP;
  static void fill(const Setting&, sga_factor_params&) {}
};
struct PointToPlaneICPFactor {
  struct Setting {};
  static constexpr int kind = SGA_PLANE_ICP;
  static void fill(const Setting&, sga_factor_params&) {}
};
struct GICPFactor {
  struct Setting {};
  static constexpr int kind = SGA_GICP;
  static void fill(const Setting&, sga_factor_params&) {}
};
struct Huber {
  struct Setting {
    double c = 1.0;
  };
  static constexpr int kind = SGA_ROBUST_HUBER;
};
struct Cauchy {
  struct Setting {
    double c = 1.0;
  };
  static constexpr int kind = SGA_ROBUST_CAUCHY;
};
template <typename Kernel, typename Factor>
struct RobustFactor {
  struct Setting {
    typename Kernel::Setting robust_kernel;
    typename Factor::Setting factor;
  };
  static constexpr int kind = Factor::kind;
  static void fill(const Setting& s, sga_factor_params& p) {
    p.robust_kind = Kernel::kind;
    p.robust_c = s.robust_kernel.c;
    Factor::fill(s.factor, p);
  }
};

// ---- registration/rejector.hpp, termination_criteria.hpp, factors/general_factor.hpp, optimizer.hpp ---------------------------------
struct NullRejector {
  double max_dist_sq_or_negative() const { return -1.0; }
};
struct DistanceRejector {
  double max_dist_sq = 1.0;
  double max_dist_sq_or_negative() const { return max_dist_sq; }
};
struct TerminationCriteria {
  double translation_eps = 1e-3;
  double rotation_eps = 0.1 * M_PI / 180.0;
};
struct NullFactor {
  void fill(sga_registration_setting&) const {}
};
struct RestrictDoFFactor {
  double lambda = 1e9;
  std::array<double, 6> mask{{1, 1, 1, 1, 1, 1}};  // (rx, ry, rz, tx, ty, tz): 1 = active, 0 = inactive
  void set_rotation_mask(double x, double y, double z) { mask[0] = x, mask[1] = y, mask[2] = z; }
  void set_translation_mask(double x, double y, double z) { mask[3] = x, mask[4] = y, mask[5] = z; }
  void fill(sga_registration_setting& s) const {
    s.restrict_dof_lambda = lambda;
    for (int i = 0; i < 6; i++) s.restrict_dof_mask[i] = mask[i];
  }
};
struct LevenbergMarquardtOptimizer {
  bool verbose = false;
  int max_iterations = 20;
  int max_inner_iterations = 10;
  double init_lambda = 1e-3;
  double lambda_factor = 10.0;
  void fill(sga_registration_setting& s) const {
    s.optimizer = SGA_LEVENBERG_MARQUARDT;
    s.verbose = verbose;
    s.max_iterations = max_iterations;
    s.max_inner_iterations = max_inner_iterations;
    s.init_lambda = init_lambda;
    s.lambda_factor = lambda_factor;
  }
};
struct GaussNewtonOptimizer {
  bool verbose = false;
  int max_iterations = 20;
  double lambda = 1e-6;
  void fill(sga_registration_setting& s) const {
    s.optimizer = SGA_GAUSS_NEWTON;
    s.verbose = verbose;
    s.max_iterations = max_iterations;
    s.gn_lambda = lambda;
  }
};

/// The reduction policy of this library: the slot of SerialReduction / ParallelReductionOMP / ParallelReductionTBB
/// (registration/reduction*.hpp).  linearize / error run as HIP kernels on `device`.
struct ParallelReductionHIP {
  int device = 0;
  int math_mode = SGA_MATH_FP32;
  sga_context* context = nullptr;  // the context (HIP stream) the passes run on; null: the source's.  Registrations on different contexts run side by side
};

/// registration/registration_result.hpp:11-30
struct RegistrationResult {
  explicit RegistrationResult(const Isometry3d& T = Isometry3d::Identity()) : T_target_source(T) {}
  Isometry3d T_target_source;
  bool converged = false;
  size_t iterations = 0;
  size_t num_inliers = 0;
  std::array<double, 36> H{};  // 6x6, symmetric
  std::array<double, 6> b{};
  double error = 0.0;
};

inline RegistrationResult to_result(const sga_result& r) {
  RegistrationResult out;
  std::memcpy(out.T_target_source.m.data(), r.T_target_source, sizeof(double) * 16);
  out.converged = r.converged != 0;
  out.iterations = r.iterations;
  out.num_inliers = r.num_inliers;
  std::memcpy(out.H.data(), r.H, sizeof(double) * 36);
  std::memcpy(out.b.data(), r.b, sizeof(double) * 6);
  out.error = r.error;
  return out;
}

/// registration/registration.hpp:17-54
template <typename PointFactor, typename Reduction = ParallelReductionHIP, typename GeneralFactor = NullFactor, typename CorrespondenceRejector = DistanceRejector, typename Optimizer = LevenbergMarquardtOptimizer>
struct Registration {
  using PointFactorSetting = typename PointFactor::Setting;

  sga_registration_setting make_setting() const {
    sga_registration_setting s;
    sga_registration_setting_default(&s);
    s.factor.factor_kind = PointFactor::kind;
    s.factor.max_dist_sq = rejector.max_dist_sq_or_negative();
    s.factor.math_mode = reduction.math_mode;
    PointFactor::fill(point_factor, s.factor);
    s.translation_eps = criteria.translation_eps;
    s.rotation_eps = criteria.rotation_eps;
    optimizer.fill(s);
    general_factor.fill(s);
    return s;
  }

  /// target_tree: KdTree (ICP / PLANE_ICP / GICP).  `target` is accepted for signature parity; the tree holds the target's data.
  RegistrationResult align(const PointCloud& target, const PointCloud& source, const KdTree& target_tree, const Isometry3d& init_T = Isometry3d::Identity()) const {
    (void)target;
    check(sga_index_refresh_attributes(source.ctx, target_tree.h, target_tree.points->h), "sga_index_refresh_attributes");
    return run(target_tree.h, source, init_T);
  }
  /// The same with the SOURCE given by its own KdTree (an addition to the reference's signature for the odometry loop,
  /// odometry_benchmark_small_gicp_omp.cpp:22-38, where every scan is indexed anyway): sga_problem_create_from_index takes the index's
  /// kd-ordered points and covariances as they are — no spatial sort, no copy.  Both trees must hold the attributes the factor needs
  /// (estimate them with the tree, or build the tree afterwards).
  RegistrationResult align(const PointCloud& target, const KdTree& source_tree, const KdTree& target_tree, const Isometry3d& init_T = Isometry3d::Identity()) const {
    (void)target;
    static_assert(std::is_same<Reduction, ParallelReductionHIP>::value, "this library provides the ParallelReductionHIP reduction only");
    sga_context* ctx = reduction.context ? reduction.context : source_tree.points->ctx;
    const sga_registration_setting s = make_setting();
    sga_problem* pb = nullptr;
    check(sga_problem_create_from_index(ctx, target_tree.h, source_tree.h, init_T.data(), &pb), "sga_problem_create_from_index");
    sga_result r;
    const int rc = sga_align_problem(ctx, pb, init_T.data(), &s, &r);
    sga_problem_destroy(pb);
    check(rc, "sga_align_problem");
    return to_result(r);
  }
  /// target_tree: ProjectiveSearch (ICP / PLANE_ICP / GICP), its search window as the members say at this call
  RegistrationResult align(const PointCloud& target, const PointCloud& source, const ProjectiveSearch& target_tree, const Isometry3d& init_T = Isometry3d::Identity()) const {
    (void)target;
    target_tree.sync();
    check(sga_index_refresh_attributes(source.ctx, target_tree.h, target_tree.points->h), "sga_index_refresh_attributes");
    return run(target_tree.h, source, init_T);
  }
  /// VGICP form (registration_helper.cpp:136: the voxel map is both target cloud and search structure)
  RegistrationResult align(const GaussianVoxelMap& target, const PointCloud& source, const GaussianVoxelMap& target_tree, const Isometry3d& init_T = Isometry3d::Identity()) const {
    (void)target_tree;
    return run(target.h, source, init_T);
  }
  /// scan-to-model forms (odometry_benchmark_small_gicp_model_omp.cpp:33-36): GICPFactor against FlatContainerCov / NormalCov,
  /// PointToPlaneICPFactor against FlatContainerNormal / NormalCov, ICPFactor against any of the four
  template <typename VoxelContents>
  RegistrationResult align(
    const IncrementalVoxelMap<VoxelContents>& target, const PointCloud& source, const IncrementalVoxelMap<VoxelContents>& target_tree, const Isometry3d& init_T = Isometry3d::Identity()) const {
    (void)target_tree;
    return run(target.h, source, init_T);
  }

  TerminationCriteria criteria;
  CorrespondenceRejector rejector;
  PointFactorSetting point_factor;
  GeneralFactor general_factor;
  Reduction reduction;
  Optimizer optimizer;

private:
  RegistrationResult run(const sga_index* index, const PointCloud& source, const Isometry3d& init_T) const {
    static_assert(std::is_same<Reduction, ParallelReductionHIP>::value, "this library provides the ParallelReductionHIP reduction only");
    const sga_registration_setting s = make_setting();
    sga_result r;
    check(sga_align(reduction.context ? reduction.context : source.ctx, index, source.h, init_T.data(), &s, &r), "sga_align");
    return to_result(r);
  }
};

// ---- registration_helper.hpp:15-90 ------------------------------------------------------------------------------------------------
struct RegistrationSetting {
  enum RegistrationType { ICP, PLANE_ICP, GICP, VGICP };
  RegistrationType type = GICP;
  double voxel_resolution = 1.0;
  double downsampling_resolution = 0.25;
  double max_correspondence_distance = 1.0;
  double rotation_eps = 0.1 * M_PI / 180.0;
  double translation_eps = 1e-3;
  int num_threads = 4;  // kept for signature parity; the GPU path ignores it
  int max_iterations = 20;
  bool verbose = false;
};

/// registration_helper.cpp:22-34: downsample -> kd-tree -> normals + covariances
inline std::pair<PointCloud::Ptr, std::shared_ptr<KdTree>> preprocess_points(const PointCloud& points, double downsampling_resolution, int num_neighbors = 10, int num_threads = 4) {
  (void)num_threads;
  auto down = voxelgrid_sampling(points, downsampling_resolution);
  auto tree = std::make_shared<KdTree>(down);
  estimate_normals_covariances(*down, *tree, num_neighbors);
  return {down, tree};
}
template <typename T, size_t D>
std::pair<PointCloud::Ptr, std::shared_ptr<KdTree>> preprocess_points(const std::vector<std::array<T, D>>& points, double downsampling_resolution, int num_neighbors = 10, int num_threads = 4) {
  return preprocess_points(PointCloud(points), downsampling_resolution, num_neighbors, num_threads);
}
/// registration_helper.cpp:50-54
inline GaussianVoxelMap::Ptr create_gaussian_voxelmap(const PointCloud& points, double voxel_resolution) {
  auto vm = std::make_shared<GaussianVoxelMap>(voxel_resolution);
  vm->insert(points);
  return vm;
}
/// sga_index_build_gaussian_voxelmap_batch: the one-shot Gaussian voxel maps of several clouds (with covariances) of one context in one
/// chain of launches and one host wait; every map is a search target whose voxels equal create_gaussian_voxelmap(cloud, voxel_resolution)'s
inline std::vector<GaussianVoxelMap::Ptr> create_gaussian_voxelmaps(sga_context* ctx, const std::vector<std::shared_ptr<const PointCloud>>& clouds, double voxel_resolution) {
  std::vector<const sga_cloud*> hs;
  for (const auto& c : clouds) hs.push_back(c->h);
  std::vector<sga_index*> out(clouds.size(), nullptr);
  check(sga_index_build_gaussian_voxelmap_batch(ctx, hs.data(), hs.size(), voxel_resolution, out.data()), "sga_index_build_gaussian_voxelmap_batch");
  std::vector<GaussianVoxelMap::Ptr> maps;
  for (size_t k = 0; k < clouds.size(); k++) {
    auto vm = std::make_shared<GaussianVoxelMap>(voxel_resolution);
    vm->ctx = ctx;
    vm->h = out[k];
    maps.push_back(vm);
  }
  return maps;
}
/// sga_voxelmap_insert_batch: maps[k]->insert(*clouds[k], Ts[k]) for all k (Ts empty: identities) — the incremental Gaussian maps of several
/// scan-to-model streams of one context updated by one chain of launches and one host wait; every map holds what the lone insert leaves,
/// bit for bit.  A map may appear once per call; a map that has not been inserted into yet is created here, as insert() creates it.
inline void insert_batch(sga_context* ctx, const std::vector<GaussianVoxelMap::Ptr>& maps, const std::vector<std::shared_ptr<const PointCloud>>& clouds, const std::vector<Isometry3d>& Ts = {}) {
  if (maps.size() != clouds.size() || (!Ts.empty() && Ts.size() != maps.size())) throw std::runtime_error("insert_batch: as many maps as clouds (and poses)");
  std::vector<sga_index*> ms;
  std::vector<const sga_cloud*> cs;
  std::vector<double> T16;
  for (size_t k = 0; k < maps.size(); k++) {
    GaussianVoxelMap& vm = *maps[k];
    if (!vm.h) {
      vm.ctx = ctx;
      check(sga_voxelmap_create(ctx, vm.leaf, &vm.h), "sga_voxelmap_create");
      check(sga_voxelmap_set_lru(vm.h, static_cast<uint32_t>(vm.lru_horizon), static_cast<uint32_t>(vm.lru_clear_cycle)), "sga_voxelmap_set_lru");
    }
    ms.push_back(vm.h);
    cs.push_back(clouds[k]->h);
    if (!Ts.empty()) T16.insert(T16.end(), Ts[k].data(), Ts[k].data() + 16);
  }
  check(sga_voxelmap_insert_batch(ctx, ms.data(), cs.data(), Ts.empty() ? nullptr : T16.data(), ms.size()), "sga_voxelmap_insert_batch");
}

/// sga_cloud_merge: the clouds posed by Ts (empty: identities) joined into one cloud — clouds[0]'s points, then clouds[1]'s, ... — by one
/// table copy and one launch whatever their number: the last K keyframes at their estimated poses as one registration target.  Normals
/// and covariances ride along rotated, each kept only if every non-empty member has it.  origin: the output's device-frame origin (NULL:
/// chosen by the library from the bounding box of the posed points, which costs one host wait).
inline PointCloud::Ptr merge_clouds(sga_context* ctx, const std::vector<std::shared_ptr<const PointCloud>>& clouds, const std::vector<Isometry3d>& Ts = {}, const double* origin = nullptr) {
  if (!Ts.empty() && Ts.size() != clouds.size()) throw std::runtime_error("merge_clouds: as many poses as clouds");
  std::vector<const sga_cloud*> cs;
  std::vector<double> T16;
  for (size_t k = 0; k < clouds.size(); k++) {
    cs.push_back(clouds[k]->h);
    if (!Ts.empty()) T16.insert(T16.end(), Ts[k].data(), Ts[k].data() + 16);
  }
  sga_cloud* made = nullptr;
  check(sga_cloud_merge(ctx, cs.data(), Ts.empty() ? nullptr : T16.data(), cs.size(), origin, &made), "sga_cloud_merge");
  return std::make_shared<PointCloud>(made, ctx);
}

/// sga_cloud_deskew_batch: PointCloud::deskewed for B sweeps by one table copy and one launch whatever B is.  times[k]: clouds[k]->size()
/// values; twists[k]: member k's motion per unit of time; ref_times empty: 1.0 each.
inline std::vector<PointCloud::Ptr> deskew_clouds(sga_context* ctx, const std::vector<std::shared_ptr<const PointCloud>>& clouds, const std::vector<const float*>& times, const std::vector<std::array<double, 6>>& twists,
                                                  const std::vector<double>& ref_times = {}) {
  if (times.size() != clouds.size() || twists.size() != clouds.size() || (!ref_times.empty() && ref_times.size() != clouds.size())) throw std::runtime_error("deskew_clouds: as many times, twists and reference times as clouds");
  std::vector<const sga_cloud*> cs;
  std::vector<double> xi;
  for (size_t k = 0; k < clouds.size(); k++) {
    cs.push_back(clouds[k]->h);
    xi.insert(xi.end(), twists[k].begin(), twists[k].end());
  }
  std::vector<sga_cloud*> made(clouds.size(), nullptr);
  check(sga_cloud_deskew_batch(ctx, cs.data(), times.data(), xi.data(), ref_times.empty() ? nullptr : ref_times.data(), cs.size(), made.data()), "sga_cloud_deskew_batch");
  std::vector<PointCloud::Ptr> out;
  for (sga_cloud* h : made) out.push_back(std::make_shared<PointCloud>(h, ctx));
  return out;
}

/// sga_cloud_crop_batch: PointCloud::cropped for B clouds, each under its own crop, by one table copy and one launch whatever B is.
/// kept (optional): kept->at(k) receives the indices kept of clouds[k].
inline std::vector<PointCloud::Ptr> crop_clouds(sga_context* ctx, const std::vector<std::shared_ptr<const PointCloud>>& clouds, const std::vector<Crop>& crops, std::vector<std::vector<int64_t>>* kept = nullptr) {
  if (crops.size() != clouds.size()) throw std::runtime_error("crop_clouds: as many crops as clouds");
  std::vector<const sga_cloud*> cs;
  std::vector<sga_crop> cr(crops.begin(), crops.end());
  std::vector<int64_t*> kp(clouds.size(), nullptr);
  if (kept) kept->assign(clouds.size(), {});
  for (size_t k = 0; k < clouds.size(); k++) {
    cs.push_back(clouds[k]->h);
    if (kept) {
      (*kept)[k].resize(clouds[k]->size());
      kp[k] = (*kept)[k].empty() ? nullptr : (*kept)[k].data();
    }
  }
  std::vector<sga_cloud*> made(clouds.size(), nullptr);
  check(sga_cloud_crop_batch(ctx, cs.data(), cr.data(), kept ? kp.data() : nullptr, cs.size(), made.data()), "sga_cloud_crop_batch");
  std::vector<PointCloud::Ptr> out;
  for (size_t k = 0; k < made.size(); k++) {
    out.push_back(std::make_shared<PointCloud>(made[k], ctx));
    if (kept) (*kept)[k].resize(out[k]->size());
  }
  return out;
}

/// The problems of create_problems: ordinary sga_problem handles (sga_linearize, sga_align_problem, sga_batch_create, ...), destroyed with the set
struct Problems {
  std::vector<sga_problem*> h;
  Problems() = default;
  Problems(const Problems&) = delete;
  Problems& operator=(const Problems&) = delete;
  Problems(Problems&& o) noexcept : h(std::move(o.h)) { o.h.clear(); }
  ~Problems() {
    for (sga_problem* pb : h) sga_problem_destroy(pb);
  }
  size_t size() const { return h.size(); }
  sga_problem* operator[](size_t k) const { return h[k]; }
};
/// sga_problem_create_batch: the problems of several (target, source cloud, initial guess) triples of one context (Ts empty: identities) by
/// one chain of launches and one host wait; problem k is what sga_problem_create(ctx, targets[k], sources[k], Ts[k]) makes, its source in
/// the same order bit for bit.  targets: the handles of KdTree / GaussianVoxelMap / IncrementalVoxelMap / ProjectiveSearch objects (`h`).
inline Problems create_problems(sga_context* ctx, const std::vector<const sga_index*>& targets, const std::vector<std::shared_ptr<const PointCloud>>& sources, const std::vector<Isometry3d>& Ts = {}) {
  if (targets.size() != sources.size() || (!Ts.empty() && Ts.size() != targets.size())) throw std::runtime_error("create_problems: as many targets as sources (and poses)");
  std::vector<const sga_cloud*> cs;
  std::vector<double> T16;
  for (size_t k = 0; k < sources.size(); k++) {
    cs.push_back(sources[k]->h);
    if (!Ts.empty()) T16.insert(T16.end(), Ts[k].data(), Ts[k].data() + 16);
  }
  Problems out;
  out.h.assign(targets.size(), nullptr);
  check(sga_problem_create_batch(ctx, targets.data(), cs.data(), Ts.empty() ? nullptr : T16.data(), targets.size(), out.h.data()), "sga_problem_create_batch");
  return out;
}

template <typename Reg>
void copy_setting(Reg& reg, const RegistrationSetting& setting) {
  reg.criteria.rotation_eps = setting.rotation_eps;
  reg.criteria.translation_eps = setting.translation_eps;
  reg.optimizer.max_iterations = setting.max_iterations;
  reg.optimizer.verbose = setting.verbose;
}

/// registration_helper.cpp:81-122
inline RegistrationResult align(const PointCloud& target, const PointCloud& source, const KdTree& target_tree, const Isometry3d& init_T = Isometry3d::Identity(), const RegistrationSetting& setting = RegistrationSetting()) {
  const double md2 = setting.max_correspondence_distance * setting.max_correspondence_distance;
  switch (setting.type) {
    case RegistrationSetting::ICP: {
      Registration<ICPFactor, ParallelReductionHIP> reg;
      reg.rejector.max_dist_sq = md2;
      copy_setting(reg, setting);
      return reg.align(target, source, target_tree, init_T);
    }
    case RegistrationSetting::PLANE_ICP: {
      Registration<PointToPlaneICPFactor, ParallelReductionHIP> reg;
      reg.rejector.max_dist_sq = md2;
      copy_setting(reg, setting);
      return reg.align(target, source, target_tree, init_T);
    }
    case RegistrationSetting::GICP: {
      Registration<GICPFactor, ParallelReductionHIP> reg;
      reg.rejector.max_dist_sq = md2;
      copy_setting(reg, setting);
      return reg.align(target, source, target_tree, init_T);
    }
    default:
      std::fprintf(stderr, "error: use align(const GaussianVoxelMap&, const PointCloud&, ...) for VGICP\n");
      return RegistrationResult(Isometry3d::Identity());
  }
}
/// registration_helper.cpp:125-137 (the rejector stays at its 1.0 m^2 default like the reference)
inline RegistrationResult align(const GaussianVoxelMap& target, const PointCloud& source, const Isometry3d& init_T = Isometry3d::Identity(), const RegistrationSetting& setting = RegistrationSetting()) {
  if (setting.type != RegistrationSetting::VGICP) std::fprintf(stderr, "invalid registration type for GaussianVoxelMap\n");
  Registration<GICPFactor, ParallelReductionHIP> reg;
  copy_setting(reg, setting);
  return reg.align(target, source, target, init_T);
}
/// registration_helper.cpp:57-69: raw points in, everything on the GPU
template <typename T, size_t D>
RegistrationResult align(const std::vector<std::array<T, D>>& target, const std::vector<std::array<T, D>>& source, const Isometry3d& init_T = Isometry3d::Identity(), const RegistrationSetting& setting = RegistrationSetting()) {
  auto [target_points, target_tree] = preprocess_points(PointCloud(target), setting.downsampling_resolution, 10, setting.num_threads);
  auto [source_points, source_tree] = preprocess_points(PointCloud(source), setting.downsampling_resolution, 10, setting.num_threads);
  if (setting.type == RegistrationSetting::VGICP) {
    auto voxelmap = create_gaussian_voxelmap(*target_points, setting.voxel_resolution);
    return align(*voxelmap, *source_points, init_T, setting);
  }
  return align(*target_points, *source_points, *target_tree, init_T, setting);
}

// ---- sweep registration: the pose and the twist of a raw sweep at once (sga_align_sweep) -------------------------
/// What align_sweep takes beyond a registration's setting (sga_sweep_params with its defaults): the time the pose refers to, the initial
/// twist ([rx ry rz tx ty tz], the sensor's motion per unit of time) and a Gaussian prior on the twist (information all zero: none).
struct SweepParams {
  double ref_time = 1.0;
  std::array<double, 6> init_twist{};
  std::array<double, 6> twist_prior{};
  std::array<double, 36> twist_information{};  // 6x6 row-major, symmetric
};
/// sga_sweep_result: T_target_source is target <- sensor at ref_time; H (12x12, row-major) and b in the order [pose | twist]
struct SweepResult {
  Isometry3d T_target_source = Isometry3d::Identity();
  std::array<double, 6> twist{};
  bool converged = false;
  size_t iterations = 0;
  size_t num_inliers = 0;
  std::array<double, 144> H{};
  std::array<double, 12> b{};
  double error = 0.0;
};
/// The raw sweep `source` — point i measured at times[i] in the sensor frame of that instant; times.size() == source.size() — registered
/// against `target` through its KdTree, the pose and the twist estimated together.  ICP, PLANE_ICP (target normals) or GICP (covariances
/// on both sides); setting.type VGICP is refused by the library's kd-tree check.
inline SweepResult align_sweep(const PointCloud& target, const PointCloud& source, const std::vector<float>& times, const KdTree& target_tree, const Isometry3d& init_T = Isometry3d::Identity(),
                               const SweepParams& params = SweepParams(), const RegistrationSetting& setting = RegistrationSetting()) {
  (void)target;
  if (times.size() != source.size()) throw std::invalid_argument("align_sweep: one time per point of the sweep");
  check(sga_index_refresh_attributes(source.ctx, target_tree.h, target_tree.points->h), "sga_index_refresh_attributes");
  sga_registration_setting s;
  sga_registration_setting_default(&s);
  s.factor.factor_kind = setting.type == RegistrationSetting::ICP ? SGA_ICP : setting.type == RegistrationSetting::PLANE_ICP ? SGA_PLANE_ICP : SGA_GICP;
  s.factor.max_dist_sq = setting.max_correspondence_distance * setting.max_correspondence_distance;
  s.rotation_eps = setting.rotation_eps;
  s.translation_eps = setting.translation_eps;
  s.max_iterations = setting.max_iterations;
  s.verbose = setting.verbose ? 1 : 0;
  sga_sweep_params p;
  sga_sweep_params_default(&p);
  p.ref_time = params.ref_time;
  std::memcpy(p.twist_prior, params.twist_prior.data(), sizeof(p.twist_prior));
  std::memcpy(p.twist_information, params.twist_information.data(), sizeof(p.twist_information));
  static const float no_time = 0.f;  // (an empty sweep: a pointer that is not NULL; nothing is read)
  sga_sweep_result r;
  check(sga_align_sweep(source.ctx, target_tree.h, source.h, times.empty() ? &no_time : times.data(), init_T.data(), params.init_twist.data(), &s, &p, &r), "sga_align_sweep");
  SweepResult out;
  std::memcpy(out.T_target_source.m.data(), r.T_target_source, sizeof(double) * 16);
  std::memcpy(out.twist.data(), r.twist, sizeof(double) * 6);
  out.converged = r.converged != 0;
  out.iterations = r.iterations;
  out.num_inliers = r.num_inliers;
  std::memcpy(out.H.data(), r.H, sizeof(double) * 144);
  std::memcpy(out.b.data(), r.b, sizeof(double) * 12);
  out.error = r.error;
  return out;
}

}  // namespace small_gicp_amd

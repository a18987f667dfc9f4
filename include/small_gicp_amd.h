/*
 * small_gicp_amd — C-ABI of the MI355X-native registration hot path.
 *
 * Drop-in boundary for koide3/small_gicp's per-iteration linearization (reference tree /root/reference, v1.0.1).
 * Every entry point names the reference interface it replaces (file:line relative to /root/reference).
 * Plain C: opaque handles, caller-owned host buffers, int status codes, no exceptions, no torch types.
 *
 * Conventions
 *   - 4x4 transforms are column-major double[16] (Eigen::Isometry3d::matrix().data()).
 *   - 6x6 H is row-major double[36] (symmetric), b is double[6]; twist order is [rx ry rz tx ty tz] (util/lie.hpp:73-77).
 *   - Symmetric 3x3 matrices ("cov6", "mahalanobis6") are packed xx,xy,xz,yy,yz,zz.
 *   - All device work of a context is serialised on ONE HIP stream; blocking calls synchronise that stream only.
 *   - A context is bound to one GPU; multi-GPU = one process (or context) per GPU with the source cloud sharded: after
 *     sga_comm_init() every sga_linearize all-reduces its 96-double accumulator (system + error-model moments) over the ranks on the
 *     context's stream before the host reads it (the 30-double sga_linearize_async() form is the building block for other transports).
 *   - Diagnostics (search statistics, debug counters) are declared in small_gicp_amd_debug.h; environment switches (SGA_*) read when the
 *     library loads select between equivalent kernels for experiments and are NOT part of this ABI.
 */
#ifndef SMALL_GICP_AMD_H
#define SMALL_GICP_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sga_context sga_context; /* one GPU + one stream */
typedef struct sga_cloud sga_cloud;     /* device-resident point cloud: points [+ normals] [+ covariances]          (points/point_cloud.hpp:15-71) */
typedef struct sga_index sga_index;     /* nearest-neighbour search target: kd-tree (replaces ann/kdtree.hpp KdTree) or GaussianVoxelMap */
typedef struct sga_problem sga_problem; /* a (target index, source cloud) pairing + per-source-point factor state (registration.hpp:41 std::vector<PointFactor>) */

enum sga_status {
  SGA_OK = 0,
  SGA_ERR_INVALID = 1,     /* bad argument */
  SGA_ERR_HIP = 2,         /* a HIP runtime call failed; see sga_last_error() */
  SGA_ERR_NO_DEVICE = 3,   /* no usable gfx950 device: the product path NEVER falls back to the CPU */
  SGA_ERR_UNSUPPORTED = 4, /* combination not available (e.g. PLANE_ICP against a Gaussian voxel map) */
  SGA_ERR_CALLBACK = 5     /* a user callback returned non-zero */
};

/* registration_helper.hpp:38 RegistrationSetting::RegistrationType (VGICP = GICP factor against a GaussianVoxelMap index) */
enum sga_factor_kind { SGA_ICP = 0, SGA_PLANE_ICP = 1, SGA_GICP = 2 };
/* factors/robust_kernel.hpp:11-59 */
enum sga_robust_kind { SGA_ROBUST_NONE = 0, SGA_ROBUST_HUBER = 1, SGA_ROBUST_CAUCHY = 2 };
enum sga_optimizer_kind { SGA_LEVENBERG_MARQUARDT = 0, SGA_GAUSS_NEWTON = 1 };
enum sga_math_mode { SGA_MATH_FP32 = 0, SGA_MATH_FP64 = 1 }; /* per-pair arithmetic; data in HBM is fp32 either way, sums are fp64 */

/* Thread-local description of the last failure on the calling thread. Never NULL. */
const char* sga_last_error(void);
/* Library version string. */
const char* sga_version(void);
/* Diagnostics of the library's caching device allocator: hipMalloc calls, allocations served by the calling stream's own free list, by
 * the shared pool, by blocks whose deferred release had completed, and frees that had to be deferred behind busy streams. */
void sga_allocator_stats(uint64_t out[5]);
/* Number of visible HIP devices (0 when there is no GPU / no driver). */
int sga_device_count(void);

/* ---- context -------------------------------------------------------------------------------------------------- */
int sga_context_create(int device, sga_context** out);
/* Borrow an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) instead of creating one. */
int sga_context_create_on_stream(int device, void* hip_stream, sga_context** out);
int sga_context_destroy(sga_context* ctx);
int sga_context_synchronize(sga_context* ctx);
void* sga_context_stream(sga_context* ctx); /* the hipStream_t */

/* ---- clouds (points/traits.hpp:15-78 accessor protocol: size / point / normal / cov) --------------------------------- */
/* Pinned host memory for the caller's scans (round 6).  The reference's drivers hold every scan in host memory before they time a frame
 * (benchmark/benchmark_odom.hpp:36-47, odometry_benchmark.cpp: the points are read into std::vector<Eigen::Vector4f> first); a caller of
 * this library that reads its scans into memory from sga_host_alloc (or any hipHostMalloc / hipHostRegister'd buffer) spares the upload
 * its only CPU pass: sga_cloud_create_f32 recognises such arrays and lets the device read them in place.  Ordinary (pageable) arrays
 * work as before: they are copied once into the context's pinned staging ring. */
int sga_host_alloc(size_t bytes, void** out);
int sga_host_free(void* p);
/* fp32 input: xyz n*3, normals n*3 or NULL, cov6 n*6 or NULL.  The arrays are free for reuse when the call returns (in stream-ordered
 * mode too: a pageable array has been copied, a pinned one has been read). */
int sga_cloud_create_f32(sga_context* ctx, const float* xyz, const float* normals, const float* cov6, size_t n, sga_cloud** out);
/* Reference PointCloud layout (points/point_cloud.hpp:69-71): xyzw n*4 doubles, normals n*4 doubles or NULL, covs n*16 doubles (4x4) or NULL */
int sga_cloud_create_f64(sga_context* ctx, const double* xyzw, const double* normals4, const double* cov4x4, size_t n, sga_cloud** out);
/* Device frames (round 5).  The reference stores and computes in double (points/point_cloud.hpp:69-71), so clouds kilometres from the origin
 * (UTM / ENU maps) register to full precision; the device keeps fp32.  Every cloud therefore has an ORIGIN (double[3]) and the device
 * holds fl32(p - origin), the subtraction done in double: sga_cloud_create_f32 / _f64 choose it themselves (the centre of the bounding
 * box rounded to a multiple of 128 m — so a cloud centred within 64 m of the origin keeps origin 0 and is stored as before); poses,
 * H, b, downloaded points, voxel coordinates and kNN queries are always the CALLER's frame, the library converts at its entry points
 * (pose: t' = R o_source + t - o_target in double; H, b: the 6x6 adjoint of the source shift, so that the twist convention of
 * util/lie.hpp:73-96 and the LM damping of optimizer.hpp:100-144 are the reference's).  The _origin forms let the caller name the origin:
 *   sga_cloud_create_f32_origin: xyz_rel are ALREADY relative to origin (true position = xyz_rel + origin; origin NULL = 0) — how an
 *     fp32 caller hands over a geo-referenced cloud without losing its millimetres;
 *   sga_cloud_create_f64_origin: absolute doubles, recentred about `origin` (NULL: chosen as above) — ranks that upload their own shard of
 *     a sharded source name a common origin (the shards' accumulators are added; slices made with sga_cloud_slice share one anyway). */
int sga_cloud_create_f32_origin(sga_context* ctx, const float* xyz_rel, const float* normals, const float* cov6, size_t n, const double origin[3], sga_cloud** out);
int sga_cloud_create_f64_origin(sga_context* ctx, const double* xyzw, const double* normals4, const double* cov4x4, size_t n, const double origin[3], sga_cloud** out);
int sga_cloud_origin(const sga_cloud* cloud, double origin[3]);
int sga_index_origin(const sga_index* index, double origin[3]);
/* the library's rule: origin of the device frame for a bounding box (empty / non-finite box: 0) */
void sga_choose_origin(const double lo[3], const double hi[3], double origin[3]);
/* A new cloud holding points [first, first + count) of `cloud` with their normals / covariances (device copy): the source shard of one
 * rank when a registration is spread over GPUs (reduction_omp.hpp:32-58 is the loop being partitioned). */
int sga_cloud_slice(sga_context* ctx, const sga_cloud* cloud, size_t first, size_t count, sga_cloud** out);
/* Posed clouds joined into one cloud — the last K keyframes at their estimated poses as one target — without leaving the device.  In the
 * reference this is a host loop over points, normals and covs (src/test/registration_test.cpp:84: pt = T * pt per point); here one table
 * and ONE launch whatever count is.  *out holds the points of clouds[0], then clouds[1], ... each in its own order, the index word of a
 * point its position in *out.  T: count poses, column-major 4x4 (NULL: identities).  R_m is the upper-left 3x3 of T_m taken as it is
 * (the reference's T * p: nothing is renormalised); with o_m the member's origin, c_m = R_m o_m + t_m — per row
 * ((R0 o0 + R1 o1) + R2 o2) + t, every operation rounded on its own — and o the output's origin, a record r of member m becomes
 *   fl32(R_m r + (c_m - o)),
 * c_m - o formed once per member on the host, the rest evaluated in double on the device and rounded once: a submap kilometres from the
 * origin keeps its millimetres.  Normals become fl32(R_m n), covariances the six entries of fl32(R_m C R_m^T), both evaluated in double
 * from the fp32 records.  ATTRIBUTES: the output has normals only if every non-empty member has them, and covariances only if every
 * non-empty member has them; otherwise the attribute is dropped (sga_cloud_has tells).  A non-finite point stays non-finite and takes no
 * part in the bounding box.
 *   origin given: o is that; a stream-ordered context waits for nothing and its cloud carries no bounding box (sga_cloud_create_device's
 *     contract), a blocking context keeps the box of the records with the cloud.
 *   origin NULL: o = sga_choose_origin of the bounding box of the finite posed points R_m r + c_m, reduced on the device in double (the
 *     one host wait the data forces).  The records are first written for the origin zero — their box is that box —; when the rule chooses
 *     another origin a second launch writes them again FROM THE MEMBERS' RECORDS: the result never depends on the route.
 * A cloud may appear several times under different poses; members made by another context of the same device are waited for; empty
 * members take no part.  count == 0, or empty members only: an empty cloud without attributes at the given origin (or zero), no device
 * work.  Refusals (SGA_ERR_INVALID, before any device work, *out = NULL as on every failure): NULL ctx, clouds or out; a NULL member, a
 * non-finite entry of a pose (both named by number) or of origin; more than 2^15 members; a member on another device; 2^31 points or
 * more in all.  sga_cloud_transform is the merge of one member. */
int sga_cloud_merge(sga_context* ctx, const sga_cloud* const* clouds, const double* T /* count x 16 column-major, or NULL: identities */, size_t count, const double origin[3] /* or NULL */, sga_cloud** out);
int sga_cloud_transform(sga_context* ctx, const sga_cloud* cloud, const double T[16], const double origin[3], sga_cloud** out);
/* Raw sweeps deskewed on the device: per-point motion compensation ahead of the voxel grid.  A spinning LiDAR
 * measures every point from the pose the sensor has at that instant; with the sensor pose T0 exp(s xi) at time s (xi: the motion per unit
 * of time, sga_se3_exp's convention, rotation first), a point P measured at s_i in the sensor frame of that instant is, in the sensor
 * frame at ref_time,
 *   P' = exp(a_i xi) P,   a_i = double(s_i) - ref_time   (a_i xi componentwise).
 * times[k][i] is the time of point i of clouds[k] in the cloud's storage order (the caller's order; the unit is the caller's, normally 0 =
 * the sweep's start and 1 = its end).  With o the cloud's origin and r a record (P = r + o), (R_i, t_i) = exp(a_i xi) evaluated in double
 * WITHOUT cancellation for every angle (sin, 2 sin^2(phi/2) and a series for phi - sin phi; csrc/lie.hpp) — a_i runs through 0 —, the
 * output record is fl32(R_i r + (R_i o + t_i - o)) ((R_i - I) o formed from its own terms), normals become fl32(R_i n) and covariances
 * the six entries of fl32(R_i C R_i^T): evaluated in double from the fp32 records and rounded once, as in sga_cloud_merge.  out[k] keeps
 * clouds[k]'s origin and attributes; the index word of a point is its position.  xi = 0, or s_i == ref_time, reproduces the record
 * exactly.  A non-finite time gives a non-finite point, which takes no part in the bounding box; nothing on the host reads the times.
 * One table copy and ONE launch whatever count is.  A blocking context keeps the box of the records with every out[k] (its one wait);
 * a stream-ordered context waits for nothing and its clouds carry no box.  An empty member yields an empty cloud without attributes;
 * count == 0 is SGA_OK without device work.  Refusals (SGA_ERR_INVALID, every out[k] = NULL as on every failure) — before any handle is
 * read: NULL arguments (clouds[k] / times[k] named by number), a non-finite twist entry or reference time (named by number), more than
 * 2^15 members; then: a cloud of another device, times in device memory (they go through sga_cloud_deskew_device).
 * sga_cloud_deskew is the batch of one.  sga_cloud_deskew_device takes the times from device memory of the context's device (float or
 * double, cols = 1, any stride >= 1: a column of a wider array), checked against its allocation, and orders user_stream as
 * sga_cloud_create_device does (flags: SGA_IO_NO_ORDER); host memory is refused (it goes through sga_cloud_deskew). */
int sga_cloud_deskew_batch(sga_context* ctx, const sga_cloud* const* clouds, const float* const* times, const double* twists /* count x 6 */, const double* ref_times /* count, or NULL: 1.0 each */,
                           size_t count, sga_cloud** out /* count */);
int sga_cloud_deskew(sga_context* ctx, const sga_cloud* cloud, const float* times, const double twist[6], double ref_time, sga_cloud** out);
/* Clouds cropped on the device: the returns nobody wants — the ego vehicle, near-field clutter, far noise, non-finite returns, what lies
 * outside a radius of a submap — dropped ahead of the deskew and the voxel grid, the survivors compacted in their order (DESIGN.md
 * section 3.20).  ONE predicate, evaluated in double from the fp32 record r and the cloud's origin o:
 *   range:  x_a = double(r_a) + (o_a - center_a) (the bracket formed once on the host), d2 = x . x; keep iff
 *           min_range^2 <= d2 && d2 <= max_range^2 (the squares formed on the host; no square root is taken);
 *   box:    y_a = double(r_a) + o_a, inside iff box_lo_a <= y_a && y_a <= box_hi_a on all three axes; box_mode 1 keeps the points inside,
 *           2 the finite points NOT inside (an ego-vehicle box: points on the closed boundary are dropped), 0 makes no box test;
 *   a record with a non-finite coordinate is dropped in every mode: the default crop (sga_crop_default: center 0, ranges 0 and +inf, no
 *   box) is "remove the non-finite points".
 * A point is kept when it passes the range test and the box test.  out[k] keeps clouds[k]'s origin; its record j is input record
 * kept[j] bit for bit in x, y, z, normal and covariance, its index word is j, kept[] ascending (the compaction is stable); out[k] carries the bounding
 * box of its records.  kept[k] (optional, room for clouds[k]'s size): the indices kept, the first size-of-out[k] entries written —
 * what a caller needs to keep its times, intensities, rings or labels aligned.  A member of which nothing is kept, and an empty
 * member, yield an empty cloud without attributes.  One table copy and ONE launch whatever count is, and one host wait — on a
 * stream-ordered context too: the sizes have to reach the host.  The arrays of out[k] have room for clouds[k]'s size.
 * count == 0 is SGA_OK before anything is looked at.  Refusals (SGA_ERR_INVALID, every out[k] = NULL as on every failure) — before any
 * handle is read: NULL arguments (clouds[k] named by number); more than 2^15 members; of crops[k], named by number: min_range negative or
 * NaN, max_range NaN, min_range > max_range, a non-finite center, box_mode outside 0..2, and with box_mode != 0 a NaN bound or
 * box_lo > box_hi (infinite bounds are fine) — then: a cloud of another device, 2^31 tiles of 2048 points or more in all.
 * sga_cloud_crop is the batch of one. */
typedef struct sga_crop {
  double center[3];            /* caller's frame; ranges are measured from here */
  double min_range, max_range; /* keep min_range^2 <= d2 <= max_range^2 */
  double box_lo[3], box_hi[3]; /* caller's frame, closed interval per axis */
  int box_mode;                /* 0: no box test, 1: keep inside, 2: keep outside */
  int pad;
} sga_crop;
void sga_crop_default(sga_crop* crop);
int sga_cloud_crop_batch(sga_context* ctx, const sga_cloud* const* clouds, const sga_crop* crops /* count */, int64_t* const* kept /* count, or NULL; entries may be NULL */, size_t count,
                         sga_cloud** out /* count */);
int sga_cloud_crop(sga_context* ctx, const sga_cloud* cloud, const sga_crop* crop, int64_t* kept /* or NULL */, sga_cloud** out);
/* A new cloud whose record j is record indices[j] of `cloud` — points, normals and covariances bit for bit, the index word j, the origin
 * kept — by ONE launch: a gather (the reference's random_sampling, util/downsampling.hpp, is the host's choice of indices followed by
 * this).  Repeats are allowed and the order is as given; m == 0 yields an empty cloud without attributes.  The indices are checked on
 * the host — an index outside [0, size) is SGA_ERR_INVALID and named by its position — and reach the device through the staging ring. */
int sga_cloud_select(sga_context* ctx, const sga_cloud* cloud, const int64_t* indices, size_t m, sga_cloud** out);
/* Outliers removed on the device: isolated returns — rain, dust, multipath, mixed pixels at depth edges — dropped from a cloud by the
 * distances to its own nearest neighbours, the survivors compacted in their order.  For a cloud of n points,
 * the point itself counts as its own nearest record at distance 0: s_i(j) is the j-th smallest Euclidean distance from point i to the
 * records of the cloud, s_i(0) = 0 — the filters depend on multisets of distances only, never on how ties are broken.
 *   mode 0, statistical (k, std_mul): d_i = (s_i(0) + ... + s_i(k')) / k' with k' = min(k, n - 1) (n = 1: d_0 = 0); mean = sum d_i / n;
 *           stddev = sqrt(sum (d_i - mean)^2 / (n - 1)), 0 for n < 2; threshold = mean + std_mul * stddev; keep iff d_i <= threshold.
 *   mode 1, radius (k = the least number of neighbours, radius): keep iff point i has at least k other records within radius, i.e. iff
 *           s_i(k) <= radius; d_i = s_i(k), +inf when n <= k (such a point is removed).
 * Distances are the fp32 squared distances of the kd search, square-rooted and summed in double; mean, stddev and threshold are formed
 * in double on the device in an order that depends on nothing but n (no floating-point atomics): two calls on the same cloud give the
 * same bits.  kdtree: a kd-tree over THIS cloud — checked as sga_estimate_normals_covariances checks it: kind, size, the origin of the
 * device frame — or NULL: a temporary one is built.  *out is what sga_cloud_crop hands back: an ordinary cloud that keeps the input's
 * order, origin, normals and covariances bit for bit, its index word the new position, its box the box of its own records; nothing
 * kept, or an empty input, yields an empty cloud without attributes (and zeroed stats for an empty input).  kept (or NULL; room for n):
 * the indices kept, ascending, the first size-of-*out entries written.  stat (or NULL; room for n): d_i in the cloud's order.  stats
 * (or NULL): mean, stddev and threshold of the d_i (radius mode: threshold = radius; mean and stddev are those of the s_i(k)) and the
 * number kept.  With a caller's tree the call enqueues at most four commands whatever n is — the statistic, the threshold, the
 * compaction's table copy, the compaction — and waits once, for the count and the box, on a stream-ordered context too.
 * A cloud with a non-finite coordinate has no kd-tree (the build refuses it: "contains non-finite coordinates", which a temporary build
 * reports from here): crop first, sga_cloud_crop's default removes such points.  Refusals (SGA_ERR_INVALID, *out = NULL as on every
 * failure) — before any handle is read: NULL ctx, cloud, filter or out; mode other than 0 or 1; k outside [1, 63] (the point and its k
 * neighbours fill the 64 lanes of a wave); in mode 0 a std_mul that is not finite and >= 0; in mode 1 a radius that is not finite and
 * > 0 — then: a cloud of another device, a tree of another kind, size or device frame, 2^31 points or more. */
typedef struct sga_outlier_filter {
  int mode; /* 0 statistical, 1 radius */
  int k;    /* neighbours: averaged over (mode 0), required within radius (mode 1) */
  double std_mul;
  double radius;
} sga_outlier_filter;
typedef struct sga_outlier_stats {
  double mean, stddev, threshold; /* radius mode: threshold = radius, mean / stddev still reported */
  size_t kept;
} sga_outlier_stats;
void sga_outlier_filter_default(sga_outlier_filter* filter); /* statistical, k = 10, std_mul = 1.0 */
int sga_cloud_remove_outliers(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree /* over this cloud, or NULL: a temporary one */, const sga_outlier_filter* filter, int64_t* kept /* n, or NULL */,
                              double* stat /* n: d_i in the cloud's order, or NULL */, sga_outlier_stats* stats /* or NULL */, sga_cloud** out);
/* A posed cloud compared with a target on the device: how much of a scan the map already explains, and which points are new (DESIGN.md
 * section 3.22) — the keyframe decision of a mapping loop, the fitness and inlier RMSE of a loop-closure candidate, "add only what the
 * map does not hold yet", change detection.  For point i of `cloud` (fp32 record r_i in the device frame at origin o_c) and a target
 * whose device frame is at o_t:  q_i = R r_i + (c - o_t) in double, c = R o_c + t (per row ((R0 o0 + R1 o1) + R2 o2) + t); T
 * (column-major 4x4, maps the cloud into the target; NULL: the identity) gives R and t.
 *   kd-tree target:   the exact nearest record of float(q_i) by the registration's 1-NN walk, searched within max_distance widened by
 *                     |q_i - float(q_i)|; d_i is that record's distance measured again in double from q_i.
 *   Gaussian map (one-shot or incremental) / flat map: the lookup of the registration over the map's own search offsets (1 / 7 / 27),
 *                     the first of equal distances winning; d_i is the distance to the voxel's mean / to the stored point.
 * Point i is MATCHED iff it has a winner and d_i <= max_distance.  It is unmatched when it has none, when the winner is farther, or
 * when a coordinate of q_i is not finite; an unmatched point reports d_i = +inf and nearest -1.  An empty target (no points, no voxels)
 * leaves every point unmatched.
 * dist (or NULL; room for n): d_i in the cloud's order.  nearest (or NULL; room for n): the winner — the target point's ORIGINAL index
 * (kd-tree), the voxel id (Gaussian map), voxel * 16 + slot (flat map: its position in sga_flatmap_download's arrays).  stats (or NULL):
 * points = n, matched, fitness = matched / points (0 for an empty cloud), rmse = sqrt(sum d_i^2 / matched) and mean_distance over the
 * matched (0 when there are none) — the sums formed in double on the device in an order that depends on nothing but n (no
 * floating-point atomics): two calls give the same bits.
 * params->keep: 0 — statistics only, out must be NULL; 1 / 2 — *out receives the matched / the unmatched points as an ordinary cloud, by
 * the compaction of sga_cloud_crop: the input's order, origin, normals and covariances, record j of *out equal to input record kept[j] bit
 * for bit, its index word j, its box the box of its own records; nothing kept, or an empty input, yields an empty cloud without
 * attributes.  As in the crop the compaction keeps finite records only: a point with a non-finite coordinate counts in `points`, never in
 * `matched`, and is in no output cloud, the unmatched one included.  kept (or NULL; room for n; only with keep != 0): the indices kept,
 * ascending, the first size-of-*out entries written.
 * Commands: a statistics-only call enqueues TWO — the distances, the sums — and waits once for the second; with an output cloud the
 * compaction's table copy and launch follow (four in all) and the one wait is the compaction's, on a stream-ordered context too.  An
 * empty cloud enqueues nothing and gives zero stats.  The cloud and the target may have been made on other contexts of the device that
 * returned before their kernels had run: the call orders itself behind both.
 * Refusals (SGA_ERR_INVALID, *out = NULL as on every failure) — before any handle is read: NULL ctx, cloud, target or params; keep
 * outside 0..2; out given with keep == 0, or missing with keep != 0; kept given with keep == 0; max_distance NaN or <= 0 (+inf is
 * allowed); a non-finite entry of T — then: a cloud or a target of another device, a projective target (SGA_ERR_UNSUPPORTED), 2^31
 * points or more. */
typedef struct sga_overlap {
  double max_distance;
  int keep; /* 0 none, 1 the matched, 2 the unmatched */
  int reserved;
} sga_overlap;
typedef struct sga_overlap_stats {
  size_t points, matched;
  double fitness; /* matched / points, 0 for an empty cloud */
  double rmse;    /* over the matched, 0 if none */
  double mean_distance;
} sga_overlap_stats;
void sga_overlap_default(sga_overlap* p); /* max_distance 1.0, keep 0 */
int sga_cloud_overlap(sga_context* ctx, const sga_cloud* cloud, const sga_index* target, const double T[16] /* or NULL */, const sga_overlap* params, double* dist /* n, or NULL */, int64_t* nearest /* n, or NULL */,
                      int64_t* kept /* n, or NULL */, sga_overlap_stats* stats /* or NULL */, sga_cloud** out /* NULL iff keep == 0 */);
/* The free-space check of a mapping loop: which points of `map` does the posed `scan` see THROUGH — the ghost
 * trails that moving objects leave in a submap — by a range image of the scan, on the device.
 * Sensor frame: x forward, y left, z up (what a spinning lidar and KITTI deliver; NOT the camera convention of the projective search).
 * Projection of a point s, every operation rounded, no product fused into a sum:  rho = sqrt((sx^2 + sy^2) + sz^2), az = atan2(sy, sx),
 * el = asin(sz / rho), su = (az / (2 pi) + 0.5) * width, u = (int)su with u == width becoming 0 (azimuth +pi is the direction of -pi),
 * sv = (fov_up - el) / (fov_up - fov_down) * height, v = floor(sv).  s is IN THE IMAGE iff rho > 0, everything is finite, 0 <= sv and
 * v < height.
 * Range image of `scan` (point = fp32 record + the cloud's origin, in double): a cell holds the least rho over the scan's returns that are
 * finite, in the image and have rho >= min_range; an empty cell holds +inf.  Returns nearer than min_range are the ego vehicle: they
 * would shadow everything behind them, and are left out.  max_range does not bound the scan's returns.
 * Map point i (fp32 record r in the map's device frame at origin o_m), T (column-major 4x4, NULL: the identity) the pose registration
 * returns — it maps the scan's sensor frame into the map's frame, T = [R t]:  w_k = (double)r_k + (o_m[k] - t[k]), the difference formed
 * once on the host;  s = R^T w, per component ((R[0][k] w0 + R[1][k] w1) + R[2][k] w2);  rho_i = |s| as above.
 * Window of (u, v): du in -window_h .. window_h, wrapping in azimuth; dv in -window_v .. window_v, rows outside the image skipped.  m_i
 * and M_i are the least and the greatest finite cell of the window.  With tol_i = margin + margin_ratio * rho_i:
 *   state 0  unobserved    s not finite, not in the image, rho_i < min_range, rho_i > max_range, or no return in the window
 *   state 3  seen through  rho_i + tol_i < m_i: every return of the window lies behind the point
 *   state 2  occluded      rho_i - tol_i > M_i: the point lies behind every return
 *   state 1  consistent    everything else
 * Clearance c_i = m_i - rho_i for the states 1 .. 3, NaN for state 0.  The rule reads only the multiset of ranges in a window: it depends
 * on no order, and two calls give the same bytes.
 * state / clearance (or NULL; room for n): per map point, the map's order.  range_image (or NULL; room for width * height): cell (u, v)
 * at [v * width + u].  stats (or NULL): points = n and the four counts.  params->keep: 0 — no cloud, out must be NULL; 1 — *out
 * receives the seen-through points; 2 — all the others (the cleaned map) — as an ordinary cloud, by the compaction of sga_cloud_crop:
 * the map's order, origin, normals and covariances, record j of *out equal to map record kept[j] bit for bit, finite records only;
 * nothing kept, or an empty map, yields an empty cloud without attributes.  A non-finite map record counts in `points` and in
 * `unobserved` and is in no output cloud.  kept (or NULL; room for n; only with keep != 0): the indices kept, ascending, the first
 * size-of-*out entries written.
 * Commands: a statistics-only call enqueues FOUR — the fill that clears the image, the image, the states, the counts — THREE when the
 * scan is empty (no image kernel: every point is unobserved), and waits once for the last; with an output cloud the compaction's table
 * copy and launch follow (six / five in all) and the one wait is the compaction's.  An empty map enqueues nothing and gives zero stats
 * and an empty cloud — unless range_image is asked for: then the image alone is built and handed back (the fill, the image, the export:
 * three, two for an empty scan).  Both clouds may have been made on other contexts of the device that returned before their kernels
 * had run: the call orders itself behind both.
 * Refusals (SGA_ERR_INVALID, *out = NULL as on every failure, nothing enqueued) — before any handle is read: NULL ctx, map, scan or
 * params; width or height below 1 or width * height above 2^24; fov_up or fov_down not finite, outside [-pi/2, pi/2], or fov_up <=
 * fov_down; min_range not finite or < 0; max_range NaN or < min_range (+inf is allowed); margin or margin_ratio not finite or < 0;
 * window_h or window_v outside [0, 16]; keep outside 0..2; out given with keep == 0, or missing with keep != 0; kept given with keep ==
 * 0; a non-finite entry of T — then: a cloud of another device, 2^31 points or more in either cloud. */
typedef struct sga_visibility {
  int width, height;
  double fov_up, fov_down;     /* radians */
  double min_range, max_range; /* max_range may be +inf */
  double margin, margin_ratio;
  int window_h, window_v;
  int keep; /* 0 none, 1 the seen-through, 2 all the others (the cleaned map) */
  int reserved;
} sga_visibility; /* 72 bytes */
typedef struct sga_visibility_stats {
  size_t points, unobserved, consistent, occluded, seen_through;
} sga_visibility_stats; /* 40 bytes */
void sga_visibility_default(sga_visibility* p); /* 1024 x 64, +3 / -25 degrees in radians, 0.5 / 60.0, 0.2 / 0.01, 1 / 1, keep 0 */
int sga_cloud_visibility(sga_context* ctx, const sga_cloud* map, const sga_cloud* scan, const double T[16] /* or NULL */, const sga_visibility* params, uint8_t* state /* n, or NULL */, double* clearance /* n, or NULL */,
                         double* range_image /* width * height, [v * width + u], or NULL */, int64_t* kept /* n, or NULL; only with keep != 0 */, sga_visibility_stats* stats /* or NULL */, sga_cloud** out /* NULL iff keep == 0 */);
/* Global registration on the device: a pose from geometry alone — FPFH descriptors, nearest rows in feature
 * space, RANSAC over the correspondences — for the initial guess every local registration needs.  Three calls, usable one by one.
 * Everything is computed in double from the fp32 records, with integer atomics and fixed-order sums only: two calls give the same bytes.
 *
 * sga_features: n rows of dim floats on the device (1 <= dim <= 128).  sga_features_create uploads a caller's rows (row-major, n * dim;
 * n == 0: an empty handle, rows may be NULL); sga_features_download writes n * dim floats.
 *
 * sga_cloud_fpfh: one 33-bin Fast Point Feature Histogram per point of a cloud WITH normals.  Neighbours of point i: its k' = min(k, n - 1)
 * nearest other records of the exact k-NN of the cloud's kd-tree, in the search's order.  viewpoint (caller's frame; NULL: normals as
 * stored): a normal is negated where n . (viewpoint - p) < 0 (nothing is written back).  Pair feature of (i, j), PCL's computePairFeatures:
 * d = p_j - p_i, l = |d| (l == 0: pair skipped); a1 = n_i . d / l, a2 = n_j . d / l; if |a1| < |a2| the roles swap (n1 = n_j, n2 = n_i,
 * d <- -d, phi = -a2), else n1 = n_i, n2 = n_j, phi = a1; v = (d / l) x n1 (|v| == 0: pair skipped), normalised; w = n1 x v; alpha = v . n2;
 * theta = atan2(w . n2, n1 . n2).  Bins, each clamped to 0 .. 10: floor(11 (theta + pi) / (2 pi)), floor(11 (alpha + 1) / 2), floor(11 (phi
 * + 1) / 2).  SPFH_i: the three 11-bin count histograms (theta, alpha, phi) over the pairs not skipped, scaled by 100 / (pairs counted);
 * zero where nothing was counted.  FPFH_i = SPFH_i + (1 / k') sum_j w_ij SPFH_j, w_ij = 1 / |p_j - p_i|^2 (0 for coincident points), the
 * sum in the list's order; each of the three sub-histograms is then rescaled to sum 100 (one that sums to 0 stays 0) and the result is
 * rounded once to fp32.  n == 0: an empty handle, nothing launched; n == 1: one zero row (one fill).  kdtree: over THIS cloud, checked as
 * sga_cloud_remove_outliers checks it, or NULL: a temporary one (a cloud with a non-finite coordinate has no kd-tree and is refused).
 * Three launches, no host wait (a blocking context waits once for the last).
 * Refusals (SGA_ERR_INVALID, *out = NULL) — before any handle is read: NULL ctx, cloud or out; k outside [2, 63]; a non-finite
 * viewpoint — then: a cloud of another device or without normals, a tree of another kind, size or device frame, 2^31 / 33 points or more.
 *
 * sga_features_match: for every row of `source` the row of `target` (same dim) of least squared L2 distance, formed in double from the
 * fp32 values, bins 0 .. dim - 1 summed in order; ties go to the lowest index.  mutual != 0: match[i] = j is kept only when the nearest
 * source row of j is i, otherwise -1.  match (n): the winner or -1; dist (n, or NULL): the square root of the winning distance, +inf for
 * -1; matched (or NULL): the number of entries that are not -1.  Two launches (three with mutual), one host wait; an empty source or
 * target gives all -1 with nothing launched.  Refusals: NULL ctx, source, target or match; mutual other than 0 or 1 — then: another
 * device, different dims, 2^31 rows or more.
 *
 * sga_ransac_correspondences: the rigid motion T (column-major 4x4, source -> target, caller's frames) that most of M index pairs
 * (pairs[2 m] into source, pairs[2 m + 1] into target) agree on.  Points are record + origin in double.  Hypothesis h in [0, iterations)
 * draws three distinct pairs with a counter-based generator: mix64(x): z = x + 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  u_j = mix64(seed ^ mix64(4 h + j)), j = 0, 1, 2; idx(u, R) = ((u >> 32) * R) >> 32;
 * i0 = idx(u0, M); i1 = idx(u1, M - 1), incremented if >= i0; i2 = idx(u2, M - 2), incremented if >= min(i0, i1), then again if >=
 * max(i0, i1).  Edge test: for each of the three edges with lengths ls, lt the hypothesis is dropped unless min(ls, lt) >=
 * edge_similarity * max(ls, lt) and min(ls, lt) >= min_edge.  Pose from triangle frames (a, b, c the triple's points): e1 = (b - a) /
 * |b - a|, e3 = e1 x (c - a) normalised — dropped when |b - a| is 0 or |e1 x (c - a)| < 1e-9 |c - a| or is 0, in either cloud —, e2 = e3 x
 * e1, F = [e1 e2 e3]; R = F_t F_s^T, t = centroid_t - R centroid_s.  Score: the number of the M pairs with |R p_s + t - p_t| <=
 * max_distance.  Best: the greatest score, ties to the lowest h (one 64-bit integer atomic max: no arrival order enters).  Refit: over the
 * best hypothesis' inliers the least-squares rotation (Horn's quaternion form, a Jacobi eigen-solver on the host) from fixed-order sums
 * formed on the device; the hypothesis pose is kept (refit = 0) when fewer than 3 inliers remain or the cross-covariance has rank < 2.
 * result: inliers and inlier_rmse are those of the best hypothesis.  M < 3, or no hypothesis passed the tests: SGA_OK, inliers = 0, T =
 * identity.  Four commands (the pairs' points, the fill of the best word, the hypotheses, the refit sums), one host wait.
 * Refusals — before any handle is read: NULL ctx, source, target, params, T or result, pairs NULL with M > 0; max_distance not finite
 * or <= 0; iterations outside [1, 2^32); edge_similarity outside [0, 1]; min_edge not finite or < 0; M >= 2^31 — then: another device,
 * an index outside either cloud (named by its position), before anything is enqueued. */
typedef struct sga_features sga_features;
int sga_features_create(sga_context* ctx, const float* rows, size_t n, int dim, sga_features** out);
int sga_features_size(const sga_features* features, size_t* n, int* dim);
int sga_features_download(sga_context* ctx, const sga_features* features, float* rows);
int sga_features_destroy(sga_features* features);
/* sga_features_create / sga_features_download with the rows in device memory of the caller's ("device-resident data" below: the struct,
 * the ordering of user_stream, the pointer checks): float or double rows of cols = dim (1..128) values, any stride >= cols; a double
 * is rounded to fp32 once on the way in and a float widened on the way out.  One launch, none for n == 0. */
struct sga_device_array;
int sga_features_create_device(sga_context* ctx, const struct sga_device_array* rows, size_t n, void* user_stream, int flags, sga_features** out);
int sga_features_export_device(sga_context* ctx, const sga_features* features, const struct sga_device_array* rows, void* user_stream, int flags);
/* Row j of *out is row indices[j] of `features`: one gather launch, no host wait; repeats are allowed; m == 0:
 * an empty handle of the same dim, nothing launched.  Refusals (SGA_ERR_INVALID, *out = NULL): NULL ctx, features or out, indices NULL with
 * m > 0, m >= 2^31 — then: another device, an index outside the rows (named by its position), before anything is enqueued. */
int sga_features_select(sga_context* ctx, const sga_features* features, const int64_t* indices, size_t m, sga_features** out);
#define SGA_FPFH_DIM 33
int sga_cloud_fpfh(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree /* over this cloud, or NULL: a temporary one */, int k, const double viewpoint[3] /* or NULL */, sga_features** out);
int sga_features_match(sga_context* ctx, const sga_features* source, const sga_features* target, int mutual, int64_t* match /* n */, double* dist /* n, or NULL */, size_t* matched /* or NULL */);
typedef struct sga_ransac {
  double max_distance;     /* inlier bound, metres */
  uint64_t iterations;     /* hypotheses, 1 .. 2^32 - 1 */
  uint64_t seed;
  double edge_similarity;  /* 0: off */
  double min_edge;
} sga_ransac; /* 40 bytes */
typedef struct sga_ransac_result {
  uint64_t inliers;
  double inlier_rmse;
  uint64_t best_hypothesis;
  uint64_t scored; /* hypotheses that passed the edge and degeneracy tests */
  int refit;       /* 1: T is the least-squares fit over the inliers, 0: the hypothesis pose (or the identity) */
  int reserved;
} sga_ransac_result; /* 40 bytes */
void sga_ransac_default(sga_ransac* p); /* 1.0, 20000, 0, 0.9, 0.0 */
int sga_ransac_correspondences(sga_context* ctx, const sga_cloud* source, const sga_cloud* target, const int64_t* pairs /* M x 2 */, size_t M, const sga_ransac* params, double T[16], sga_ransac_result* result);

/* ---- place recognition: Scan Context (Kim & Kim, IROS 2018) and an exhaustive shift-aligned search ------------
 * "Which of my earlier keyframes is this place, and how am I turned against it?"  A database keeps one descriptor per keyframe on the
 * device; a query compares a scan with every candidate at every column shift.  All arithmetic is double from the fp32 records, with
 * integer atomics and fixed-order sums only: two calls give the same bytes.  tests/place_ref.py restates the rule in numpy.
 *
 * Descriptor of a cloud under the parameters rings R, sectors S, max_range L, height and under center (the sensor's position in the cloud's
 * own coordinates, caller's frame; NULL: zeros): a row-major R x S fp32 image D.  For each record, p = (record + origin) - center in
 * double; a record with a non-finite component is skipped; rho = sqrt(px^2 + py^2), skipped if rho >= L; ring = min(floor(rho / L * R),
 * R - 1); theta = atan2(py, px), plus 2 pi when negative (atan2(0, 0) = 0); sector = min(floor(theta / (2 pi) * S), S - 1); v =
 * float32(max(pz + height, 0)); D[ring][sector] is the greatest v of its cell, 0 for an empty cell.
 *
 * Distance of a query image q to an entry c at shift s in [0, S): n_q[j] = sqrt(sum_r q[r][j]^2), rings ascending, likewise n_c; the
 * column pair (j, (j + s) mod S) counts when both norms are > 0; d(s) = 1 - (1 / count) sum_j (sum_r q[r][j] c[r][(j + s) mod S]) /
 * (n_q[j] n_c[(j + s) mod S]) over the counting pairs, in double; count == 0: d(s) = 1.  d = min_s d(s), ties to the lowest s.  (The
 * device adds the terms of four fixed slices of j, each ascending, and the slices in order: a fixed order, within a few 2^-53 of the
 * plain ascending sum.)  Meaning of the shift: if the query's sensor frame is the entry's turned by yaw about z (T_entry^-1 T_query =
 * rotz(yaw)), the best shift is round(yaw / (2 pi / S)) mod S.
 *
 * Query: the candidates are the entries [first, first + count); the result is the k best (fewer when there are fewer candidates) by
 * ascending (d, index), written to out[0 .. *found); all_dist / all_shift (count values each, or NULL): d and its shift for every
 * candidate.  Zero candidates: *found = 0, nothing launched.
 *
 * The database grows by doubling from 64 entries (a device-to-device copy on the context's stream; earlier entries stay bytewise equal).
 * Commands: sga_places_add three (the fill of the slot, the descriptor, the column norms; one fill for an empty cloud; plus one copy
 * when the database grows), no host wait on a stream-ordered context (a blocking context waits once); sga_places_add_descriptor one;
 * sga_places_query four by cloud (fill, descriptor, match, selection; three for an empty cloud), two by image, exactly one host wait;
 * sga_cloud_scan_context three (fill, descriptor, the hand-over to the host; two for an empty cloud), one wait.
 * Refusals (SGA_ERR_INVALID; outputs untouched) — before any handle is read: NULL arguments (center may be NULL); rings outside [1, 64],
 * sectors outside [1, 256], rings * sectors > 4096, max_range not finite or <= 0, height not finite; a non-finite center; k outside
 * [1, 32] — then, before anything is enqueued: a context, cloud or database of another device; first + count beyond the size; a host
 * image with a non-finite or negative value (named by its position). */
typedef struct sga_place_params {
  int rings, sectors;
  double max_range;
  double height;
} sga_place_params; /* 24 bytes */
typedef struct sga_place_match {
  int64_t index;
  int32_t shift;
  int32_t reserved;
  double distance;
} sga_place_match; /* 24 bytes */
typedef struct sga_places sga_places;
void sga_place_params_default(sga_place_params* p); /* 20, 60, 80.0, 2.0 */
int sga_places_create(sga_context* ctx, const sga_place_params* params, sga_places** out);
int sga_places_destroy(sga_places* db);
int sga_places_size(const sga_places* db, size_t* n);
int sga_places_params(const sga_places* db, sga_place_params* params);
int sga_places_add(sga_context* ctx, sga_places* db, const sga_cloud* cloud, const double center[3] /* or NULL */, size_t* index);
int sga_places_add_descriptor(sga_context* ctx, sga_places* db, const float* image /* R x S */, size_t* index);
int sga_places_download(sga_context* ctx, const sga_places* db, size_t first, size_t count, float* images /* count x R x S */);
int sga_cloud_scan_context(sga_context* ctx, const sga_cloud* cloud, const sga_place_params* params, const double center[3] /* or NULL */, float* image /* R x S */);
int sga_places_query(sga_context* ctx, const sga_places* db, const sga_cloud* cloud, const double center[3] /* or NULL */, size_t first, size_t count, int k, sga_place_match* out /* k */, size_t* found,
                     double* all_dist /* count, or NULL */, int32_t* all_shift /* count, or NULL */);
int sga_places_query_descriptor(sga_context* ctx, const sga_places* db, const float* image /* R x S */, size_t first, size_t count, int k, sga_place_match* out /* k */, size_t* found, double* all_dist /* count, or NULL */,
                                int32_t* all_shift /* count, or NULL */);
/* Fixed-radius neighbourhoods on the device: radius search and clustering, both over one walk of the kd-tree
 * that visits every record within a radius.  THE PREDICATE, for both: record j is a neighbour of q iff d2(q, j) = dx dx + dy dy + dz dz
 * <= radius * radius, formed in double from the fp32 records — two records of one cloud as they are, a query of another device frame as
 * its record plus the origin difference, added in double.  The tree prunes in fp32 against a bound widened so that nothing the predicate
 * accepts is excluded (csrc/kd_radius.hpp); every candidate is tested in double.
 *
 * sga_index_radius_search: for each of the m points of `queries` (any cloud of the context's device; it may be the indexed cloud itself)
 * the records of the kd-tree within radius.  counts (room for m): the number per query, always written.  Lists, on request (offsets
 * non-NULL; then indices and sq_dists are required): CSR — offsets[m + 1], indices[total] (positions in the indexed cloud, not kd
 * positions), sq_dists[total] (double) — in the walk's order within a list, which is reproducible for a given tree and not otherwise
 * specified.  capacity: the room of indices / sq_dists in entries.  When total exceeds it, counts, offsets and result->total are still
 * written, the lists are not, result->overflow is 1 and the status is SGA_OK: call again with room for total.  Passes: count, prefix
 * (one workgroup), fill; one host wait for the counts, a second one behind the copy of the lists.  m == 0, or an index over no points:
 * SGA_OK without device work (counts zeroed).  Refusals (SGA_ERR_INVALID) — before any handle is read: NULL ctx, kdtree, queries, counts or
 * result; offsets without indices and sq_dists; a radius that is not finite and > 0 — then: another device, an index that is no kd-tree
 * (projective: SGA_ERR_UNSUPPORTED), 2^31 queries or more. */
typedef struct sga_radius_result {
  uint64_t total;   /* sum of counts */
  uint64_t written; /* entries of indices / sq_dists written: total, or 0 */
  int overflow;     /* 1: lists were asked for and total > capacity */
  int reserved;
} sga_radius_result; /* 24 bytes */
int sga_index_radius_search(sga_context* ctx, const sga_index* kdtree, const sga_cloud* queries, double radius, size_t capacity, int64_t* counts /* m */, int64_t* offsets /* m + 1, or NULL */,
                            int64_t* indices /* capacity, or NULL */, double* sq_dists /* capacity, or NULL */, sga_radius_result* result);
/* sga_cloud_cluster: DBSCAN with a deterministic border rule, in terms of cloud indices.
 *   core point    i is core iff at least min_points records lie within radius of it, itself included (min_points <= 1: every point).
 *   cluster       two core points within radius of each other are in one cluster: the connected components of that graph.
 *   border point  a non-core point with a core point within radius joins the cluster of its NEAREST core point (d2 in double; ties:
 *                 the lowest cloud index); with none it is noise.
 *   size filter   a cluster's size counts core and border members; clusters outside [min_size, max_size] are dropped (max_size 0: no limit).
 *   numbering     kept clusters are numbered 0 .. C - 1 in ascending order of their SEED, the lowest cloud index among their core points.
 * labels (room for n, or NULL): the number, or -1 for noise and for members of dropped clusters.  table (room for table_capacity rows,
 * or NULL with capacity 0): row c = seed, size and box (min / max of the members' fp32 records + the origin, in double) of cluster c;
 * rows beyond the capacity are not written, result->clusters is the full count.  result (or NULL): clusters kept, noise points, points
 * of dropped clusters, rows written.  The labels are a function of the records alone: not of scheduling, the tree's layout or the call.
 * keep 1 / 2: *out is the cloud of the clustered (label >= 0) / the other points, compacted as sga_cloud_crop does (order, normals,
 * covariances, origin kept; kept, or NULL, room for n: their indices); keep 0: out and kept must be NULL.
 * kdtree: a kd-tree over THIS cloud, checked as sga_cloud_remove_outliers checks it, or NULL: a temporary one (a cloud with a non-finite
 * coordinate has no kd-tree and is refused: crop first).  n == 0: SGA_OK, zero clusters, nothing launched.  One host wait.
 * Refusals (SGA_ERR_INVALID) — before any handle is read: NULL ctx, cloud or params; keep outside [0, 2] or at odds with out / kept; a
 * table without capacity or a capacity without table; a radius that is not finite and > 0; min_points < 1; min_size < 1; max_size < 0;
 * min_size > max_size (max_size > 0) — then: as sga_cloud_remove_outliers. */
typedef struct sga_cluster_params {
  double radius;    /* eps */
  int min_points;   /* records within radius, the point included, that make a core point */
  int keep;         /* 0 no cloud, 1 the clustered points, 2 the rest */
  int64_t min_size; /* >= 1 */
  int64_t max_size; /* 0: no limit */
} sga_cluster_params; /* 32 bytes */
typedef struct sga_cluster_result {
  uint64_t clusters, noise, dropped, rows;
} sga_cluster_result; /* 32 bytes */
typedef struct sga_cluster_row {
  int64_t seed, size;
  double lo[3], hi[3];
} sga_cluster_row; /* 64 bytes */
void sga_cluster_params_default(sga_cluster_params* p); /* radius 0.5, min_points 1, keep 0, min_size 1, max_size 0 */
int sga_cloud_cluster(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree /* over this cloud, or NULL: a temporary one */, const sga_cluster_params* params, int32_t* labels /* n, or NULL */,
                      sga_cluster_row* table /* table_capacity, or NULL */, size_t table_capacity, int64_t* kept /* n, or NULL */, sga_cluster_result* result /* or NULL */, sga_cloud** out /* NULL iff keep == 0 */);
/* Plane segmentation on the device: sga_cloud_segment_plane — the plane with the most points within
 * distance_threshold among `iterations` hypotheses, each through three records, refitted to its inliers.  THE RULE is a function of the
 * records, the parameters and the seed alone.  All arithmetic is in double on the cloud's fp32 records in the cloud's own frame, as
 * differences from a record; r_i is record i as doubles.  The origin enters on the host alone, when the plane is reported.
 *   hypothesis h  id = the draw of sga_ransac_correspondences (seed, h, n); a, b, c = r_id[0], r_id[1], r_id[2]; u = b - a, v = c - a,
 *                 m = u x v = (uy vz - uz vy, uz vx - ux vz, ux vy - uy vx), |w| = sqrt((wx wx + wy wy) + wz wz).  Dropped when
 *                 !(|m| > 0) (a triple with a NaN drops out here), when |m| < 1e-9 |u| |v|, or when !(|m| < infinity) (a triple
 *                 with an infinite coordinate).  nhat = m / |m|.  With an axis: s = (nhat_x axis_x + nhat_y axis_y) + nhat_z axis_z; s < 0
 *                 flips nhat and s; dropped unless s / |axis| >= cos(max_angle).  Without: nhat is flipped so that the first non-zero
 *                 of (nhat_z, nhat_y, nhat_x) is positive.
 *   score         the number of records i with |dist_i| <= distance_threshold, dist_i = (nhat_x dx + nhat_y dy) + nhat_z dz, (dx, dy,
 *                 dz) = r_i - a.  (The device contracts products into the sums, fused multiply-adds, in ONE function that every kernel
 *                 calls.)  A record with a non-finite coordinate is never an inlier: the comparison is false.
 *   best          the greatest score, ties to the lowest h.  scores[h] (room for `iterations`, or NULL): the score, 0xFFFFFFFF for a
 *                 dropped hypothesis.  Nothing scored, or a best score below min_inliers: SGA_OK, result->inliers 0, a zero plane, *out
 *                 an empty cloud (keep 1) or the whole cloud (keep 2).
 *   refit         (refit 1) over the best hypothesis' inliers, x = r_i - a: k, sum x and sum x x^T; c = a + sum x / k, S = sum x x^T -
 *                 (sum x)(sum x)^T / k; the normal is the unit eigenvector of S's smallest eigenvalue (Jacobi), oriented as above.  The
 *                 triple's plane stays, result->refit 0, when k < 3, when lambda_1 - lambda_0 <= 1e-12 lambda_2, or when the refitted
 *                 normal violates the axis constraint.  Sums over points: lane t of workgroup g of G adds the records 256 g + t +
 *                 256 G j, j = 0, 1, ..., in that order; the 256 lanes of a workgroup meet in a binary tree (t += t + 128, 64, ...,
 *                 1); the host adds the workgroups' partials g = 0 .. G - 1 in order, G = min(256, ceil(n / 1024)).
 *   final         the FINAL inliers are the records within distance_threshold of the final plane about its anchor (c, or a).
 *                 plane = (n, d) with n . p + d = 0 in the caller's frame, d = -((n_x (anchor_x + origin_x) + n_y (..)) + n_z (..)).
 *                 result: inliers (final), rmse (sqrt of the mean squared distance of the final inliers, summed as above),
 *                 hypothesis_inliers, best_hypothesis, scored (hypotheses not dropped), refit.
 * keep 1 / 2: *out is the cloud of the final inliers / of all the other records (those with a non-finite coordinate among them),
 * compacted as sga_cloud_crop does (order, normals, covariances, origin kept; kept, or NULL, room for n: their indices); keep 0: out and
 * kept must be NULL.  n < 3: SGA_OK, nothing scored, none of the routine's kernels launched.  Host waits: one behind the sums, one at
 * the end when a refit or a cloud follows.  Refusals (SGA_ERR_INVALID) — before any handle is read, *out = NULL: NULL ctx, cloud, params,
 * plane or result; a distance_threshold that is not finite and > 0; iterations outside [1, 2^20]; a non-finite axis; max_angle outside
 * [0, pi/2], or 0 with a non-zero axis; min_inliers < 3; refit outside {0, 1}; keep outside [0, 2] or at odds with out / kept — then:
 * another device, 2^31 points or more. */
typedef struct sga_plane_params {
  double distance_threshold; /* finite, > 0 */
  uint64_t iterations;       /* hypotheses, 1 .. 2^20 (the hypothesis table is device memory) */
  uint64_t seed;
  double axis[3];            /* 0 0 0: no constraint */
  double max_angle;          /* radians, (0, pi/2], with an axis */
  uint64_t min_inliers;      /* >= 3 */
  int refit;                 /* 0 or 1 */
  int keep;                  /* 0 no cloud, 1 the plane's points, 2 the rest */
} sga_plane_params; /* 72 bytes */
typedef struct sga_plane_result {
  uint64_t inliers;            /* of the final plane */
  double rmse;                 /* over them */
  uint64_t hypothesis_inliers; /* the best hypothesis' score */
  uint64_t best_hypothesis;
  uint64_t scored;             /* hypotheses that were not dropped */
  int refit;                   /* 1: the final plane is the refitted one */
  int reserved;
} sga_plane_result; /* 48 bytes */
void sga_plane_default(sga_plane_params* p); /* distance_threshold 0.1, iterations 1000, seed 0, no axis, min_inliers 3, refit 1, keep 0 */
int sga_cloud_segment_plane(sga_context* ctx, const sga_cloud* cloud, const sga_plane_params* params, double plane[4], uint32_t* scores /* iterations, or NULL */, int64_t* kept /* n, or NULL */,
                            sga_cloud** out /* NULL iff keep == 0 */, sga_plane_result* result);
/* ISS keypoints on the device: sga_cloud_iss_keypoints — the salient points of a cloud (Intrinsic Shape
 * Signatures, as Open3D computes them), in terms of cloud indices.  THE RULE is a function of the records, the tree and the parameters
 * alone.  All arithmetic is in double from the fp32 records of the cloud's own device frame; the origin never enters: everything is a
 * difference from the query's own record.
 *   1 neighbourhood  N_i(r) = { j : d2(i, j) <= r * r }, the predicate of sga_index_radius_search; i is a member.  c_i = |N_i(salient_radius)|.
 *   2 scatter        x_j = r_j - r_i; s = sum x_j and S = sum x_j x_j^T over N_i(salient_radius) in the walk's order;
 *                    C = S / c_i - (s / c_i)(s / c_i)^T, the unweighted covariance; l1 >= l2 >= l3 its eigenvalues (cyclic Jacobi).
 *   3 saliency       sal_i = l3 when c_i >= min_neighbors, l1 > 0, l2 < gamma_21 l1, l3 < gamma_32 l2 and l3 > 1e-9 l1 (products, never a
 *                    division; the floor keeps an exactly planar neighbourhood, whose l3 is rounding noise of either sign, from
 *                    deciding anything); else sal_i = 0.
 *   4 suppression    i is a keypoint iff sal_i > 0, |N_i(non_max_radius)| >= min_neighbors, and no j != i in N_i(non_max_radius) has
 *                    sal_j > sal_i, or sal_j == sal_i with j < i (ties go to the lowest index).
 *   5 determinism    no floating-point atomics: two calls give the same bytes.
 * saliency (room for n, or NULL): sal_i.  kept (room for n, or NULL): the keypoints' indices, ascending; *count: their number.  keep 1:
 * *out is the cloud of the keypoints, compacted as sga_cloud_crop does (order, normals, covariances, origin kept); keep 0: out must be
 * NULL, and no cloud is made.  kdtree: the kd-tree over this cloud, or NULL: a temporary one is built (a cloud with a non-finite
 * coordinate has no kd-tree and is refused: crop first).  n == 0: SGA_OK, nothing launched.  One host wait.  Refusals (SGA_ERR_INVALID)
 * — before any handle is read, *out = NULL and *count = 0: NULL ctx, cloud, params or count; a radius that is not finite and > 0; a gamma
 * outside (0, 1]; min_neighbors < 1; keep outside {0, 1} or at odds with out — then: another device; a tree of another kind, size or
 * device frame. */
typedef struct sga_iss_params {
  double salient_radius; /* finite, > 0: no default */
  double non_max_radius; /* finite, > 0: no default */
  double gamma_21;       /* (0, 1] */
  double gamma_32;       /* (0, 1] */
  int32_t min_neighbors; /* >= 1 */
  int32_t keep;          /* 0 no cloud, 1 the keypoints */
} sga_iss_params; /* 40 bytes */
void sga_iss_default(sga_iss_params* p); /* radii 0 (to be set), gamma_21 = gamma_32 = 0.975, min_neighbors 5, keep 0 */
int sga_cloud_iss_keypoints(sga_context* ctx, const sga_cloud* cloud, const sga_index* kdtree /* over this cloud, or NULL: a temporary one */, const sga_iss_params* params, double* saliency /* n, or NULL */,
                            int64_t* kept /* n, or NULL */, size_t* count, sga_cloud** out /* NULL iff keep == 0 */);
/* ---- occupancy grid: posed scans ray-cast into free and occupied space -----------------------------------------
 * The product a mapping loop hands to a planner or a map cleaner: a volume that says free, occupied or never observed, accumulated over
 * many scans.  A persistent handle on the device; double arithmetic from the fp32 records, integer atomics only, every log-odds value
 * written by one lane per scan: the result is a function of the inputs alone, and two runs give the same bytes.  tests/occupancy_ref.py
 * restates the rule in numpy.
 *
 * THE GRID.  Dense and caller-placed: origin g (the box's minimum corner in the world), leaf > 0, dims nx x ny x nz (each >= 1, product
 * <= 2^27).  inv_leaf = 1.0 / leaf, formed once.  Cell (x, y, z) has the linear index (z * ny + y) * nx + x and holds 8 bytes: a uint32
 * stamp — 0: never observed; otherwise 2 * epoch + (1 if the cell was an endpoint in that scan, else 0) of the last scan that touched it —
 * and an fp32 log-odds L (0 at creation).  l_hit, l_miss, l_min, l_max are fp32 (defaults OctoMap's: 0.85, -0.4, -2.0, 3.5).
 *
 * THE RULE of sga_occupancy_integrate(scan, T, min_range, max_range, mode).  Every successful call advances the epoch by one (an empty
 * scan too); the scan's epoch e is the new value.  The scan is in the sensor frame (record r at the cloud's origin o_c); T = [R t]
 * (column-major 4x4, NULL: the identity) maps the sensor frame into the world, so the sensor sits at t.
 *  1. Per return s = r + o_c (double): rho = sqrt((sx^2 + sy^2) + sz^2), every operation rounded.  A return with a non-finite component
 *     or rho, or with rho < min_range, is IGNORED.  With rho > max_range the beam is TRUNCATED: p = s * (max_range / rho), the quotient
 *     formed once; it marks free space only.  Otherwise the beam is a HIT.
 *  2. Grid coordinates, with q0 = t - g and q = (R o_c + t) - g formed once on the host in double (R o_c per component as (R[k][0] o0 +
 *     R[k][1] o1) + R[k][2] o2):  go = q0 * inv_leaf;  a hit's end ge = ((R r) + q) * inv_leaf, a truncated beam's ge = ((R p) + q0) *
 *     inv_leaf, R v per component as above.  (A return whose ge is not finite — a T that is no rigid motion — is ignored.)  Cells c =
 *     floor(go), ce = floor(ge).
 *  3. The walk, with d = ge - go, per axis a: rem_a = |ce_a - c_a|; if ce_a > c_a: tmax_a = ((c_a + 1) - go_a) / d_a, tdel_a = 1 / d_a;
 *     if ce_a < c_a: tmax_a = (go_a - c_a) / (-d_a), tdel_a = 1 / (-d_a).  While rem_x + rem_y + rem_z > 0: the current cell is a free
 *     candidate; the axis a of least tmax among those with rem_a > 0, ties to the lowest axis, is stepped: c_a moves one cell towards
 *     ce_a, tmax_a += tdel_a, rem_a -= 1.  The walk ends in ce after exactly the Manhattan distance of the two cells; the loop counts
 *     that INTEGER down (at most 3 * (4096 + 2): a beam that would need more is dropped), never a floating-point exit.  A truncated beam
 *     also offers ce as a free candidate; a hit beam offers ce as the hit cell.  Cells outside dims are walked but not touched (the walk
 *     stops early once an axis is outside the box for good: an integer test that changes no result).
 *  4. Per scan a cell is updated ONCE, and an endpoint wins (OctoMap's rule): the hit cells H: L = min(fp32(L + l_hit), l_max), stamp
 *     2 e + 1; the free candidates not in H: L = max(fp32(L + l_miss), l_min), stamp 2 e.  mode 1 (endpoints only) skips the free phase.
 * If the box lies farther than max_range from the sensor (the distance of t to [g, g + dims * leaf], in double on the host), or the scan is
 * empty, the epoch advances and nothing is enqueued (stats: beams alone).
 * Commands: mode 0 two launches — the endpoints (a lane per return: atomicMax(stamp, 2 e + 1), the lane that raised it writes L), then
 * the walk (a lane per beam: a plain load of the stamp skips cells this scan has touched, atomicMax(stamp, 2 e), the lane that raised it
 * writes L) — mode 1 one; NO host wait, on any context: the call returns with its kernels in flight, and every later call on the grid,
 * from whichever context, orders itself behind them.  stats (or NULL): beams, ignored, hits, truncated, and the cells hit / freed,
 * counted where the first toucher is decided; asking for them costs ONE wait.
 *
 * sga_occupancy_classify: per point of a posed cloud (record r at origin o_c; T maps the cloud's frame into the world, NULL: the
 * identity): gc = ((R r) + q) * inv_leaf with q as above; state 0 UNKNOWN: a non-finite gc, a component outside [0, dims), or stamp 0;
 * 1 FREE: L < threshold; 2 OCCUPIED: L >= threshold (L widened to double).  state (room for n, or NULL); counts (or NULL): total = n and
 * the three counts, with the epoch.  keep_mask: bit 0 unknown, bit 1 free, bit 2 occupied; 0 — no cloud, out must be NULL; otherwise *out
 * receives the points whose state's bit is set as an ordinary cloud, by the compaction of sga_cloud_crop: the cloud's order, origin,
 * normals and covariances, record j of *out equal to record kept[j] bit for bit (a non-finite record is unknown, and kept with bit 0);
 * nothing kept, or an empty cloud, yields an empty cloud without attributes.  kept (room for n, or NULL; only with keep_mask != 0): the
 * indices kept, ascending.  keep_mask 5 is the cleaner a keyframe runs against accumulated evidence.  One launch and one wait; with an
 * output cloud the compaction's table copy and launch follow, and the one wait is the compaction's.  An empty cloud enqueues nothing.
 * sga_occupancy_stats: the unknown / free / occupied cells (total = the cells) and the epoch; one launch, one wait.
 * sga_occupancy_export: the cells whose state's bit is set in which_mask (1 .. 7), in ascending linear index, the first min(*count,
 * capacity) of them written: *out (or NULL) a cloud of cell centres at origin g with the records fp32((i + 0.5) * leaf) per axis,
 * indices (or NULL) their linear indices, log_odds (or NULL) their L; *count: the number selected, whatever the capacity.  The count needs
 * ONE wait (one launch); the fill — two more launches, only when something is selected and asked for — a SECOND (a stream-ordered context
 * that asks for the cloud alone returns without it).
 * sga_occupancy_download: the raw arrays (stamp and / or log_odds, room for the cells each), for tests and persistence.
 * sga_occupancy_clear: every cell back to {0, 0} and the epoch to 0; one fill.  sga_occupancy_get: the parameters and / or the epoch.
 *
 * Refusals (SGA_ERR_INVALID; *out = NULL on every failure, nothing enqueued) — before any handle is read: NULL arguments; create: a
 * non-finite origin, leaf not finite or <= 0, a dim below 1, more than 2^27 cells, a non-finite log-odds parameter, l_hit <= 0, l_miss >=
 * 0, l_min >= l_max; integrate: min_range not finite or < 0, max_range not finite or < min_range, a mode other than 0 or 1; a
 * non-finite entry of T; a NaN threshold; keep_mask outside 0 .. 7, out given with keep_mask 0 or missing otherwise, kept given with
 * keep_mask 0; which_mask outside 1 .. 7 — then: a grid or cloud of another device, 2^31 points or more, max_range / leaf > 4096, an
 * epoch of 2^31 - 1. */
typedef struct sga_occupancy_params {
  double origin[3];
  double leaf;
  int dims[3];
  int reserved;
  float l_hit, l_miss, l_min, l_max;
} sga_occupancy_params; /* 64 bytes */
typedef struct sga_occupancy_scan_stats {
  size_t beams, ignored, hits, truncated, cells_hit, cells_freed;
} sga_occupancy_scan_stats; /* 48 bytes */
typedef struct sga_occupancy_counts {
  size_t total, unknown, free, occupied;
  uint64_t epoch;
} sga_occupancy_counts; /* 40 bytes */
typedef struct sga_occupancy sga_occupancy;
void sga_occupancy_params_default(sga_occupancy_params* p); /* origin 0, leaf 0 and dims 0 (to be set), 0.85, -0.4, -2.0, 3.5 */
int sga_occupancy_create(sga_context* ctx, const sga_occupancy_params* params, sga_occupancy** out);
int sga_occupancy_destroy(sga_occupancy* grid);
int sga_occupancy_get(const sga_occupancy* grid, sga_occupancy_params* params /* or NULL */, uint64_t* epoch /* or NULL */);
int sga_occupancy_clear(sga_context* ctx, sga_occupancy* grid);
int sga_occupancy_integrate(sga_context* ctx, sga_occupancy* grid, const sga_cloud* scan, const double T[16] /* or NULL */, double min_range, double max_range, int mode, sga_occupancy_scan_stats* stats /* or NULL */);
int sga_occupancy_classify(sga_context* ctx, const sga_occupancy* grid, const sga_cloud* cloud, const double T[16] /* or NULL */, double threshold, int keep_mask, uint8_t* state /* n, or NULL */,
                           int64_t* kept /* n, or NULL; only with keep_mask != 0 */, sga_occupancy_counts* counts /* or NULL */, sga_cloud** out /* NULL iff keep_mask == 0 */);
int sga_occupancy_stats(sga_context* ctx, const sga_occupancy* grid, double threshold, sga_occupancy_counts* counts);
int sga_occupancy_export(sga_context* ctx, const sga_occupancy* grid, double threshold, int which_mask, size_t capacity, int64_t* indices /* capacity, or NULL */, float* log_odds /* capacity, or NULL */, size_t* count,
                         sga_cloud** out /* or NULL */);
int sga_occupancy_download(sga_context* ctx, const sga_occupancy* grid, uint32_t* stamp /* cells, or NULL */, float* log_odds /* cells, or NULL */);
int sga_cloud_destroy(sga_cloud* cloud);
int sga_cloud_size(const sga_cloud* cloud, size_t* n);
int sga_cloud_has(const sga_cloud* cloud, int* has_normals, int* has_covs);
/* Any of xyz / normals / cov6 may be NULL. */
int sga_cloud_download(sga_context* ctx, const sga_cloud* cloud, float* xyz, float* normals, float* cov6);
/* the same with the points in double (device record + origin, added in double): what a caller far from the origin wants back */
int sga_cloud_download_f64(sga_context* ctx, const sga_cloud* cloud, double* xyz, float* normals, float* cov6);

/* ---- device-resident data: clouds, queries and results that never touch the host ------------------------------------------------
 * A caller whose scan is in device memory already (a tensor from a driver, a range image unprojected on the device, the output of its
 * own filter) hands over the device pointer; results are written into device arrays of the caller's.  One struct describes an array:
 * rows of `stride` elements of which the first `cols` are used, so an N x 4 KITTI scan goes down as cols 3, stride 4 without a copy.
 *
 * Ordering, the same for the four calls.  user_stream is the hipStream_t the caller produced the inputs on and will consume the outputs
 * on (NULL: the null stream).  Unless it is the context's own stream, or flags has SGA_IO_NO_ORDER, the call records an event on
 * user_stream, makes the context's stream wait for it ahead of the first kernel that touches the caller's memory, records a second
 * event behind the last such kernel and makes user_stream wait for that one before it returns: work the caller enqueues on user_stream
 * afterwards (a caching allocator handing the block out again included) is ordered behind the library's accesses.  The host waits for
 * neither.  A blocking context synchronises its stream once at the end, as everywhere; a stream-ordered context returns with the work
 * enqueued.  With SGA_IO_NO_ORDER the caller orders the two streams itself.
 *
 * Refusals (SGA_ERR_INVALID, before any launch): null arguments; 2^31 rows or more; a dtype, cols or stride other than the struct
 * allows; cols the array cannot have; normals / covariances asked from a cloud without them; a data pointer that is not device
 * memory of the context's device (host memory, pinned or pageable, is named as such, with the host entry point that takes it); a
 * data pointer whose [data, data + rows * stride * element size) is not inside the allocation the runtime knows it by.  These checks
 * are what keeps a caller's wrong row count from faulting the device. */
enum { SGA_F32 = 0, SGA_F64 = 1 };
typedef struct sga_device_array {
  const void* data; /* device memory of the context's device (written through by the export call) */
  int dtype;        /* SGA_F32 | SGA_F64 */
  int cols;         /* layout of a row: points 3, normals 3, covariances 6 (xx xy xz yy yz zz) | 9 (3x3) | 16 (4x4, the reference's) */
  int stride;       /* elements from one row to the next, >= cols */
} sga_device_array;
enum { SGA_IO_NO_ORDER = 1, SGA_IO_RELATIVE = 2 };
/* The cloud of n points from device arrays; normals / covs may be NULL and may differ from the points in dtype.  origin NULL: absolute
 * coordinates, the origin chosen from the box of the finite coordinates as sga_cloud_create_f32 / _f64 choose it (the box comes back
 * from the device as a note: the one host wait the data forces); origin given: absolute coordinates recentred about it, the
 * subtraction done in double (sga_cloud_create_f64_origin); origin given with SGA_IO_RELATIVE: the records are taken as they are
 * (sga_cloud_create_f32_origin).  The result is an ordinary cloud with the records, the origin and the bounding box the host entry
 * point makes from the same values, bit for bit; covariances given as 3x3 or 4x4 rows contribute m[0], m[1], m[2], m[5], m[6], m[10] (of
 * the 4x4).  With origin given a stream-ordered context waits for nothing; its cloud then carries no bounding box (the box only shortens
 * the voxel grid's sort keys, results do not depend on it).  n == 0 is SGA_OK with *out = NULL: nothing is examined and no cloud is
 * made (an empty cloud comes from sga_cloud_create_f32 with n = 0). */
int sga_cloud_create_device(sga_context* ctx, const sga_device_array* points, const sga_device_array* normals, const sga_device_array* covs, size_t n, const double origin[3], void* user_stream, int flags, sga_cloud** out);
/* sga_cloud_download / _f64 into device arrays of the caller's (any of the three may be NULL; those given share one dtype): the points in
 * the caller's frame — the origin is added in double, the sum rounded to dtype —, normals 3 per row, covariances 6, 9 (the symmetric
 * 3x3) or 16 (4x4, fourth row and column zero) per row.  Elements of a row past its cols are left untouched. */
int sga_cloud_export_device(sga_context* ctx, const sga_cloud* cloud, const sga_device_array* points, const sga_device_array* normals, const sga_device_array* covs, void* user_stream, int flags);
/* sga_cloud_deskew with the times in device memory (above: "Raw sweeps deskewed on the device") */
int sga_cloud_deskew_device(sga_context* ctx, const sga_cloud* cloud, const sga_device_array* times /* float | double, cols 1, any stride */, const double twist[6], double ref_time, void* user_stream, int flags, sga_cloud** out);
/* sga_cloud_crop with the indices kept written to device memory: d_kept (or NULL) is device memory of the context's device with room for
 * the cloud's size in int64, checked against its allocation; the first size-of-*out entries are written.  user_stream is ordered as
 * sga_cloud_create_device orders it (flags: SGA_IO_NO_ORDER). */
int sga_cloud_crop_device(sga_context* ctx, const sga_cloud* cloud, const sga_crop* crop, int64_t* d_kept, void* user_stream, int flags, sga_cloud** out);
/* sga_index_knn for m queries in device memory (float or double rows; the search runs on fl32(double(q) - origin of the index), computed
 * by a kernel): d_idx m*k int64 and d_sq_dist m*k floats, device memory of the caller's.  kd-trees, Gaussian and flat voxel maps, with
 * the kernels, k limits and messages of the host call; a projective index is SGA_ERR_UNSUPPORTED, and the double distances of
 * sga_index_knn_f64 stay a host-only form.  m == 0 is SGA_OK with nothing examined. */
int sga_index_knn_device(sga_context* ctx, const sga_index* index, const sga_device_array* queries, size_t m, int k, double max_sq_dist, int64_t* d_idx, float* d_sq_dist, void* user_stream, int flags);
/* sga_problem_get_factors into device memory: d_target_index n int64, d_mahalanobis6 n*6 floats (one of them may be NULL). */
int sga_problem_get_factors_device(sga_context* ctx, const sga_problem* problem, int64_t* d_target_index, float* d_mahalanobis6, void* user_stream, int flags);

/* ---- preprocessing (registration_helper.cpp:22-34 preprocess_points) ----------------------------------------------- */
/* util/downsampling.hpp:23-78 voxelgrid_sampling: centroid per occupied voxel, output in ascending packed-key order. */
int sga_voxelgrid_sampling(sga_context* ctx, const sga_cloud* in, double leaf_size, sga_cloud** out);
/* The voxel grid that carries per-point columns — times, intensities, rings, labels — through the merge.
 * *out is the cloud sga_voxelgrid_sampling makes of `in`, byte for byte; voxel v is its row v.  The members of a voxel are the input
 * points whose voxel it is, taken in ascending original index i_0 < ... < i_{N-1}.  Row v of *out_fields holds, per column c under
 * ops[c] (ops NULL: MEAN each):
 *   MEAN     fl32(S / N), S the sum of the N values formed in double in an order that depends on N alone (no atomics);
 *   MIN/MAX  the least / greatest value (equal under ==; the sign of a zero is not specified); NaN values are skipped, all NaN: NaN;
 *   FIRST    the value of i_0, bit for bit;
 *   NEAREST  the value, bit for bit, of the member whose fp32 record r minimises sum_a (double(r_a) - double(c_a))^2, c the fp32
 *            record this call writes for the voxel; ties go to the lowest original index.  (What a column that must come from ONE
 *            real return follows the grid by: a time across the seam of a sweep, a label.)
 * counts[v] = N (or NULL; room for in's size, the first size-of-*out entries are written); voxel_of[i] = the row of input point i, -1
 * for a point the grid drops (a non-finite coordinate, outside the grid), or NULL.  fields == NULL with out_fields == NULL: membership
 * only.  Two calls give the same bytes in every output.  The chain is sga_voxelgrid_sampling's — keys, one sort, the runs — with ONE
 * other last launch that writes the centroids, every reduced column, counts and voxel_of; one host wait, the voxel count.  An empty
 * input, or one of which every point is dropped: an empty cloud and an empty features handle of the same dim.
 * Refusals (SGA_ERR_INVALID, every out pointer NULL, nothing enqueued) — before any handle is read: NULL ctx, in or out; out_fields
 * NULL with fields given, or the reverse; a leaf that is not positive; in the device form, whose struct tells the number of columns,
 * a dtype, cols outside [1, 32] or stride the struct cannot have and an op outside 0..4, named by its column — then (the host form
 * reads the number of ops from the handle: its dim and its ops are checked first): fields or a cloud of another device, 2^31 points or
 * more, a row count other than the cloud's size; for the device form the pointer checks of sga_cloud_create_device, for fields (the
 * last row need only reach its last column: scan[:, 3:4] of an N x 4 tensor goes down as a view), d_counts and d_voxel_of. */
enum { SGA_REDUCE_MEAN = 0, SGA_REDUCE_MIN = 1, SGA_REDUCE_MAX = 2, SGA_REDUCE_FIRST = 3, SGA_REDUCE_NEAREST = 4 };
int sga_voxelgrid_sampling_fields(sga_context* ctx, const sga_cloud* in, const sga_features* fields /* in's size rows, dim 1..32; or NULL */, const int* ops /* dim entries, or NULL: MEAN each */, double leaf_size, sga_cloud** out,
                                  sga_features** out_fields /* NULL iff fields is NULL */, int32_t* counts /* or NULL */, int64_t* voxel_of /* or NULL; in's size entries */);
/* the same with the fields in device memory of the caller's (float | double — a double is rounded to fp32 once, on entry —, cols = dim,
 * any stride >= cols) and counts / voxel_of written to device memory; user_stream and flags order the streams as
 * sga_cloud_create_device does */
int sga_voxelgrid_sampling_fields_device(sga_context* ctx, const sga_cloud* in, const sga_device_array* fields, const int* ops, double leaf_size, sga_cloud** out, sga_features** out_fields, int32_t* d_counts, int64_t* d_voxel_of,
                                         void* user_stream, int flags);
/* sga_voxelgrid_sampling(ctx, clouds[k], leaf_size, &out[k]) for `count` clouds on the context's device in one chain of launches on the
 * context's stream — keys, ONE sort over the concatenation under the key (member << W) | the member's own short key, runs, centroids —
 * whose length does not grow with count.  out[k] is an ordinary cloud, owning its buffers, in the input's device frame, its records
 * bit-identical to the lone call's.  The chain takes the members that have a bounding box (uploads), 1 .. 262144 points, and whose
 * composite key fits 64 bits (2^24 points in all); the others — clouds made on the device, larger ones — go through the lone routine, one
 * after the other, inside the call; an empty member gives an empty cloud.  The same cloud may appear twice (inputs are only read); a member
 * made by another context of the device is waited for.  The host waits once, for the voxel counts of all members of the chain.  All
 * arguments are checked before any device work (status and message as the lone call's, naming the member); on any failure every out[k]
 * is NULL.  count == 0 is SGA_OK. */
int sga_voxelgrid_sampling_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, double leaf_size, sga_cloud** out);
/* util/normal_estimation.hpp:65-92 estimate_local_features: kNN(k, incl. self) -> mean/cov -> eigvecs -> normal / covariance.
 * index: a kd-tree built over `cloud`, or NULL to build a temporary one.  flags: bit0 = normals, bit1 = covariances. */
int sga_estimate_normals_covariances(sga_context* ctx, sga_cloud* cloud, const sga_index* index, int num_neighbors, int flags);
/* sga_estimate_normals_covariances for `count` (cloud, kd-tree index built over that cloud) pairs on the context's device in one chain
 * of launches on the context's stream (a member made by another context of that device is waited for, as in the lone call; a member on
 * another device is SGA_ERR_INVALID); every cloud and index gets, bit for bit, what the lone call gives it.  indices[k] must not be NULL, no cloud or index may
 * appear twice.  Members of more than sga_set_knn_wave_max points (default 81920), and calls with num_neighbors > 64, are estimated by
 * the lone routine, one after the other, inside the call.  All arguments are checked before any device work.  count == 0 is SGA_OK. */
int sga_estimate_normals_covariances_batch(sga_context* ctx, sga_cloud* const* clouds, sga_index* const* indices, size_t count, int num_neighbors, int flags);

/* ---- search indices --------------------------------------------------------------------------------------------- */
/* Replaces KdTree<PointCloud>(points) (ann/kdtree.hpp:80-126, :250-252): exact nearest neighbour / kNN over `target`.
 * An implicit, perfectly balanced kd-tree (median splits like the reference, no pointers) built on the GPU; the index keeps its
 * own kd-ordered copy of the target's points / normals / covariances. */
int sga_index_build_kdtree(sga_context* ctx, const sga_cloud* target, sga_index** out);
/* sga_index_build_kdtree for `count` clouds on the context's device in one chain of launches on the context's stream (a cloud made by
 * another context of that device is waited for, as in the lone call; a cloud on another device is SGA_ERR_INVALID): out[k] is an ordinary kd-tree index over clouds[k],
 * bit-identical to the lone call's, owning its buffers, destroyed with sga_index_destroy in any order.  Clouds of at most 32768 points
 * (a LiDAR scan after the voxel grid) share the launches — B scans of similar size cost the launches of one; empty and larger clouds are
 * built by the lone path, one after the other, inside the call.  The host waits once for the bounding boxes of all members; a member
 * with non-finite coordinates fails the call (SGA_ERR_INVALID).  On any failure every out[k] is NULL.  count == 0 is SGA_OK. */
int sga_index_build_kdtree_batch(sga_context* ctx, const sga_cloud* const* clouds, size_t count, sga_index** out);
/* Replaces create_gaussian_voxelmap (registration_helper.cpp:50-54; ann/incremental_voxelmap.hpp:55-92, gaussian_voxelmap.hpp:32-53):
 * one-shot insert of a cloud WITH covariances; voxel ids follow first-insertion order like the reference. */
int sga_index_build_gaussian_voxelmap(sga_context* ctx, const sga_cloud* points_with_covs, double leaf_size, sga_index** out);
/* sga_index_build_gaussian_voxelmap(ctx, clouds_with_covs[k], leaf_size, &out[k]) for `count` clouds on the context's device in one chain
 * of launches on the context's stream — keys, ONE stable sort over the concatenation under the key (member << 49) | 16 bits per axis,
 * runs, one sort of all runs for the voxel ids, one launch that clears every hash table, one finalize launch — whose length does not grow
 * with count.  out[k] is an ordinary one-shot voxel-map index: it owns its buffers, is destroyed with sga_index_destroy in any order, is a
 * search target (not insertable) in its cloud's device frame with the default search offsets, and its contents (coordinates, counts,
 * means, covariances, voxel ids) are bit-identical to the lone call's; only the layout of its hash table may differ.  The chain takes, in
 * the call's order, the members of 1 .. 262144 points while their concatenation stays within 2^24 points; larger members, and members
 * that span 65536 or more voxels along an axis (the device finds out, the host hears of it at its wait), go through the lone routine, one
 * after the other, inside the call; an empty member gives an empty map.  The same cloud may appear twice (inputs are only read); a member
 * made by another context of the device is waited for.  The host waits ONCE, for the voxel counts of all members of the chain, then
 * allocates every index at its exact size and enqueues the rest: a stream-ordered context returns without a second wait, other contexts
 * synchronise once at the end.  All arguments are checked before any device work (status and message as the lone call's, naming the
 * member); on any failure every out[k] is NULL.  count == 0 is SGA_OK. */
int sga_index_build_gaussian_voxelmap_batch(sga_context* ctx, const sga_cloud* const* clouds_with_covs, size_t count, double leaf_size, sga_index** out);
/* The same kind of index from voxels that already exist on the host — the reference's GaussianVoxelMap object as it is (flat order:
 * coords n*3 int32, means n*3 doubles, cov6 n*6 doubles xx,xy,xz,yy,yz,zz; ann/incremental_voxelmap.hpp:39-92): the voxel ids are the
 * caller's.  What lets Registration<GICPFactor, ParallelReductionHIP>::align(voxelmap, source, voxelmap) (registration_helper.cpp:125-137) work. */
int sga_index_create_voxelmap_from_voxels(sga_context* ctx, double leaf_size, const int32_t* coords, const double* means3, const double* cov6, size_t n, sga_index** out);
/* A flat voxel map (IncrementalVoxelMap<FlatContainer*>, ann/flat_container.hpp:21-58) from voxels that exist on the host, flat order: coords
 * n*3, counts n (<= 16 each), points n*16*3 doubles and cov6 n*16*6 doubles (16 slots per voxel, the first counts[v] valid; cov6 may be NULL
 * for ICP), searched over 1, 7 or 27 voxels.  Target indices are (voxel_id << 32) | point_id with the caller's ids. */
int sga_index_create_flatmap_from_voxels(sga_context* ctx, double leaf_size, const int32_t* coords, const uint32_t* counts, const double* points3, const double* cov6, int search_offsets, size_t n, sga_index** out);
/* Re-copy normals / covariances from `cloud` (the cloud the tree was built over) into the index's kd-ordered arrays, e.g. after
 * attributes were estimated or set once the index already existed (reference flow: KdTree first, estimate_covariances second). */
int sga_index_refresh_attributes(sga_context* ctx, sga_index* index, const sga_cloud* cloud);
/* A deep copy of an index on ctx's device, which may differ from the source's (peer copy): a replicated target reaches the other GPUs of a
 * sharded registration without being built once per GPU. */
int sga_index_clone(sga_context* ctx, const sga_index* src, sga_index** out);
int sga_index_destroy(sga_index* index);
/* Number of target points (kd-tree) or voxels (voxel map): traits::size(target). */
int sga_index_size(const sga_index* index, size_t* n);
/* Voxel map contents in voxel-id order: coords n*3 int32, means n*3, cov6 n*6, counts n (any may be NULL). */
int sga_index_voxelmap_download(sga_context* ctx, const sga_index* index, int32_t* coords, float* means, float* cov6, uint32_t* counts);
/* Incremental GaussianVoxelMap (ann/incremental_voxelmap.hpp:55-92, the scan-to-model target): an empty map, then any number of
 * insert(points_with_covs, T): the points are moved by T (column-major 4x4, NULL = identity), voxels keep running means over
 * everything ever inserted while they live, voxel ids follow the creation order, and every `clear_cycle` inserts the voxels not
 * touched for more than `horizon` inserts are removed (defaults 100 / 10, incremental_voxelmap.hpp:46).  Usable as the target of
 * sga_problem_create / sga_align like a one-shot map; problems created before an insert must be re-created. */
int sga_voxelmap_create(sga_context* ctx, double leaf_size, sga_index** out);
int sga_voxelmap_insert(sga_context* ctx, sga_index* voxelmap, const sga_cloud* points_with_covs, const double T[16]);
/* sga_voxelmap_insert(ctx, maps[k], clouds_with_covs[k], T + 16 k) for k = 0 .. count - 1 (T: count column-major 4x4 matrices, NULL =
 * identities): B scans into the B maps of B scan-to-model streams.  Afterwards every map holds exactly what the lone call leaves — voxel
 * ids in creation order, coordinates, counts, the fp64 means and covariances and the exported fp32 records, the origin of the export, the
 * LRU stamps and counter, the LRU sweep when it falls due — bit for bit; only the layout of a hash table may differ.  Incremental GAUSSIAN
 * maps with clouds of 1 .. 262144 points share one chain of launches on the context's stream (while their concatenation stays within
 * 2^24 points) and ONE host wait, for the members' voxel counts; behind it every map grows under the lone call's conditions, LRU sweeps
 * that fall due run one map at a time, and one launch exports the records of all maps.  A member whose scan spans 65536 or more voxels
 * along an axis (the device finds out), a larger cloud and a FLAT map of any contents go through the lone routine inside the call, one
 * after the other: a batched flat-map update is not built.  An empty cloud advances its map's insert counter (and sweeps, and exports)
 * as the lone call does.  A map may appear ONCE per call (two inserts into one map are ordered: SGA_ERR_INVALID); a cloud may appear
 * several times; members made by another context of the device are waited for.  Every member is checked before any device work, with
 * the lone call's status and message plus the member's number; on such a failure no map is touched.  count == 0 is SGA_OK.  Blocking
 * contexts synchronise once at the end; stream-ordered contexts return after the one wait. */
int sga_voxelmap_insert_batch(sga_context* ctx, sga_index* const* maps, const sga_cloud* const* clouds_with_covs, const double* T, size_t count);
int sga_voxelmap_set_lru(sga_index* voxelmap, uint32_t horizon, uint32_t clear_cycle);
/* IncrementalVoxelMap<FlatContainerCov> (ann/flat_container.hpp:15-100): voxels that keep up to max_num_points_in_cell (default 10,
 * at most 16) of the inserted points, at least sqrt(min_sq_dist_in_cell) (default 0.1 m) apart, with their covariances — the
 * scan-to-model GICP target (odometry_benchmark_small_gicp_model_omp.cpp).  Inserted with sga_voxelmap_insert / _set_lru like a
 * Gaussian map; searched over 1, 7 or 27 voxels (incremental_voxelmap.hpp:157-186); target indices are (voxel_id << 32) | point_id. */
int sga_flatmap_create(sga_context* ctx, double leaf_size, sga_index** out);
int sga_flatmap_set_setting(sga_index* flatmap, double min_sq_dist_in_cell, uint32_t max_num_points_in_cell);
/* Voxels visited around the query's own (incremental_voxelmap.hpp:157-186): 1 (default), 7 or 27 — for flat AND Gaussian maps, incremental,
 * one-shot or created from host voxels; every visited Gaussian voxel offers its mean, the nearest wins (the first of equal distances). */
int sga_voxelmap_set_search_offsets(sga_index* voxelmap, int num_offsets);
/* coords n*3, counts n, points n*16*3 and cov6 n*16*6 (16 slots per voxel, the first counts[v] of them valid); any pointer may be NULL
 * (a map without covariances: cov6 is filled with zeros) */
int sga_flatmap_download(sga_context* ctx, const sga_index* flatmap, int32_t* coords, uint32_t* counts, float* points, float* cov6);
/* The four contents of the reference's flat container (ann/flat_container.hpp:18-58, FlatContainer<HasNormals, HasCovs>; the Python names
 * IncrementalVoxelMap / IncrementalVoxelMapNormal / IncrementalVoxelMapCov / IncrementalVoxelMapNormalCov, src/python/voxelmap.cpp:146-151):
 * `contents` = 0 (points only), SGA_FLAT_NORMALS, SGA_FLAT_COVS or both.  A kept point's normal is R n (T.matrix() * normal, w = 0), its
 * covariance R C R^T; the accept / reject rule depends on the points alone, so every kind keeps the same points in the same slots.
 * sga_voxelmap_insert then needs exactly the attributes the map keeps.  Targets: ICP for every kind, PLANE_ICP where the map keeps normals
 * (its target normal is the one stored in the matched slot), GICP where it keeps covariances.  sga_flatmap_create = SGA_FLAT_COVS. */
enum { SGA_FLAT_NORMALS = 1, SGA_FLAT_COVS = 2 };
int sga_flatmap_create_contents(sga_context* ctx, double leaf_size, int contents, sga_index** out);
/* Which contents a flat map keeps (SGA_FLAT_NORMALS | SGA_FLAT_COVS bits). */
int sga_flatmap_get_contents(const sga_index* flatmap, int* contents);
/* sga_flatmap_download with the normals: normals n*16*3 floats.  normals / cov6 must be NULL where the map keeps none (SGA_ERR_INVALID). */
int sga_flatmap_download_contents(sga_context* ctx, const sga_index* flatmap, int32_t* coords, uint32_t* counts, float* points, float* normals, float* cov6);
/* sga_index_create_flatmap_from_voxels with the normals of the slots (normals3 n*16*3 doubles, NULL = none): the reference's
 * IncrementalVoxelMap<FlatContainer<HasNormals, HasCovs>> object as it is.  The contents follow the non-NULL arrays. */
int sga_index_create_flatmap_from_voxels_contents(sga_context* ctx, double leaf_size, const int32_t* coords, const uint32_t* counts, const double* points3, const double* normals3, const double* cov6, int search_offsets, size_t n,
                                                   sga_index** out);
/* traits::knn_search / nearest_neighbor_search (ann/traits.hpp:22-57) for m host queries (m*3 floats):
 * idx m*k int64 (original target indices, -1 = none), sq_dist m*k floats ascending (inf = none).
 * max_sq_dist < 0 means unbounded.  k <= 116 for kd-trees.  Voxel maps (Gaussian and flat, incremental_voxelmap.hpp:99-149): any
 * k <= 128, the voxels at the map's search offsets in the reference's order, KnnResult::push semantics; idx is then the reference's global
 * index (voxel_id << 32) | point_id (point_id = 0 for a Gaussian voxel, the slot within its voxel for a flat map). */
int sga_index_knn(sga_context* ctx, const sga_index* index, const float* queries, size_t m, int k, double max_sq_dist, int64_t* idx, float* sq_dist);
/* The same with the reference's types (double queries m*3, double squared distances): the search runs on the fp32 roundings of the
 * queries, the squared distances of the neighbours found are then evaluated in double against the double queries (the reference's
 * Python tests compare them with scipy to 1e-6 at ranges where fp32 resolves 1e-4, src/test/python_test.py:194-257). */
int sga_index_knn_f64(sga_context* ctx, const sga_index* index, const double* queries, size_t m, int k, double max_sq_dist, int64_t* idx, double* sq_dist);

/* Replaces ProjectiveSearch<PointCloud>(width, height, target) (ann/projective_search.hpp:161-163, UnsafeProjectiveSearch :49-62):
 * the equirectangular index image of `cloud` (EquirectangularProjection :13-27; y down, z forward), one pixel per point, the highest
 * index owning a pixel; points whose pixel lies out of the image (u == width) are dropped, non-finite points are skipped (undefined in
 * the reference).  Search window 10 / 5, BorderRepeat horizontally and BorderClamp vertically (:42, :49).  A target for
 * sga_problem_create / sga_align (ICP, PLANE_ICP with target normals, GICP with target covariances; correspondences and kNN indices are
 * the cloud's own indices) and for sga_index_knn / _f64 (any k <= 128; the scan of :107-140 with KnnResult::push, duplicates of a column
 * visited twice kept; the _f64 form measures double distances, sga_index_knn float ones).  Not usable as a source index, with a host
 * rejector, for per-point factors or for normal / covariance estimation (SGA_ERR_UNSUPPORTED). */
int sga_index_build_projective(sga_context* ctx, const sga_cloud* cloud, int width, int height, sga_index** out);
/* search_window_h / search_window_v (:153-154), read at each search; each in [0, 65535]. */
int sga_projective_set_search_window(sga_index* index, int h, int v);
/* BorderModeH / BorderModeV (:41-42): non-zero = BorderRepeat (wraps once), 0 = BorderClamp (out-of-range rows / columns are skipped). */
int sga_projective_set_border_modes(sga_index* index, int repeat_h, int repeat_v);
/* {width, height, window h, window v, repeat_h, repeat_v} */
int sga_projective_get_params(const sga_index* index, int out[6]);
/* index_map (:152) in the reference's layout: out[v * width + u] = index_map(v, u), 0xFFFFFFFF = invalid_index. */
int sga_projective_download_map(sga_context* ctx, const sga_index* index, uint32_t* out);

/* ---- the hot path: Reduction::linearize / Reduction::error (registration/reduction_omp.hpp:24-70) ------------------------- */
typedef struct sga_factor_params {
  int factor_kind;    /* sga_factor_kind */
  int robust_kind;    /* sga_robust_kind */
  double robust_c;    /* robust kernel width (robust_kernel.hpp:16,42) */
  double max_dist_sq; /* DistanceRejector::max_dist_sq (rejector.hpp:19-28); < 0 = NullRejector */
  int math_mode;      /* sga_math_mode */
} sga_factor_params;
void sga_factor_params_default(sga_factor_params* p);

/* Pair a target index with a source cloud.  The problem keeps a spatially sorted copy of the source (sorted by the target kd-leaf
 * init_T * p falls into) and the per-point factor state (target index + cached mahalanobis), i.e. registration.hpp:41. */
int sga_problem_create(sga_context* ctx, const sga_index* target, const sga_cloud* source, const double init_T[16], sga_problem** out);
/* The same with the source given by ITS OWN kd-tree index (the odometry loop, src/benchmark/odometry_benchmark_small_gicp_omp.cpp:22-38:
 * every scan is indexed once, for its covariances and as the next target): the problem takes the index's kd-ordered points and
 * covariances as they are — the order is spatially coherent already, so no sort.  Factor state is reported in the ORIGINAL order of the
 * cloud the index was built over, exactly as with sga_problem_create.  Attributes must be present in the index (build it after
 * estimating them, or call sga_index_refresh_attributes). */
int sga_problem_create_from_index(sga_context* ctx, const sga_index* target, const sga_index* source_index, const double init_T[16], sga_problem** out);
/* registration.hpp:41 for B pairs: out[k] is what sga_problem_create(ctx, targets[k], sources[k], init_T + 16 k, &out[k]) makes — an
 * ordinary sga_problem with its own buffers, the source in the lone call's order bit for bit, usable and destroyable like any other.
 * Sources of 1 .. 262144 points against kd-tree, Gaussian or flat targets share ONE chain on the context's stream whatever B is: a table
 * copy, a keys launch, one stable sort of the concatenation under (member, the member's lone key), one launch that gathers, writes the
 * initial factor state and reduces every member's bounding box — and ONE host wait, for the boxes of all members.  Larger clouds, members
 * with a projective target and empty sources go through the lone routine inside the call.  A target may serve several members, a cloud
 * may appear several times; a mix of target kinds is fine here (sga_batch_create still refuses it).  A NULL member or a member on
 * another device is refused before any device work with the lone call's status and message plus the member's number; a member with a
 * non-finite coordinate fails the call with SGA_ERR_INVALID "source cloud contains non-finite coordinates (problem k)".  On any failure
 * every out[k] is NULL.  count == 0 is SGA_OK. */
int sga_problem_create_batch(sga_context* ctx, const sga_index* const* targets, const sga_cloud* const* sources,
                             const double* init_T /* count x 16 column-major, or NULL: identities */, size_t count, sga_problem** out);
int sga_problem_destroy(sga_problem* problem);
/* Sum_i (H_i, b_i, e_i) at T over all source points with a correspondence; refreshes the factor state. */
int sga_linearize(sga_context* ctx, sga_problem* problem, const sga_factor_params* params, const double T[16], double H[36], double b[6], double* e, uint64_t* num_inliers);
/* Sum_i e_i at T with the correspondences and mahalanobis cached by the last sga_linearize (gicp_factor.hpp:80-89).  With those
 * frozen the sum is a quadratic polynomial in T: sga_linearize accumulates its coefficients next to H / b (63 more sums) and this
 * call evaluates it on the host — no pass over the cloud, no device round trip.  Robust kernels (not quadratic) and calls after
 * sga_linearize_async run the error kernel.  Every factor has a fixed matrix per pair once the correspondence is frozen (GICP its cached
 * mahalanobis, PLANE_ICP diag(n * n) of the matched target normal — also the normal of a flat map's slot, ICP I), so the model serves every
 * (factor, target) combination sga_linearize accepts. */
int sga_error(sga_context* ctx, sga_problem* problem, const sga_factor_params* params, const double T[16], double* e);
/* Enqueue-only forms for multi-GPU: results stay in device memory so they can be all-reduced (RCCL) on the same stream before
 * the host reads them.  d_out30: [0..20] upper triangle of H row-wise, [21..26] b, [27] e, [28] num_inliers (as double), [29] 0.
 * d_out1: e.  Both must be device pointers valid on the context's device; no host synchronisation is performed. */
#define SGA_ACCUM_DOUBLES 30
int sga_linearize_async(sga_context* ctx, sga_problem* problem, const sga_factor_params* params, const double T[16], double* d_out30);
int sga_error_async(sga_context* ctx, sga_problem* problem, const sga_factor_params* params, const double T[16], double* d_out1);
/* Native multi-GPU form: give the context an RCCL communicator over the ranks that share ONE registration (source sharded, target
 * replicated).  From then on sga_linearize / sga_error / sga_align all-reduce their accumulators over the ranks on the context's
 * stream before reading them back, so every rank returns the system of the whole source cloud.  Rank 0 creates the 128-byte id
 * and hands it to the others out of band (MPI, torch.distributed, a file).  librccl is bound with dlopen on first use. */
int sga_comm_unique_id(unsigned char id[128]);
int sga_comm_init(sga_context* ctx, int nranks, int rank, const unsigned char id[128]);
int sga_comm_destroy(sga_context* ctx);
/* The same protocol with the sum over ranks supplied by the caller: wherever the RCCL form runs ncclAllReduce (same place in the
 * stream order: behind the row reduction, before the result is handed to the host), the library copies the accumulator to the host,
 * calls fn(user, values, count) — which must replace values[0..count) by their sum over all ranks (MPI_Allreduce, gloo, a pipe) and
 * return 0 — and copies the sums back.  For transports other than RCCL, and for running the N-rank code path on a single device
 * (tests/test_distributed_gpu.py).  count is 96 (system + error-model moments) or 30 / 1 (robust factors). */
typedef int (*sga_allreduce_fn)(void* user, double* values, size_t count);
int sga_comm_init_callback(sga_context* ctx, int nranks, int rank, sga_allreduce_fn fn, void* user);
/* Host only (no device): the error at trial pose T from the 96-double accumulator of a linearization at T_lin — what sga_error answers
 * from after sga_linearize.  acc96: [0, 30) the system (SGA_ACCUM_DOUBLES layout), [32, 95) the moments sum p_a g (9), sum p_a M' (18),
 * sum p_a p_b M' (36) with M' = R^T M R, g = R^T M r in the source frame; sums over ranks of such accumulators are
 * accumulators. */
#define SGA_MODEL_DOUBLES 96
int sga_error_model_eval(const double acc96[SGA_MODEL_DOUBLES], const double T_lin[16], const double T[16], double* e);
/* Expand a 30-double accumulator (host memory) into H[36], b[6], e, num_inliers. */
void sga_unpack_accumulator(const double acc30[SGA_ACCUM_DOUBLES], double H[36], double b[6], double* e, uint64_t* num_inliers);
/* A custom CorrespondenceRejector on the host (registration/rejector.hpp:11-28 is a duck-typed functor `bool operator()(target, source, T,
 * target_index, source_index, sq_dist)`, true = reject).  Batch form: once per linearization the callback receives, for every source
 * point in the caller's order, the index of its nearest target point (caller's target order, -1 = the target is empty) and the
 * squared distance, and fills reject[i] (1 = reject).  While a callback is set the search is unbounded and params->max_dist_sq is
 * ignored, exactly as with a user-supplied rejector type in the reference.  Costs a device->host->device round trip per
 * linearization: a correctness path, not a fast one.  fn = NULL restores the built-in DistanceRejector / NullRejector.  kd-tree targets. */
typedef int (*sga_rejector_fn)(void* user, const double T[16], size_t n, const int64_t* target_index, const float* sq_dist, unsigned char* reject);
int sga_problem_set_rejector(sga_problem* problem, sga_rejector_fn fn, void* user);
/* Factor::linearize per source point, as the reference's Python binding exposes it (src/python/factors.cpp:52-101; gicp_factor.hpp:35-73,
 * icp_factor.hpp:20-54, plane_icp_factor.hpp:19-57): runs one linearization at T, then returns for every source point (caller's order)
 * values28 n*28 doubles = [0..20] upper triangle of H_i row-wise, [21..26] b_i, [27] e_i, and inlier n bytes (0: no correspondence, all
 * values 0).  kd-tree targets and flat voxel maps; the pairs are the correspondences of that linearization (sga_problem_get_factors
 * afterwards), a host rejector's verdicts included; per-pair arithmetic in fp64.  A diagnostic / binding entry point, not the hot path. */
int sga_linearize_per_point(sga_context* ctx, sga_problem* problem, const sga_factor_params* params, const double T[16], double* values28, unsigned char* inlier);
/* Factor state in the caller's source order: target_index n int64 (-1 = outlier; voxel id for voxel maps), mahalanobis6 n*6 floats (GICP only). */
int sga_problem_get_factors(sga_context* ctx, const sga_problem* problem, int64_t* target_index, float* mahalanobis6);
/* Stream-ordered mode (default off): sga_index_build_kdtree and sga_estimate_normals_covariances return as soon as their kernels are
 * enqueued on the context's stream instead of waiting for them (a 15k-point odometry scan spends a fifth of its time in such waits).
 * Later calls on the SAME context see their results in stream order; before their outputs are used from another context / stream,
 * call sga_context_synchronize.  Errors of the enqueued kernels are reported by the next synchronising call. */
int sga_context_set_stream_ordered(sga_context* ctx, int enabled);
/* Average device time (ms) of the linearize / error kernel chains measured with HIP events on the context's stream (0 if profiling
 * off).  enabled = 0: off; 1: every pass is bracketed with events; N > 1: every N-th pass (an event record costs microseconds). */
int sga_context_set_profiling(sga_context* ctx, int enabled);
int sga_context_get_kernel_ms(sga_context* ctx, double* linearize_ms, uint64_t* linearize_calls, double* error_ms, uint64_t* error_calls);
/* The part of a COLD pass's time spent in the nearest-neighbour search kernel (the rest: factor evaluation + block reduction). */
int sga_context_get_search_ms(sga_context* ctx, double* search_ms, uint64_t* search_calls);
/* Sharded contexts (sga_comm_init*): average time (ms) of the timed passes between the end of the row reduction and the end of the all-reduce
 * of the accumulator on the context's stream — the time inside the collective, incl. waiting for the slowest rank. */
int sga_context_get_comm_ms(sga_context* ctx, double* comm_ms, uint64_t* comm_calls);
/* linearize_ms split by kind of pass against a kd-tree.  cold = the exact nearest-neighbour walk (kdtree.hpp:193-233) for every source
 * point; warm = the neighbour of the previous linearization is kept wherever it is certified still exact (its exclusion radius minus
 * the point's motion since, triangle inequality) and only the other points walk.  Same results either way, bit for bit in the
 * correspondences.  warm_search_ms: the part of warm_ms spent in the search kernel. */
int sga_context_get_pass_ms(sga_context* ctx, double* cold_ms, uint64_t* cold_calls, double* warm_ms, uint64_t* warm_calls, double* warm_search_ms);
/* A pass runs warm while no source point can have moved farther than warm_delta_m metres since the previous linearization (default
 * 0.1; negative: never, i.e. every pass walks in full).  Process-wide; results do not depend on it, only speed does. */
void sga_set_warm_limit(double warm_delta_m);
/* 0: sga_error always runs the error kernel (the reference's literal procedure; tests compare the two). Default 1. */
void sga_set_error_model(int enabled);
/* Which nearest-neighbour kernel the linearization runs (results do not depend on it; tests compare the two): 1 = the queue-fed
 * kernel (a wave owns chunk_tiles x 64 source points and refills its lanes from a queue), 0 = one query per lane, 2 (default) =
 * queue-fed for warm passes after a small motion, one query per lane otherwise.  chunk_tiles_* <= 0 keep the current value (4 / 4). */
void sga_set_search_mode(int queue, int chunk_tiles_cold, int chunk_tiles_warm);
double sga_get_warm_limit(void);
/* Passes of each kind since the problem was created, and the number of source points that had to walk in the warm passes. */
int sga_problem_get_pass_stats(sga_context* ctx, const sga_problem* problem, uint64_t* cold_passes, uint64_t* warm_passes, uint64_t* walked_points);

/* ---- the driver: Registration<>::align + optimizers (registration/registration.hpp:33-54, optimizer.hpp:24-149) -------- */
typedef struct sga_registration_setting {
  sga_factor_params factor;  /* PointFactor + CorrespondenceRejector */
  int optimizer;             /* sga_optimizer_kind */
  int max_iterations;        /* optimizer.hpp: 20 */
  int max_inner_iterations;  /* LM: 10 */
  double init_lambda;        /* LM: 1e-3 */
  double lambda_factor;      /* LM: 10 */
  double gn_lambda;          /* GN: 1e-6 */
  double translation_eps;    /* termination_criteria.hpp: 1e-3 */
  double rotation_eps;       /* 0.1 deg in rad */
  int verbose;
  /* general_factor.hpp:41-75 RestrictDoFFactor: if restrict_dof_lambda > 0, H += lambda * diag(|mask - 1|) */
  double restrict_dof_lambda;
  double restrict_dof_mask[6];
} sga_registration_setting;
void sga_registration_setting_default(sga_registration_setting* s);

/* registration_result.hpp:11-30, field for field */
typedef struct sga_result {
  double T_target_source[16];
  int converged;
  uint64_t iterations;
  uint64_t num_inliers;
  double H[36];
  double b[6];
  double error;
} sga_result;

/* Registration<Factor, ParallelReductionHIP>::align(target, source, target_tree, init_T): everything device-resident, LM/GN on the host. */
int sga_align(sga_context* ctx, const sga_index* target, const sga_cloud* source, const double init_T[16], const sga_registration_setting* setting, sga_result* out);
/* Same, on an existing problem (re-uses the sorted source and the factor buffers). */
int sga_align_problem(sga_context* ctx, sga_problem* problem, const double init_T[16], const sga_registration_setting* setting, sga_result* out);

/* ---- sweep registration: the pose and the twist of a RAW sweep at once ---------------------------------------
 * State: T (column-major 4x4, target <- sensor at ref_time) and twist xi (6 values, rotation first, sga_se3_exp's convention: the
 * sensor's motion per unit of time, as in sga_cloud_deskew).  Source point i with the time s_i = times[i] (a host float array in the
 * cloud's storage order; it reaches the device through the staging ring) has a pose of its own:  a_i = double(s_i) - ref_time,
 * E_i = exp(a_i xi) (evaluated without cancellation, as sga_cloud_deskew does), p'_i = E_i p_i, q_i = T p'_i.  Its pair j is the exact
 * nearest target record of float(q_i) — sga_cloud_overlap's walk, the bound widened by |q_i - float(q_i)|, the winner's distance
 * measured again in double — rejected when d^2 > max_dist_sq (max_dist_sq < 0: no rejector); a point with a non-finite coordinate or
 * time has no pair.  Per pair, in double from the fp32 records:  r = t_j - q_i,  J_T = [R_T skew(p'_i) | -R_T],
 * J_xi = J_T a_i J_l(a_i xi) with J_l(x) = sum_k ad(x)^k / (k + 1)! the left Jacobian of SE(3) (its series, cut where the terms left out
 * are below 1e-17 of J_T),  J = [J_T | J_xi];  H = sum J^T M J (12 x 12, row-major, order [pose: rx ry rz tx ty tz | twist: the same]),
 * b = sum J^T M r,  e = sum r^T M r / 2, with M = (C^t_j + (R_T R_Ei) C_i (R_T R_Ei)^T)^-1 (SGA_GICP), diag(n_j^2) (SGA_PLANE_ICP) or I
 * (SGA_ICP).  params->math_mode is not read.  The sums are formed without floating-point atomics in an order that depends on nothing
 * but n: two calls give the same bytes.  A call is TWO launches and one host wait; an empty source launches nothing and gives zeros.
 * Target: a kd-tree (voxel maps and projective searches: SGA_ERR_UNSUPPORTED); GICP needs covariances on both sides (SGA_ERR_INVALID),
 * PLANE_ICP target normals (SGA_ERR_UNSUPPORTED), as in sga_linearize.  Refusals before any handle is read: NULL arguments (nearest may
 * be NULL), a non-finite entry of T, twist or ref_time (SGA_ERR_INVALID), a robust kernel (SGA_ERR_UNSUPPORTED).  Then: another device,
 * 2^31 points or more, times in device memory, and a twist with max_i |a_i| (|omega| + |v|) > 8, where the series is not summed
 * (SGA_ERR_INVALID).
 * nearest (or NULL; room for n): the pair's ORIGINAL target index, -1 without a pair. */
int sga_sweep_linearize(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* params, const double T[16], const double twist[6], double ref_time, double H[144],
                        double b[12], double* e, uint64_t* num_inliers, int64_t* nearest /* n, or NULL */);
/* e at another state (T, twist) over the pairs — and, for GICP, the M — of the last sga_sweep_linearize of this (ctx, target, source,
 * factor kind), which the context keeps: Reduction::error for a sweep.  Two launches, one wait.  SGA_ERR_INVALID without such a
 * linearization; the other refusals are sga_sweep_linearize's. */
int sga_sweep_error(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const sga_factor_params* params, const double T[16], const double twist[6], double ref_time, double* e);
typedef struct sga_sweep_params {
  double ref_time;              /* default 1.0 */
  double twist_prior[6];        /* default 0 */
  double twist_information[36]; /* symmetric, PSD; all zero (default) = no prior */
} sga_sweep_params;
typedef struct sga_sweep_result {
  double T_target_source[16];
  double twist[6];
  int converged;
  uint64_t iterations, num_inliers;
  double H[144]; /* the last linearization, the prior included */
  double b[12];
  double error;
} sga_sweep_result;
void sga_sweep_params_default(sga_sweep_params* p); /* ref_time 1.0, no prior */
/* The loop of sga_align in 12 dimensions:  (H + lambda I) delta = -b by an LDL^T in double,  T <- T exp(delta[0:6]),
 * xi <- xi + delta[6:12];  LM (the default) takes a trial's error from sga_sweep_error and handles lambda as sga_align does, GN uses
 * gn_lambda;  converged when BOTH halves of delta meet rotation_eps / translation_eps.  The prior adds twist_information to the twist
 * block of H, twist_information (xi - twist_prior) to b and (xi - twist_prior)^T twist_information (xi - twist_prior) / 2 to e, on the
 * host.  init_T NULL: the identity; init_twist NULL: zero.  An empty source: SGA_OK with the initial state, converged = 0, nothing
 * launched.  Refusals before any handle is read: those of sga_sweep_linearize, a non-finite entry of the prior or of its information, an
 * information that is not symmetric (SGA_ERR_INVALID), restrict_dof_lambda > 0 (SGA_ERR_UNSUPPORTED). */
int sga_align_sweep(sga_context* ctx, const sga_index* target, const sga_cloud* source, const float* times, const double init_T[16] /* or NULL */, const double init_twist[6] /* or NULL */,
                    const sga_registration_setting* setting, const sga_sweep_params* sweep_params, sga_sweep_result* out);

/* ---- several independent registrations in one chain of launches ---------------------------------------------------------------------
 * A batch pairs `count` existing problems of ONE context (it borrows them: the caller keeps ownership and destroys the batch first).
 * One linearization of the batch is ONE search + factor launch over the tiles of all its active pairs, ONE row reduction and ONE
 * hand-off to the host, whatever `count` is: the throughput form for many small clouds (a 11k-point scan fills 2 % of an MI355X).
 * Every pair has its own pose and its own device frames; its sums do not depend on the company it keeps, bit for bit.
 * Scope: the members' targets are ALL kd-trees, ALL Gaussian voxel maps (VGICP) or ALL flat maps — one-shot, incremental or created from
 * host voxels, any mix of leaf sizes, search offsets and flat contents, and one map may be the target of several members; a batch that
 * mixes the kinds, or holds a projective index, is SGA_ERR_UNSUPPORTED at creation.  A map batch runs one factor launch (the lookup
 * inside it) instead of the search + factor launch.  One factor kind per call (ICP, PLANE_ICP, GICP; against maps as the lone path takes
 * them: PLANE_ICP needs a flat map with normals, GICP covariances on both sides — refused with the lone path's status), distance or null
 * rejector; SGA_MATH_FP32, SGA_ROBUST_NONE, the error model on (sga_set_error_model) and no host
 * rejector on any member — otherwise SGA_ERR_UNSUPPORTED before any device work.  count == 0 is SGA_OK and does nothing.  A problem
 * is in one batch at a time and is not used through the lone entry points while a batch call runs; after a batch call it holds what a
 * lone pass at the same pose leaves (sga_problem_get_factors, sga_linearize_per_point, sga_error keep working on it). */
typedef struct sga_batch sga_batch;
int sga_batch_create(sga_context* ctx, sga_problem* const* problems, size_t count, sga_batch** out);
int sga_batch_destroy(sga_batch* batch);
int sga_batch_size(const sga_batch* batch, size_t* count);
/* Reduction::linearize (reduction_omp.hpp:24-58) for every pair with active[k] != 0 (active == NULL: all).  T: count x 16, H: count x 36,
 * b: count x 6, e / num_inliers (may be NULL): count.  Entries of inactive pairs are left untouched. */
int sga_batch_linearize(sga_context* ctx, sga_batch* batch, const sga_factor_params* params, const double* T, const unsigned char* active, double* H, double* b, double* e, uint64_t* num_inliers);
/* Registration<>::align (registration.hpp:33-54) for every pair, LM or GN on the host in lock-step rounds: a round linearizes the pairs
 * that are not done, each then runs its LM inner loop against its error model.  init_T: count x 16 or NULL (identity); out: count.
 * Per pair the result is that of the same loop run on the pair alone; like sga_align_problem, no search state of earlier calls is used. */
int sga_align_batch(sga_context* ctx, sga_batch* batch, const double* init_T, const sga_registration_setting* setting, sga_result* out);
/* The host loop alone over caller-supplied batched reductions (the batched form of sga_optimize, no device involved): each callback
 * serves the pairs with active[k] != 0 (T: count x 16 and the outputs laid out as above, entries of the others untouched) and returns 0
 * on success.  For every pair the sequence of linearize / error requests and the sga_result are exactly those of sga_optimize run on
 * that pair alone; verbose lines carry the pair's number. */
typedef int (*sga_batch_linearize_fn)(void* user, size_t count, const unsigned char* active, const double* T, double* H, double* b, double* e, uint64_t* num_inliers);
typedef int (*sga_batch_error_fn)(void* user, size_t count, const unsigned char* active, const double* T, double* e);
int sga_optimize_batch(const sga_registration_setting* setting, size_t count, const double* init_T, sga_batch_linearize_fn linearize, sga_batch_error_fn error, void* user, sga_result* out);

/* ---- one registration over several GPUs of THIS process ------------------------------------------------------------------------
 * The single-process form of the sharded path and the analogue of ParallelReductionOMP::num_threads (registration/reduction_omp.hpp:22,72:
 * the loop over the source points, :32-58, is what gets partitioned).  Shard g owns the source points [g n / G, (g + 1) n / G) of the
 * caller's order and their factor state on device devices[g]; the target and its search index are replicated on every device.  A
 * linearization enqueues the pass on every device from the calling thread, collects the G accumulators and adds them in shard order on
 * the host (bit-reproducible; no collective, no communicator, no launcher).  The same device may be listed more than once (logical
 * shards on one GPU: how the path is tested on single-GPU machines).  Inputs use the reference's PointCloud layout like
 * sga_cloud_create_f64.  The process-per-GPU form with an RCCL all-reduce on the stream is sga_comm_init. */
typedef struct sga_multi sga_multi;
int sga_multi_create(const int* devices, int num_devices, sga_multi** out);
int sga_multi_destroy(sga_multi* m);
int sga_multi_num_devices(const sga_multi* m);
int sga_multi_set_target_f64(sga_multi* m, const double* xyzw, const double* normals4, const double* cov4x4, size_t n);
/* the same with fp32 arrays in the layout of sga_cloud_create_f32 (xyz n*3, normals n*3, cov6 n*6: xx xy xz yy yz zz) */
int sga_multi_set_target_f32(sga_multi* m, const float* xyz, const float* normals3, const float* cov6, size_t n);
int sga_multi_set_source_f32(sga_multi* m, const float* xyz, const float* normals3, const float* cov6, size_t n, const double init_T[16]);
/* the same with xyz_rel relative to `origin` (see sga_cloud_create_f32_origin): a caller that repacks double clouds subtracts in double while it repacks */
int sga_multi_set_target_f32_origin(sga_multi* m, const float* xyz_rel, const float* normals3, const float* cov6, size_t n, const double origin[3]);
int sga_multi_set_source_f32_origin(sga_multi* m, const float* xyz_rel, const float* normals3, const float* cov6, size_t n, const double origin[3], const double init_T[16]);
/* a Gaussian voxel map as the target (see sga_index_create_voxelmap_from_voxels): replicated on every device */
int sga_multi_set_target_voxels(sga_multi* m, double leaf_size, const int32_t* coords, const double* means3, const double* cov6, size_t n);
/* A custom CorrespondenceRejector for the whole registration (see sga_problem_set_rejector): the batch callback is invoked once per shard and
 * linearization with the shard's range [first, first + n) of the caller's source order; fn = NULL restores the built-in rejectors. */
typedef int (*sga_multi_rejector_fn)(void* user, const double T[16], size_t first, size_t n, const int64_t* target_index, const float* sq_dist, unsigned char* reject);
int sga_multi_set_rejector(sga_multi* m, sga_multi_rejector_fn fn, void* user);
/* search offsets of the voxel-map target on every device (sga_voxelmap_set_search_offsets) */
int sga_multi_set_search_offsets(sga_multi* m, int num_offsets);
/* a flat voxel map as the target (see sga_index_create_flatmap_from_voxels): replicated on every device */
int sga_multi_set_target_flat_voxels(sga_multi* m, double leaf_size, const int32_t* coords, const uint32_t* counts, const double* points3, const double* cov6, int search_offsets, size_t n);
int sga_multi_set_source_f64(sga_multi* m, const double* xyzw, const double* normals4, const double* cov4x4, size_t n, const double init_T[16]);
/* Reduction::linearize / ::error over all shards (reduction_omp.hpp:24-70), Registration<>::align (registration.hpp:33-43) on the host */
int sga_multi_linearize(sga_multi* m, const sga_factor_params* params, const double T[16], double H[36], double b[6], double* e, uint64_t* num_inliers);
int sga_multi_error(sga_multi* m, const sga_factor_params* params, const double T[16], double* e);
int sga_multi_align(sga_multi* m, const double init_T[16], const sga_registration_setting* setting, sga_result* out);
/* every registration starts without search hints (sga_multi_align calls it; callers that drive linearize / error themselves call it per align) */
int sga_multi_reset_search_state(sga_multi* m);
/* factor state of the whole source in the caller's order (see sga_problem_get_factors) */
int sga_multi_get_factors(sga_multi* m, int64_t* target_index, float* mahalanobis6);

/* The optimizer alone, over user reductions (the reference's Optimizer::optimize with a pluggable Reduction, optimizer.hpp:27-36):
 * used for sharded multi-GPU runs where linearize = local kernels + all-reduce.  Callbacks return 0 on success. */
typedef int (*sga_linearize_fn)(void* user, const double T[16], double H[36], double b[6], double* e, uint64_t* num_inliers);
typedef int (*sga_error_fn)(void* user, const double T[16], double* e);
int sga_optimize(const sga_registration_setting* setting, const double init_T[16], sga_linearize_fn linearize, sga_error_fn error, void* user, sga_result* out);

/* util/lie.hpp:77-96 se3_exp (host), and its inverse for rotation angles below pi; twist = [rx ry rz tx ty tz].  Both are evaluated
 * without cancellation at small angles (csrc/lie.hpp; the optimizer multiplies by the reference's own expressions, as before). */
void sga_se3_exp(const double twist[6], double T[16]);
void sga_se3_log(const double T[16], double twist[6]);

#ifdef __cplusplus
}
#endif
#endif /* SMALL_GICP_AMD_H */

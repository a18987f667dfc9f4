/*
 * small_gicp_amd — diagnostics of the MI355X registration hot path.  NOT part of the drop-in boundary (small_gicp_amd.h): these entry
 * points expose how the searches went (for the scripts under scripts/ and for DESIGN.md's measurements), never what they returned.
 */
#ifndef SMALL_GICP_AMD_DEBUG_H
#define SMALL_GICP_AMD_DEBUG_H

#include "small_gicp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Record, for the following linearization passes of this problem, the number of kd-tree leaves each source point's search scanned
 * (source order of the engine, i.e. sorted); get returns the last pass's counts (n ints).  While enabled every pass walks the kd-tree. */
int sga_problem_set_search_stats(sga_context* ctx, sga_problem* pb, int enabled);
int sga_problem_get_search_stats(sga_context* ctx, const sga_problem* pb, int* leaves_per_point);
/* The source points in the engine's order (n x 4 floats: x, y, z, original index as bits). */
int sga_problem_get_sorted_points(sga_context* ctx, const sga_problem* pb, float* xyzw);
/* The plan of the last linearization pass of this problem (csrc/linearize.hip: PassPlan, plan_pass): out[0] = the route (enum class Route:
 * 0 factors, 1 grid, 2 certify, 3 fused lane, 4 fused queue, 5 queue, 6 lane), out[1] = warm, out[2] = the cell grid serves the pass,
 * out[3] = points per lane of the factor kernel, out[4] = that kernel also summed the rows, out[5] = tiles per wave of the queue-fed
 * kernels, out[6] = partial rows given to reduce_rows_kernel and out[7] = its workgroups (both 0 when the factor kernel summed the rows).
 * All 0 before the first pass. */
int sga_problem_get_last_plan(const sga_problem* pb, int out[8]);
/* Cell-grid passes (cell_grid.hip) since the problem was created: out[0] = passes searched through the grid, out[1] = queries their
 * first ring left open (finished by the second kernel), out[2] = sum of the rings those queries then scanned, out[3] = cell edge in
 * micrometres (0: the target has no grid); out[4], out[5]: always 0 (counters of experiments removed in round 6). */
int sga_problem_get_grid_stats(const sga_problem* pb, uint64_t out[6]);
/* What the cell grid (a second, flat search structure of large kd-tree indices) is used for; results do not depend on it (tests compare
 * the searches): mode 0 nothing (no grid is built); 1 (default) the walkers of warm passes try its first ring before they walk the tree;
 * 2 also the cold passes of a registration but its first; 3 the first pass too; 4 every pass.  min_points: targets with fewer points get
 * no grid (default 65536; applies to indices built afterwards).  Negative arguments keep the current value.
 * Environment: SGA_GRID, SGA_GRID_MIN_POINTS. */
void sga_set_grid_mode(int mode, long long min_points);
/* Normal / covariance estimation: clouds of at most max_points points search their neighbours with one wave per query (csrc/knn_wave.hpp:
 * the form for clouds that do not fill the chip), larger ones with one query per lane.  Both are exact; the tests compare them.
 * Default 81920 (environment: SGA_KNN_WAVE_MAX); 0 = never. */
void sga_set_knn_wave_max(long long max_points);
/* The length scale of a kd-tree index: the geometric mean of the diagonals of its leaf boxes (a leaf = a neighbourhood of <= 8 points),
 * computed by the build.  The pass routing of the linearization measures the source's motion in units of it (csrc/linearize.hip:
 * routing_unit), so that the choice between the exact search kernels does not depend on the unit of length or the density of the cloud.
 * 0 while the build's kernels have not run yet (the value arrives as a late note, csrc/notes.hpp) or for other kinds of index. */
int sga_index_spacing(const sga_index* index, double* spacing);
/* A kd-tree index as built: depth = D (leaves of at most 8 points); nodes = 2^D x {threshold, axis as int bits} (entry 2^d + k is node k
 * of depth d; entry 0 unused, never written); xyzw = the n points in kd order (device frame, w = original index as bits).  nodes / xyzw may be null
 * (depth only).  Other kinds of index are refused. */
int sga_debug_kd_tree(sga_context* ctx, const sga_index* index, int* depth, float* nodes, float* xyzw);
/* The bounding box of its points (device frame: the cloud's records) that the build of an index stored: a kd-tree's comes from the root
 * level of its build; all zeros for an empty index. */
int sga_debug_index_bbox(const sga_index* index, float lo[3], float hi[3]);
/* Kernels enqueued so far, in this process, by the forest form of sga_index_build_kdtree_batch and
 * sga_estimate_normals_covariances_batch (members that take the lone path inside those calls are not counted): a forest of B clouds of
 * equal depth enqueues as many kernels as a forest of one. */
int sga_debug_forest_launches(unsigned long long* launches);
/* What sga_voxelgrid_sampling(cloud, leaf) would do, decided by the very code the call itself runs (csrc/preprocess.hip: voxelgrid_plan):
 * out[0] = bytes of a sort key (4 or 8), out[1..3] = key bits of x, y, z, out[4] = their sum (the dropped-point key is 1 << total),
 * out[5] = the layout comes from the cloud's box (0: the reference's 21 / 21 / 21), out[6] = the sort's branch (csrc/sort_util.hpp:
 * sort_path, 0 up to 2048 keys, 1 up to 200 000, 2 above), out[7] = tiles (workgroups) of ds_segments_kernel, out[8] = the centroid kernel
 * is launched for n voxels before the host knows their number.  All 0 for an empty cloud (no kernel runs).  No device work. */
int sga_debug_voxelgrid_plan(const sga_cloud* cloud, double leaf, int out[9]);
/* What sga_voxelgrid_sampling_batch(clouds, count, leaf) would do, decided by the very code the call itself runs (csrc/preprocess.hip:
 * grid_forest_plan): out[0] = bytes of a composite sort key (4 or 8; 0: no member shares the chain), out[1] = W, the bits below the member
 * number (the widest member layout's total + 1), out[2] = the bits of the member number, out[3] = members of the shared chain, out[4] =
 * members that go through the lone routine (empty members are in neither), out[5] = tiles (workgroups) of the runs kernel.  No device work. */
int sga_debug_voxelgrid_batch_plan(const sga_cloud* const* clouds, size_t count, double leaf, int out[6]);
/* Launches enqueued so far, in this process, by the shared chain of sga_voxelgrid_sampling_batch: its own kernels plus one per sort call
 * (members that take the lone path inside the call are not counted): a chain of B clouds counts as many as a chain of one. */
int sga_debug_voxelgrid_batch_launches(unsigned long long* launches);
/* What sga_index_build_gaussian_voxelmap_batch(clouds, count, leaf) would do, decided by the very code the call itself runs
 * (csrc/forest.hpp: vox_forest_plan): out[0] = members of the shared chain, out[1] = members that go through the lone routine (more than
 * 262144 points, or past the chain's caps), out[2] = empty members, out[3] = the bits of the member number, out[4] = the end bit of the
 * chain's sort (49 + out[3]; 0: no chain), out[5] = points of the concatenation.  A member whose voxels span 65536 or more per axis is
 * counted in out[0]: the device finds that out.  The arguments are checked as the call checks them.  No device work. */
int sga_debug_voxelmap_batch_plan(const sga_cloud* const* clouds, size_t count, double leaf, int out[6]);
/* Launches enqueued so far, in this process, by the shared chain of sga_index_build_gaussian_voxelmap_batch: its kernels, one per sort
 * and scan call, and its copy commands (members that take the lone path inside the call are not counted): a chain of B clouds counts as
 * many as a chain of one. */
int sga_debug_voxelmap_batch_launches(unsigned long long* launches);
/* What sga_voxelmap_insert_batch(maps, clouds, count) would do, decided by the very code the call itself runs (csrc/forest.hpp:
 * ivm_forest_plan): out[0] = members of the shared chain, out[1] = members that go through the lone routine (flat maps, more than 262144
 * points, past the chain's caps), out[2] = Gaussian maps with an empty cloud, out[3] = the bits of the member number, out[4] = the end bit
 * of the chain's sort (49 + out[3]; 0: no chain), out[5] = points of the concatenation.  A member whose scan spans 65536 or more voxels
 * per axis is counted in out[0]: the device finds that out.  The members are checked as the call checks them.  No device work. */
int sga_debug_voxelmap_insert_batch_plan(sga_index* const* maps, const sga_cloud* const* clouds, size_t count, int out[6]);
/* Launches enqueued so far, in this process, by the shared chain of sga_voxelmap_insert_batch: its kernels, one per sort and scan call,
 * and its table copies (growth, LRU sweeps and members that take the lone path inside the call are not counted): a round of B members
 * without growth counts as many as a round of one. */
int sga_debug_voxelmap_insert_batch_launches(unsigned long long* launches);
/* What sga_problem_create_batch(targets, sources, count) would do, decided by the very code the call itself runs (csrc/forest.hpp:
 * problem_forest_plan): out[0] = members of the shared chain, out[1] = members that go through the lone routine (a projective target,
 * more than 262144 points, past the cap of the concatenation), out[2] = members with an empty source, out[3] = points of the
 * concatenation.  The members are checked for NULL as the call checks them.  No device work. */
int sga_debug_problem_batch_plan(const sga_index* const* targets, const sga_cloud* const* sources, size_t count, int out[4]);
/* Launches enqueued so far, in this process, by the shared chain of sga_problem_create_batch: its table copy, its two kernels and its one
 * sort call (members that take the lone routine inside the call are not counted): a call of B chain members counts as many as a call of
 * one. */
int sga_debug_problem_batch_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_cloud_merge / sga_cloud_transform: per pass one table copy and one kernel, whatever
 * the number of members (a second pass only when origin == NULL chooses an origin other than zero). */
int sga_debug_cloud_merge_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_cloud_deskew / _batch / _device: per call one table copy and one kernel, whatever
 * the number of members (a call without a non-empty member: none). */
int sga_debug_cloud_deskew_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_cloud_crop / _batch / _device: per call one table copy and one kernel, whatever
 * the number of members (a call without a non-empty member: none). */
int sga_debug_cloud_crop_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_cloud_remove_outliers: per call the statistic, the threshold (statistical mode; radius
 * mode only when stats are asked for), the compaction's table copy and the compaction — at most four whatever the cloud's size.  The build
 * of a temporary tree is not counted here; an empty cloud enqueues nothing. */
int sga_debug_cloud_outliers_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_cloud_overlap: per call the distances and the sums — two for a statistics-only call —
 * and, when a cloud is made, the compaction's table copy and the compaction: four, whatever the cloud's size and the kind of target.  An
 * empty cloud enqueues nothing.  (The compaction of an overlap call is counted here, not by sga_debug_cloud_outliers_launches.) */
int sga_debug_cloud_overlap_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_sweep_linearize, sga_sweep_error and sga_align_sweep: two per pass (the pass kernel
 * and the sum of its rows), whatever the cloud's size; an empty source and a refused call enqueue nothing. */
int sga_debug_sweep_launches(unsigned long long* launches);
/* Launches enqueued so far, in this process, by sga_voxelgrid_sampling_fields and its device form: per call the keys, the sort (counted
 * as one), the runs and the one launch that writes centroids, columns, counts and voxel_of — four; three when a cloud above the
 * speculative limit has no voxel and no voxel_of is asked for; none for an empty cloud and for a refused call. */
int sga_debug_voxelgrid_fields_launches(unsigned long long* launches);
/* Commands enqueued so far, in this process, by sga_cloud_visibility: per call the fill that clears the range image, the image kernel
 * (none for an empty scan), the states and the counts — four for a statistics-only call, three with an empty scan — and, when a cloud is
 * made, the compaction's table copy and the compaction: six / five.  An empty map enqueues nothing, unless the range image is asked for:
 * then the fill, the image kernel (none for an empty scan) and the export, three / two. */
int sga_debug_cloud_visibility_launches(unsigned long long* launches);
/* Commands enqueued so far, in this process, by the three calls of the global registration (small_gicp_amd.h):
 * sga_cloud_fpfh three per call (the neighbour lists, the SPFH counts, the FPFH rows; one fill for a cloud of one point, none for an empty one),
 * sga_features_match two (three with mutual; none when either side is empty), sga_ransac_correspondences four (the pairs' points, the
 * fill of the best word, the hypotheses, the refit sums; none for M < 3).  The build of a temporary tree is not counted. */
int sga_debug_cloud_fpfh_launches(unsigned long long* launches);
int sga_debug_features_match_launches(unsigned long long* launches);
int sga_debug_ransac_launches(unsigned long long* launches);
/* Commands enqueued so far, in this process, by the place-recognition calls (small_gicp_amd.h).  add: what
 * sga_places_add (three: the fill of the slot, the descriptor, the column norms; one for an empty cloud), sga_places_add_descriptor (one)
 * and sga_cloud_scan_context (three; two for an empty cloud) enqueue, plus one copy whenever the database grows.  query: what
 * sga_places_query (four: fill, descriptor, match, selection; three for an empty cloud) and sga_places_query_descriptor (two) enqueue;
 * none over zero candidates.  waits: the host waits of all these calls (a query: one; an add on a stream-ordered context: none). */
int sga_debug_places_add_launches(unsigned long long* launches);
int sga_debug_places_query_launches(unsigned long long* launches);
int sga_debug_places_waits(unsigned long long* waits);
/* Commands enqueued so far, in this process, by the fixed-radius calls (small_gicp_amd.h).
 * sga_index_radius_search: the count and the prefix — two — and with lists that fit the fill and two copies: five.  sga_cloud_cluster: the
 * fill of its tables, the hook, the flatten, the sizes, the selection and the labels — six — plus the count and the border pass when
 * min_points > 1 — eight — plus the compaction's table copy and the compaction when a cloud is made.  The build of a temporary tree is not
 * counted; an empty cloud / no queries enqueue nothing.  waits: the host waits of both (a clustering: one; a search: one, two with lists). */
int sga_debug_radius_search_launches(unsigned long long* launches);
int sga_debug_cloud_cluster_launches(unsigned long long* launches);
int sga_debug_radius_waits(unsigned long long* waits);
/* Commands enqueued so far, in this process, by sga_cloud_segment_plane (small_gicp_amd.h): the hypotheses, the
 * scores, the selection and the sums — four — plus the flags when the refit succeeded or a cloud is made — five — plus the compaction's
 * table copy and the compaction when a cloud is made — seven.  Nothing for n < 3 but the compaction's two with keep 2 and n >= 1.  waits:
 * its host waits — one behind the sums, a second one (the compaction's, or a synchronisation) whenever the flags kernel ran; when no
 * plane is found, the one behind the sums and the compaction's with keep 2. */
int sga_debug_segment_plane_launches(unsigned long long* launches);
int sga_debug_segment_plane_waits(unsigned long long* waits);
/* Commands enqueued so far, in this process, by sga_cloud_iss_keypoints (small_gicp_amd.h): the saliencies and
 * the suppression — two — plus the listing kernel without a cloud — three — or the compaction's table copy and the compaction with
 * one — four.  The build of a temporary tree is not counted; an empty cloud enqueues nothing.  waits: its host waits, one per call. */
int sga_debug_iss_launches(unsigned long long* launches);
int sga_debug_iss_waits(unsigned long long* waits);
/* Commands enqueued so far, in this process, by the occupancy grid's calls (small_gicp_amd.h): sga_occupancy_create
 * two fills, clear one; integrate two launches (one with mode 1; none for an empty scan or a box out of reach); classify one, plus the
 * compaction's table copy and launch with an output cloud; stats one; export one, plus two when it fills.  waits: their host waits —
 * integrate none (one with stats), classify one, stats one, export one or two, download one per 2^20 cells. */
int sga_debug_occupancy_launches(unsigned long long* launches);
int sga_debug_occupancy_waits(unsigned long long* waits);
/* The host arithmetic of sga_cloud_segment_plane's refit, exposed so that it can be tested without a device: from k, sum x and sum x x^T
 * (sum_xx6 = xx, xy, xz, yy, yz, zz) of the inliers' differences x from an anchor: centroid_offset = sum x / k, eigenvalues (ascending)
 * of S = sum x x^T - (sum x)(sum x)^T / k, and normal = the unit eigenvector of the smallest, with the first non-zero of (z, y, x)
 * positive.  Returns 1, or 0 when there is no refit: k < 3, a non-finite sum, or lambda_1 - lambda_0 <= 1e-12 lambda_2 (then normal is
 * untouched; centroid_offset and eigenvalues are written when k >= 1 and the sums are finite). */
int sga_debug_plane_from_sums(uint64_t k, const double sum_x[3], const double sum_xx6[6], double normal[3], double centroid_offset[3], double eigenvalues[3]);
/* The host arithmetic of sga_ransac_correspondences, exposed so that it can be tested without a device.  draw: the three distinct pair
 * numbers hypothesis h draws from M >= 3 pairs under `seed` (SGA_ERR_INVALID for M < 3 or M >= 2^31).  rigid_from_sums: the least-squares
 * rigid motion of n point pairs from their plain sums — sum_s = sum p_s, sum_t = sum p_t, cross[3 r + c] = sum p_s[r] p_t[c] — by Horn's
 * quaternion form over a Jacobi eigen-solver; T column-major 4x4.  Returns 1 and writes T, or 0 with T untouched when n < 3 or the
 * centred cross-covariance has rank < 2 (its second singular value is below 1e-12 of the first). */
int sga_debug_ransac_draw(uint64_t seed, uint64_t h, uint64_t M, uint64_t out[3]);
int sga_debug_rigid_from_sums(uint64_t n, const double sum_s[3], const double sum_t[3], const double cross[9], double T[16]);
/* The bounding box of its finite records (device frame) that a cloud carries, when its producer knew it (uploads, sga_cloud_merge; the
 * voxel grid sorts short keys with it): *has_box = 0 and zeros when it carries none. */
int sga_debug_cloud_box(const sga_cloud* cloud, int* has_box, float lo[3], float hi[3]);
/* Sets the launch epoch of the context's voxel-grid calls (the tag of ds_segments_kernel's status words; the next call uses epoch + 1, and
 * a call that finds 2^30 - 1 clears the words and starts again at 1) so that a test reaches the wrap-around a service meets after 2^30
 * calls.  Forwards only: an epoch below the current one, or above 2^30 - 1, is refused (words of earlier launches would read as current). */
int sga_debug_set_voxelgrid_epoch(sga_context* ctx, unsigned epoch);
/* GPU time (HIP events) between two points of the context's stream: start() records an event, stop() records another, waits for it and
 * returns the milliseconds in between — the kernel times of bench.py's per-stage roofline lines (voxel grid, index build, covariances). */
int sga_debug_timer_start(sga_context* ctx);
int sga_debug_timer_stop(sga_context* ctx, double* ms);
/* The host arithmetic of the frame check of sharded registrations (csrc/frames.hip: problem_check_shard_frames), exposed so that it can be
 * tested without a device: pack() turns a source origin into the SGA_FRAME_CHECK_DOUBLES values a rank contributes to the all-reduce,
 * agree() says whether the ranks whose contributions were summed all named the same origin (exact for any origin, up to 1024 ranks). */
#define SGA_FRAME_CHECK_DOUBLES 32
void sga_debug_shard_frame_pack(const double origin[3], double out[SGA_FRAME_CHECK_DOUBLES]);
int sga_debug_shard_frame_agree(const double sum[SGA_FRAME_CHECK_DOUBLES]);
/* The row sum that ends a linearization pass, on rows given by the caller: uploads `nrows` rows of 96 doubles and adds them exactly as a
 * pass does (csrc/reduce_rows.hpp: launch_reduce over the 95 columns of a row, reduce_groups(nrows) workgroups, fixed summation order, the
 * result handed to the host through the pinned block); derive != 0 fills the derived columns in from the totals as a pass does.
 * out = 96 doubles (column 95 is 0).  For tests of the summation order and for the clock stamps below. */
int sga_debug_reduce_rows(sga_context* ctx, const double* rows, int nrows, int derive, double* out);
/* Diagnostics build only (make stamps): the 100 MHz clock at six points of the last reduce_rows_kernel (entry, end of stage 1, after the
 * ticket, end of stage 2, after the host stores, after the system fence) from the first workgroup (out[0..5]), the last (out[8..13]) and
 * the one that finished the sum (out[16..21]; out[22] its index, out[23] the number of workgroups). */
int sga_debug_reduce_stamps(unsigned long long* out24);
/* Diagnostics build only (make trips): loop-trip counters of the kd walk and the start / end clock of every search wave. */
int sga_debug_kd_trips(unsigned long long* out16);
int sga_debug_kd_wave_times(unsigned long long* out, int waves);

#ifdef __cplusplus
}
#endif
#endif /* SMALL_GICP_AMD_DEBUG_H */

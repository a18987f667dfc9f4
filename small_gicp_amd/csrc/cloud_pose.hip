// Clouds posed on the device: posed clouds joined into one (sga_cloud_merge / _transform) and sweeps deskewed with
// a pose per point (sga_cloud_deskew / _batch / _device).  One table and ONE launch over the members each.
#include "cloud_box.hpp"
#include "device_io.hpp"
#include "forest.hpp"
#include "lie.hpp"
#include "voxel_steps.hpp"
#include "notes.hpp"

#include <cmath>
#include <memory>

namespace sga {

// What a pose does to one record, stated once for merge_cloud_kernel and deskew_cloud_kernel: the point R r + t (posed_point,
// voxel_steps.hpp), the normal R n and the covariance R C R^T are evaluated in double from the fp32 records, with the insert kernels'
// expressions (voxelmap.hip: fvm_update_kernel, ivm_update_kernel), and rounded once.
__device__ __forceinline__ float4 posed_normal_record(const Pose12& T, const float4 q) {
  double N[3];
#pragma unroll
  for (int a = 0; a < 3; a++) N[a] = T.r[3 * a] * q.x + T.r[3 * a + 1] * q.y + T.r[3 * a + 2] * q.z;
  return make_float4(static_cast<float>(N[0]), static_cast<float>(N[1]), static_cast<float>(N[2]), 0.f);
}
__device__ __forceinline__ void posed_cov_record(const Pose12& T, const Cov8* __restrict__ in, Cov8* __restrict__ out) {
  const float4* cin = reinterpret_cast<const float4*>(in);
  const float4 c0 = cin[0], c1 = cin[1];  // xx xy xz yy | yz zz 0 0
  const double Cm[3][3] = {{c0.x, c0.y, c0.z}, {c0.y, c0.w, c1.x}, {c0.z, c1.x, c1.y}};
  double RC[3][3], C6[6];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = 0; b < 3; b++) RC[a][b] = T.r[3 * a] * Cm[0][b] + T.r[3 * a + 1] * Cm[1][b] + T.r[3 * a + 2] * Cm[2][b];
  int k = 0;
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int b = a; b < 3; b++) C6[k++] = RC[a][0] * T.r[3 * b] + RC[a][1] * T.r[3 * b + 1] + RC[a][2] * T.r[3 * b + 2];
  float4* cout = reinterpret_cast<float4*>(out);
  cout[0] = make_float4(static_cast<float>(C6[0]), static_cast<float>(C6[1]), static_cast<float>(C6[2]), static_cast<float>(C6[3]));
  cout[1] = make_float4(static_cast<float>(C6[4]), static_cast<float>(C6[5]), 0.f, 0.f);
}

// One member of a merge (read with scalar loads): its records, its pose with the offset between the two device
// frames folded in — t = (R o_m + t_m) - o, formed on the host in double — and its stretch of the output.
struct MergeMember {
  const float4* pts;
  const float4* nrm;  // read only when the output keeps the attribute
  const Cov8* cov;
  Pose12 T;
  uint32_t n, off;
};
static_assert(sizeof(MergeMember) % 8 == 0, "the table is copied in 8-byte words");

// Posed clouds -> one cloud: workgroup b moves 256 points of the member m with prefix[m] <= b < prefix[m + 1] to their place in the
// concatenation, each record posed by the member's pose (above); w is the point's index in the output.  box != null: the
// bounding box of the posed points that are finite, taken BEFORE the rounding (which is monotone: the rounded box bounds the records
// exactly), leaves as a note in payload words 1..6 (box64_reduce_publish).
__global__ __launch_bounds__(kIoBlock) void merge_cloud_kernel(const MergeMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, float4* __restrict__ opts, float4* __restrict__ onrm, Cov8* __restrict__ ocov,
                                                               unsigned long long* __restrict__ box, unsigned long long* __restrict__ note_slot, unsigned long long seq) {
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const MergeMember& g = *uniform_const(members + m);
  const uint32_t i = (blockIdx.x - prefix[m]) * static_cast<uint32_t>(kIoBlock) + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < g.n) {
    const Pose12& T = g.T;
    const uint32_t j = g.off + i;
    double x, y, z;
    posed_point(T, g.pts[i], x, y, z);
    opts[j] = make_float4(static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), __uint_as_float(j));
    if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0) lo[0] = hi[0] = x, lo[1] = hi[1] = y, lo[2] = hi[2] = z;  // a non-finite point stays out of the box
    if (onrm != nullptr) onrm[j] = posed_normal_record(T, g.nrm[i]);
    if (ocov != nullptr) posed_cov_record(T, g.cov + i, ocov + j);
  }
  if (box == nullptr) return;  // (uniform)
  box64_reduce_publish(lo, hi, box, note_slot, seq);
}

// One member of a deskew (read with scalar loads): its records and where they go, its times, what its twist
// and its origin contribute to every point's pose (lie.hpp), and where its box is reduced and handed over.
struct DeskewMember {
  const float4* pts;
  const float4* nrm;  // or null
  const Cov8* cov;
  float4* opts;
  float4* onrm;
  Cov8* ocov;
  const void* times;         // float or double (tf64), tstride elements apart: device memory, or pinned host memory by its device address
  unsigned long long* acc;   // {min x y z, max x y z (encoded), arrival counter, 0} in the call's table (cloud_box.hpp: MemberBoxes); null: no box
  unsigned long long* slot;  // the member's slot of the context's box block (pinned, device-mapped; cloud_ops.hpp: kBoxSlotLo)
  double ref_time;
  TwistConst c;
  uint32_t n, blocks;
  int tstride, tf64;
};
static_assert(sizeof(DeskewMember) % 8 == 0, "the table is copied in 8-byte words");

// Sweeps -> sweeps as seen from the sensor frame at ref_time: workgroup b takes 256 points of the member m with prefix[m] <= b <
// prefix[m + 1]; point i gets the pose exp((s_i - ref_time) xi) — in double, from the member's constants, with no cancellation for any
// angle (lie.hpp) — and is posed as a member of a merge is.  w is the index.  A non-finite time makes every entry of the pose a NaN.
// g.acc != null: the box of the member's finite unrounded points is joined in its accumulator; the member's last workgroup writes it into
// the member's words of the box block, and the last member to arrive publishes the call's sequence number (forest_box_arrive).
__global__ __launch_bounds__(kIoBlock) void deskew_cloud_kernel(const DeskewMember* __restrict__ members, const uint32_t* __restrict__ prefix_g, int count, const ForestBoxes hand) {
  __shared__ bool sh_last;
  const uint32_t* prefix = uniform_const(prefix_g);
  const int m = forest_member_of(prefix, count, blockIdx.x);
  const DeskewMember& g = *uniform_const(members + m);
  const uint32_t i = (blockIdx.x - prefix[m]) * static_cast<uint32_t>(kIoBlock) + threadIdx.x;
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < g.n) {
    const size_t ti = static_cast<size_t>(i) * static_cast<size_t>(g.tstride);
    const double s = g.tf64 ? static_cast<const double*>(g.times)[ti] : static_cast<double>(static_cast<const float*>(g.times)[ti]);
    Pose12 T;
    twist_pose(g.c, s - g.ref_time, T.r, T.t);
    double x, y, z;
    posed_point(T, g.pts[i], x, y, z);
    g.opts[i] = make_float4(static_cast<float>(x), static_cast<float>(y), static_cast<float>(z), __uint_as_float(i));
    if (x - x == 0.0 && y - y == 0.0 && z - z == 0.0) lo[0] = hi[0] = x, lo[1] = hi[1] = y, lo[2] = hi[2] = z;  // a non-finite point stays out of the box
    if (g.onrm != nullptr) g.onrm[i] = posed_normal_record(T, g.nrm[i]);
    if (g.ocov != nullptr) posed_cov_record(T, g.cov + i, g.ocov + i);
  }
  if (g.acc == nullptr) return;  // (uniform: a call has boxes for all members or for none)
  box64_reduce_block(lo, hi, g.acc);
  if (threadIdx.x == 0) sh_last = __hip_atomic_fetch_add(&g.acc[6], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == g.blocks - 1u;
  __syncthreads();
  if (!sh_last) return;  // workgroup-uniform
  if (threadIdx.x < 6) g.slot[kBoxSlotLo + threadIdx.x] = __hip_atomic_load(&g.acc[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) forest_box_arrive(hand);
}

namespace {

// ---- sga_cloud_merge -----------------------------------------------------------------------------------------

// Member m's pose for an output frame at `o`: R as given (column-major T16, null: the identity), t = c - o with c = R o_m + t_m the
// member's origin in the caller's frame.  Every product and sum is rounded on its own, in the order written (no contraction): the
// offset is a function of the inputs alone, and c - o — the form of pose_to_device — is formed ONCE here, so a merge far from the origin
// cancels nothing on the device.
Pose12 merge_pose(const double* T16, const double o_m[3], const double o[3]) {
#pragma clang fp contract(off)
  Pose12 T;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T.r[3 * r + c] = T16 ? T16[4 * c + r] : (r == c ? 1.0 : 0.0);
    const double t = T16 ? T16[12 + r] : 0.0;
    const double c = ((T.r[3 * r] * o_m[0] + T.r[3 * r + 1] * o_m[1]) + T.r[3 * r + 2] * o_m[2]) + t;
    T.t[r] = c - o[r];
  }
  return T;
}

// One pass over the non-empty members `live`: the table ([members][prefix of the grid: live + 1]) and ONE launch over the concatenation.  want_box: the box of the finite posed points, relative to o,
// arrives as a note the call waits for (lo > hi: no finite point).
int merge_pass(sga_context* ctx, const sga_cloud* const* clouds, const double* T, const std::vector<size_t>& live, const double o[3], sga_cloud* c, bool want_box, DevBuf<unsigned long long>& table, double lo[3], double hi[3]) {
  const size_t count = live.size();
  std::vector<MergeMember> members(count);
  std::vector<uint32_t> prefix(count + 1, 0u);
  uint32_t off = 0;
  for (size_t j = 0; j < count; j++) {
    const size_t k = live[j];
    MergeMember& g = members[j];
    std::memset(&g, 0, sizeof(g));
    g.pts = clouds[k]->pts.p;
    g.nrm = c->has_normals ? clouds[k]->nrm.p : nullptr;
    g.cov = c->has_covs ? clouds[k]->cov.p : nullptr;
    g.T = merge_pose(T ? T + 16 * k : nullptr, clouds[k]->origin, o);
    g.n = static_cast<uint32_t>(clouds[k]->n);
    g.off = off;
    off += g.n;
    prefix[j + 1] = prefix[j] + (g.n + kIoBlock - 1u) / kIoBlock;
  }
  const uint32_t* d_prefix = nullptr;
  count_launch(Chain::Merge);
  SGA_TRY(upload_entries(ctx, table, members, prefix, &d_prefix));
  unsigned long long* note = nullptr;
  const unsigned long long seq = want_box ? note_begin(ctx, &note) : 0ull;
  count_launch(Chain::Merge);
  hipLaunchKernelGGL(merge_cloud_kernel, dim3(prefix[count]), dim3(kIoBlock), 0, ctx->stream, reinterpret_cast<const MergeMember*>(table.p), d_prefix, static_cast<int>(count), c->pts.p, c->nrm.p, c->cov.p,
                     want_box ? ctx->d_box64.p : nullptr, note, seq);
  SGA_HIP(hipGetLastError());
  if (want_box) {
    unsigned long long payload[kNoteWords - 1];
    SGA_TRY(note_wait(ctx, seq, payload));
    for (int k = 0; k < 3; k++) lo[k] = box_dec64(payload[k]), hi[k] = box_dec64(payload[3 + k]);
  }
  return SGA_OK;
}

int cloud_merge(sga_context* ctx, const sga_cloud* const* clouds, const double* T, size_t count, const double origin[3], sga_cloud** out) {
  if (out) *out = nullptr;  // on any failure *out is NULL
  if (!ctx || !out || (count > 0 && !clouds)) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(cloud_members_args(clouds, count));
  for (size_t k = 0; T != nullptr && k < count; k++)
    for (int e = 0; e < 16; e++)
      if (!(T[16 * k + e] - T[16 * k + e] == 0.0)) return fail(SGA_ERR_INVALID, "pose %zu has a non-finite entry", k);
  for (int k = 0; origin != nullptr && k < 3; k++)
    if (!(origin[k] - origin[k] == 0.0)) return fail(SGA_ERR_INVALID, "origin has a non-finite entry");
  // ---- (from here on the handles are read)
  CloudMembers mem;
  SGA_TRY(cloud_members(ctx, clouds, count, kIoBlock, &mem));
  const std::vector<size_t>& live = mem.live;
  const size_t total = mem.points;
  if (total >= (1ull << 31)) return fail(SGA_ERR_INVALID, "merged cloud too large (%zu points; limit 2^31-1)", total);
  if (total > 0) SGA_HIP(hipSetDevice(ctx->device));  // (no member, or empty members only: no device work)
  StreamScope stream_scope(ctx->stream);
  std::unique_ptr<sga_cloud> c;  // an attribute is kept when every non-empty member has it; without one: no attributes
  SGA_TRY(cloud_make(ctx, origin, total, total > 0 && mem.normals, total > 0 && mem.covs, &c));
  if (total == 0) {
    *out = c.release();
    return SGA_OK;
  }
  // The box of the finite posed points.  The origin is chosen from it (origin == NULL: the one host wait the data forces); a blocking
  // context, which waits anyway, also keeps it with the cloud.  A stream-ordered context with the origin given waits for nothing and its
  // cloud carries no box — sga_cloud_create_device's contract.
  const bool want_box = origin == nullptr || !ctx->stream_ordered;
  if (want_box) SGA_TRY(ensure_box64(ctx));
  for (size_t k : live) SGA_TRY(wait_ready(ctx, clouds[k]->ready));  // made by another context in stream-ordered mode (common.hpp: Ready)
  DevBuf<unsigned long long> table, table2;  // live to the end of the call (then: the stream's free list)
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  // origin == NULL: the first pass writes the records for the origin zero, so its box IS the box of the posed points in the caller's
  // frame — the same numbers whatever follows.  An origin other than zero (a submap far from the origin: rare) takes a second pass, which
  // starts from the members' records again and brings the box of its own records.
  SGA_TRY(merge_pass(ctx, clouds, T, live, c->origin, c.get(), want_box, table, lo, hi));
  if (origin == nullptr) {
    choose_origin(lo, hi, c->origin);
    if (!origin_is_zero(c->origin)) SGA_TRY(merge_pass(ctx, clouds, T, live, c->origin, c.get(), true, table2, lo, hi));
  }
  // (a note has shown that the last launch is over; without one the context is stream-ordered)
  cloud_set_box(c.get(), lo, hi, true, false);  // the rounding is monotone: the rounded box of the unrounded records is the box of the records
  SGA_TRY(mark_ready(ctx, c->ready));
  *out = c.release();
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

// ---- sga_cloud_deskew ------------------------------------------------------------------------------------------
// Where member k's n times live: host times must not be device memory, a device array must cover the n rows it is read at
static int deskew_times_check(sga_context* ctx, size_t n, const float* times, const sga_device_array* dtimes, size_t k) {
  if (times != nullptr) {
    bool on_device = false;
    (void)pinned_device_view(times, n * sizeof(float), &on_device);
    if (on_device) return fail(SGA_ERR_INVALID, "times[%zu] is device memory: times that live on the device go through sga_cloud_deskew_device", k);
    return SGA_OK;
  }
  const size_t elem = dtimes->dtype == SGA_F64 ? 8 : 4;
  size_t span = 0;  // the last element read ends here: a column of a wider array need not own the rest of its last row
  if (__builtin_mul_overflow(n - 1, static_cast<size_t>(dtimes->stride) * elem, &span) || __builtin_add_overflow(span, elem, &span))
    return fail(SGA_ERR_INVALID, "times: %zu rows of stride %d overflow the address space", n, dtimes->stride);
  return check_device_range(ctx, dtimes->data, span, elem, "times", "sga_cloud_deskew");
}

// `count` sweeps, each point of member k posed by exp((s - ref_time_k) xi_k): one table — [members][prefix of the grid][box accumulators:
// 8 words per member][ticket] — and ONE launch over the concatenation.  The times come from host arrays (times != null: all members'
// in ONE slot of the staging ring, which the kernel reads by its device address) or, for a single member, from a device array (dtimes).
// A blocking context waits for the members' boxes (the context's box block: its one wait); a stream-ordered one waits for nothing.
static int cloud_deskew(sga_context* ctx, const sga_cloud* const* clouds, const float* const* times, const sga_device_array* dtimes, const double* twists, const double* ref_times, size_t count, void* user_stream, int flags, sga_cloud** out) {
  null_out(out, count);
  if (!ctx || (count > 0 && (!out || !clouds || (!times && !dtimes) || !twists))) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(cloud_members_args(clouds, count, reinterpret_cast<const void* const*>(times), "times"));
  for (size_t k = 0; k < count; k++) {
    for (int e = 0; e < 6; e++)
      if (!(twists[6 * k + e] - twists[6 * k + e] == 0.0)) return fail(SGA_ERR_INVALID, "twist %zu has a non-finite entry", k);
    if (ref_times != nullptr && !(ref_times[k] - ref_times[k] == 0.0)) return fail(SGA_ERR_INVALID, "reference time %zu is not finite", k);
  }
  if (count == 0) return SGA_OK;
  // ---- (from here on the handles are read)
  CloudMembers mem;
  SGA_TRY(cloud_members(ctx, clouds, count, kIoBlock, &mem));
  const std::vector<size_t>& live = mem.live;
  const size_t total = mem.points;
  if (mem.blocks >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points in all (%zu)", total);
  if (!live.empty()) SGA_HIP(hipSetDevice(ctx->device));
  for (size_t k : live) SGA_TRY(deskew_times_check(ctx, clouds[k]->n, times ? times[k] : nullptr, dtimes, k));
  StreamScope stream_scope(ctx->stream);
  std::vector<std::unique_ptr<sga_cloud>> made(count);
  for (size_t k = 0; k < count; k++) SGA_TRY(cloud_make_like(ctx, clouds[k], clouds[k]->n, &made[k]));  // a sweep moves by metres: it stays in its frame
  if (live.empty()) return hand_over(made, out);
  const size_t L = live.size();
  const bool want_box = !ctx->stream_ordered;
  for (size_t k : live) SGA_TRY(wait_ready(ctx, clouds[k]->ready));  // made by another context in stream-ordered mode (common.hpp: Ready)
  // ---- host times: all members' in one slot of the staging ring
  sga_context::StageSlot* tslot = nullptr;
  if (times != nullptr) {
    SGA_TRY(stage_acquire(ctx, total * sizeof(float), &tslot));
    size_t off = 0;
    for (size_t k : live) {
      std::memcpy(static_cast<float*>(tslot->host) + off, times[k], clouds[k]->n * sizeof(float));
      off += clouds[k]->n;
    }
  }
  // ---- the table
  TableLayout lay;
  const auto s_members = lay.add<DeskewMember>(L);
  const auto s_prefix = lay.add_prefixes(1, L);
  MemberBoxes boxes;
  boxes.add(lay, want_box ? L : 0);
  DevBuf<unsigned long long> table;
  ForestBoxes hand;
  SGA_TRY(boxes.begin(ctx, lay, table, &hand));
  std::vector<DeskewMember> members(L);
  std::vector<uint32_t> prefix(L + 1, 0u);
  size_t toff = 0;
  for (size_t j = 0; j < L; j++) {
    const size_t k = live[j];
    const sga_cloud* in = clouds[k];
    DeskewMember& g = members[j];
    std::memset(&g, 0, sizeof(g));
    g.pts = in->pts.p, g.nrm = in->has_normals ? in->nrm.p : nullptr, g.cov = in->has_covs ? in->cov.p : nullptr;
    g.opts = made[k]->pts.p, g.onrm = made[k]->nrm.p, g.ocov = made[k]->cov.p;
    if (times != nullptr) {
      g.times = static_cast<const float*>(tslot->dev) + toff, g.tstride = 1, g.tf64 = 0;
      toff += in->n;
    } else {
      g.times = dtimes->data, g.tstride = dtimes->stride, g.tf64 = dtimes->dtype == SGA_F64 ? 1 : 0;
    }
    if (want_box) g.acc = lay.at(boxes.acc, table.p) + 8 * j, g.slot = forest_slot_dev(ctx, j, kBoxSlotWords);
    g.ref_time = ref_times ? ref_times[k] : 1.0;
    g.c = twist_const(twists + 6 * k, in->origin);
    g.n = static_cast<uint32_t>(in->n);
    g.blocks = (g.n + kIoBlock - 1u) / kIoBlock;
    prefix[j + 1] = prefix[j] + g.blocks;
  }
  IoOrder ord;
  if (dtimes != nullptr) SGA_TRY(io_begin(ctx, user_stream, flags, &ord));
  auto enqueue = [&]() -> int {
    count_launch(Chain::Deskew);
    SGA_TRY(upload_table(ctx, table.p, lay.words(), [&](unsigned long long* host) {
      lay.put(s_members, host, members.data());
      lay.put(s_prefix, host, prefix.data());
      boxes.init(host);
    }));
    count_launch(Chain::Deskew);
    hipLaunchKernelGGL(deskew_cloud_kernel, dim3(prefix[L]), dim3(kIoBlock), 0, ctx->stream, lay.at(s_members, table.p), lay.at(s_prefix, table.p), static_cast<int>(L), hand);
    SGA_HIP(hipGetLastError());
    return SGA_OK;
  };
  if (!want_box) {  // a stream-ordered context waits for nothing
    SGA_TRY(enqueue());
    if (tslot != nullptr) SGA_TRY(stage_release(ctx, tslot));
  } else {  // (a blocking context: the wait shows that the kernel is over)
    SGA_TRY(forest_call_wait(ctx, enqueue(), hand.seq, "boxes of a deskew"));
    for (size_t j = 0; j < L; j++) boxes.read(ctx, j, made[live[j]].get());  // the rounding is monotone: the rounded box of the unrounded records is the box of the records
  }
  if (dtimes != nullptr) SGA_TRY(io_end(ctx, ord));
  for (size_t k : live) SGA_TRY(mark_ready(ctx, made[k]->ready));
  return hand_over(made, out);
}

extern "C" {

// Posed clouds joined into one (the host loop of src/test/registration_test.cpp:84 over points, normals and covs, on the device)
int sga_cloud_merge(sga_context* ctx, const sga_cloud* const* clouds, const double* T, size_t count, const double origin[3], sga_cloud** out) { return cloud_merge(ctx, clouds, T, count, origin, out); }

int sga_cloud_transform(sga_context* ctx, const sga_cloud* cloud, const double T[16], const double origin[3], sga_cloud** out) { return cloud_merge(ctx, &cloud, T, 1, origin, out); }

// Sweeps deskewed on the device: every point posed by exp((its time - ref_time) twist), DESIGN.md section 3.19
int sga_cloud_deskew_batch(sga_context* ctx, const sga_cloud* const* clouds, const float* const* times, const double* twists, const double* ref_times, size_t count, sga_cloud** out) {
  return cloud_deskew(ctx, clouds, times, nullptr, twists, ref_times, count, nullptr, 0, out);
}

int sga_cloud_deskew(sga_context* ctx, const sga_cloud* cloud, const float* times, const double twist[6], double ref_time, sga_cloud** out) {
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  return cloud_deskew(ctx, &cloud, &times, nullptr, twist, &ref_time, 1, nullptr, 0, out);
}

int sga_cloud_deskew_device(sga_context* ctx, const sga_cloud* cloud, const sga_device_array* times, const double twist[6], double ref_time, void* user_stream, int flags, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!out || !times) return fail(SGA_ERR_INVALID, "null argument");
  if (times->dtype != SGA_F32 && times->dtype != SGA_F64) return fail(SGA_ERR_INVALID, "times: dtype %d is neither SGA_F32 nor SGA_F64", times->dtype);
  if (times->cols != 1 || times->stride < 1) return fail(SGA_ERR_INVALID, "times: cols = %d, stride = %d (one time per row, rows one element or more apart)", times->cols, times->stride);
  return cloud_deskew(ctx, &cloud, nullptr, times, twist, &ref_time, 1, user_stream, flags, out);
}

int sga_debug_cloud_deskew_launches(unsigned long long* launches) { return report_launches(Chain::Deskew, launches); }

int sga_debug_cloud_merge_launches(unsigned long long* launches) { return report_launches(Chain::Merge, launches); }

}  // extern "C"

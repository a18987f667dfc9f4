// Device frames (common.hpp): the choice of an origin and, at the C-ABI boundary, the caller's pose -> the pose between the two device
// frames, a system of the source's device frame -> the caller's twist convention (on the host and, for the asynchronous entry points, on
// the device), and the check that the ranks of a sharded registration share one source frame.
#include "batch.hpp"
#include "common.hpp"

#include <cmath>

namespace sga {

int comm_allreduce_sum(sga_context* ctx, double* d_buf, size_t count);  // comm.hip

void choose_origin(const double lo[3], const double hi[3], double origin[3]) {
  for (int k = 0; k < 3; k++) {
    origin[k] = 0.0;
    if (!(lo[k] <= hi[k])) continue;  // empty or non-finite
    const double c = 0.5 * (lo[k] + hi[k]);
    if (c - c != 0.0) continue;
    origin[k] = kOriginQuantum * std::nearbyint(c / kOriginQuantum);
  }
}

void pose_to_device(const double T[16], const double o_s[3], const double o_t[3], double Td[16]) {
  for (int i = 0; i < 16; i++) Td[i] = T[i];
  for (int r = 0; r < 3; r++) Td[12 + r] = (T[r] * o_s[0] + T[4 + r] * o_s[1] + T[8 + r] * o_s[2]) + (T[12 + r] - o_t[r]);  // R o_s + (t - o_t)
}

void system_to_caller(const double o[3], double H[36], double b[6]) {
  // A = [[I, 0], [X, I]], X = -skew(o):  H = A^T H' A, b = A^T b'  (J = J' A with J' = [R skew(p'), -R], p = p' + o)
  const double X[3][3] = {{0, o[2], -o[1]}, {-o[2], 0, o[0]}, {o[1], -o[0], 0}};
  double HA[6][6];  // H' A: columns 0..2 get H'[:, 3..5] X added
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double v = H[6 * i + j];
      if (j < 3)
        for (int k = 0; k < 3; k++) v += H[6 * i + 3 + k] * X[k][j];
      HA[i][j] = v;
    }
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {  // the upper triangle, mirrored as frame_accumulator_kernel does: the two roundings of an entry pair would differ
      double v = HA[i][j];
      if (i < 3)
        for (int k = 0; k < 3; k++) v += X[k][i] * HA[3 + k][j];  // (A^T)[i][3 + k] = X[k][i]
      H[6 * i + j] = H[6 * j + i] = v;
    }
  for (int i = 0; i < 3; i++)
    for (int k = 0; k < 3; k++) b[i] += X[k][i] * b[3 + k];
}

// ---- device frames (common.hpp): what crosses the boundary is converted HERE, everything below works between the two device frames ----
bool problem_framed(const sga_problem* pb) { return !origin_is_zero(pb->src_origin) || !origin_is_zero(pb->target->origin); }
// the caller's pose -> the same rigid motion between the source's and the target's device frames; returns Td (or T itself when both origins are 0)
const double* problem_pose(const sga_problem* pb, const double T[16], double Td[16]) {
  if (!problem_framed(pb)) return T;
  pose_to_device(T, pb->src_origin, pb->target->origin, Td);
  return Td;
}
void problem_system_to_caller(const sga_problem* pb, double H[36], double b[6]) {
  if (!origin_is_zero(pb->src_origin)) system_to_caller(pb->src_origin, H, b);
}
// the 30-double accumulator of the asynchronous entry points, in place on the device (one thread: a 6x6 congruence)
__global__ void frame_accumulator_kernel(double* __restrict__ acc, double ox, double oy, double oz) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double H[36], b[6];
  int k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      H[6 * i + j] = H[6 * j + i] = acc[k];
      k++;
    }
  for (int i = 0; i < 6; i++) b[i] = acc[21 + i];
  const double X[3][3] = {{0, oz, -oy}, {-oz, 0, ox}, {oy, -ox, 0}};  // -skew(o), see system_to_caller above
  double HA[6][6];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < 6; j++) {
      double v = H[6 * i + j];
      if (j < 3)
        for (int c = 0; c < 3; c++) v += H[6 * i + 3 + c] * X[c][j];
      HA[i][j] = v;
    }
  k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      double v = HA[i][j];
      if (i < 3)
        for (int c = 0; c < 3; c++) v += X[c][i] * HA[3 + c][j];
      acc[k++] = v;
    }
  for (int i = 0; i < 3; i++) {
    double v = b[i];
    for (int c = 0; c < 3; c++) v += X[c][i] * b[3 + c];
    acc[21 + i] = v;
  }
}
int problem_accumulator_to_caller(sga_context* ctx, const sga_problem* pb, double* d_out30) {
  if (!origin_is_zero(pb->src_origin)) {  // the caller reads H / b in its own twist convention (common.hpp: device frames)
    hipLaunchKernelGGL(frame_accumulator_kernel, dim3(1), dim3(64), 0, ctx->stream, d_out30, pb->src_origin[0], pb->src_origin[1], pb->src_origin[2]);
    SGA_HIP(hipGetLastError());
  }
  return SGA_OK;
}
// Sharded contexts add the ranks' accumulators: their moments are sums over source points in the SOURCE's device frame, so every rank's
// shard must live in the same one (slices of one uploaded cloud do: sga_cloud_slice; separately uploaded shards name a common origin:
// sga_cloud_create_*_origin).  Checked once per problem with one small sum over the ranks: all equal <=> n sum(o^2) == (sum o)^2.
// The ranks of a sharded registration must share ONE source frame (their accumulators are added).  Compared with one all-reduce of sums
// that are EXACT for any number of ranks and any origin (n * sum(o^2) == (sum o)^2 on the doubles themselves rounds differently
// on both sides for 3+ ranks and non-round origins): every origin coordinate is cut into four 16-bit pieces of its bit pattern, each an
// integer < 2^16, and the ranks add the pieces p and their squares p^2.  All of those sums are integers below 2^53 for up to 2^10 ranks, so
// they do not depend on the order of the additions, every rank reads the same numbers and takes the same decision, and by the equality case
// of Cauchy-Schwarz  n * sum(p^2) == (sum p)^2  holds iff all ranks hold the same piece.
constexpr int kFrameCheckDoubles = SGA_FRAME_CHECK_DOUBLES;
void shard_frame_pack(const double origin[3], double out[kFrameCheckDoubles]) {
  for (int k = 0; k < 3; k++) {
    const double o = origin[k] + 0.0;  // -0.0 and +0.0 are one origin
    unsigned long long bits;
    memcpy(&bits, &o, sizeof(bits));
    for (int j = 0; j < 4; j++) {
      const double piece = static_cast<double>((bits >> (16 * j)) & 0xffffull);
      out[4 * k + j] = piece;
      out[12 + 4 * k + j] = piece * piece;
    }
  }
  out[24] = 1.0;  // the number of ranks
  for (int i = 25; i < kFrameCheckDoubles; i++) out[i] = 0.0;
}
bool shard_frame_agree(const double sum[kFrameCheckDoubles]) {
  for (int i = 0; i < 12; i++)
    if (sum[24] * sum[12 + i] != sum[i] * sum[i]) return false;
  return true;
}
int problem_check_shard_frames(sga_context* ctx, sga_problem* pb) {
  if (pb->frame_checked || !ctx->sharded()) return SGA_OK;
  double h[kFrameCheckDoubles];
  shard_frame_pack(pb->src_origin, h);
  DevBuf<double> d;
  SGA_TRY(d.alloc(kFrameCheckDoubles));
  SGA_HIP(hipMemcpyAsync(d.p, h, sizeof(h), hipMemcpyHostToDevice, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  SGA_TRY(comm_allreduce_sum(ctx, d.p, kFrameCheckDoubles));
  SGA_HIP(hipMemcpyAsync(h, d.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  if (!shard_frame_agree(h))
    return fail(SGA_ERR_INVALID, "the source shards of the ranks live in different device frames (origins differ): slice ONE uploaded cloud (sga_cloud_slice) or upload the shards with a common origin (sga_cloud_create_f64_origin)");
  pb->frame_checked = true;
  return SGA_OK;
}
}  // namespace sga

using namespace sga;

extern "C" {

int sga_index_origin(const sga_index* index, double origin[3]) {
  if (!index || !origin) return fail(SGA_ERR_INVALID, "null argument");
  for (int k = 0; k < 3; k++) origin[k] = index->origin[k];
  return SGA_OK;
}

void sga_choose_origin(const double lo[3], const double hi[3], double origin[3]) { choose_origin(lo, hi, origin); }

void sga_debug_shard_frame_pack(const double origin[3], double out[SGA_FRAME_CHECK_DOUBLES]) { shard_frame_pack(origin, out); }
int sga_debug_shard_frame_agree(const double sum[SGA_FRAME_CHECK_DOUBLES]) { return shard_frame_agree(sum) ? 1 : 0; }

}  // extern "C"

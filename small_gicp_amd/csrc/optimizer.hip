// Host side of Registration<>::align: Levenberg-Marquardt / Gauss-Newton over the 6x6 normal equations.
// Mirrors registration/optimizer.hpp:24-149, termination_criteria.hpp:11-20, general_factor.hpp:41-75 and
// util/lie.hpp:54-96 of the reference (/root/reference) including their control-flow quirks:
//   * LM accepts a step iff new_e <= e, then lambda /= factor, else lambda *= factor (<= 10 trials per outer iteration);
//   * result.iterations is the index of the last executed outer iteration; result.H/b are the last linearization;
//   * convergence is tested on the accepted delta only: |rot| <= rotation_eps && |trans| <= translation_eps.
// The reductions are callbacks so the same optimizer drives one GPU (sga_align) or sharded GPUs + all-reduce (sga_optimize).
#include <cmath>
#include <cstdio>

#include "batch.hpp"
#include "common.hpp"
#include "lie.hpp"

namespace sga {

// ---- tiny fixed-size double algebra (host) ------------------------------------------------------------------------------------
struct M4 {
  double a[16];  // column-major
};

static M4 mul(const M4& A, const M4& B) {
  M4 C;
  for (int c = 0; c < 4; c++)
    for (int r = 0; r < 4; r++) {
      double s = 0;
      for (int k = 0; k < 4; k++) s += A.a[4 * k + r] * B.a[4 * c + k];
      C.a[4 * c + r] = s;
    }
  return C;
}

// util/lie.hpp:77-96 — rotation-first twist; quaternion exp map after Sophus (lie.hpp:54-71), Eigen's toRotationMatrix.
static M4 se3_exp(const double d[6]) {
  const double wx = d[0], wy = d[1], wz = d[2];
  const double theta_sq = wx * wx + wy * wy + wz * wz;
  const double theta = std::sqrt(theta_sq);
  double imag, real;
  if (theta_sq < 1e-10) {
    const double t4 = theta_sq * theta_sq;
    imag = 0.5 - theta_sq / 48.0 + t4 / 3840.0;
    real = 1.0 - theta_sq / 8.0 + t4 / 384.0;
  } else {
    imag = std::sin(0.5 * theta) / theta;
    real = std::cos(0.5 * theta);
  }
  const double qw = real, qx = imag * wx, qy = imag * wy, qz = imag * wz;
  double R[3][3];
  {
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw;
    const double txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    R[0][0] = 1 - (tyy + tzz);
    R[0][1] = txy - twz;
    R[0][2] = txz + twy;
    R[1][0] = txy + twz;
    R[1][1] = 1 - (txx + tzz);
    R[1][2] = tyz - twx;
    R[2][0] = txz - twy;
    R[2][1] = tyz + twx;
    R[2][2] = 1 - (txx + tyy);
  }
  double t[3];
  const double v[3] = {d[3], d[4], d[5]};
  if (theta < 1e-10) {
    for (int r = 0; r < 3; r++) t[r] = R[r][0] * v[0] + R[r][1] * v[1] + R[r][2] * v[2];
  } else {
    const double W[3][3] = {{0, -wz, wy}, {wz, 0, -wx}, {-wy, wx, 0}};
    const double c1 = (1.0 - std::cos(theta)) / theta_sq, c2 = (theta - std::sin(theta)) / (theta_sq * theta);
    for (int r = 0; r < 3; r++) {
      t[r] = 0;
      for (int c = 0; c < 3; c++) {
        double w2 = 0;
        for (int k = 0; k < 3; k++) w2 += W[r][k] * W[k][c];
        t[r] += ((r == c ? 1.0 : 0.0) + c1 * W[r][c] + c2 * w2) * v[c];
      }
    }
  }
  M4 T;
  for (int i = 0; i < 16; i++) T.a[i] = 0;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T.a[4 * c + r] = R[r][c];
    T.a[12 + r] = t[r];
  }
  T.a[15] = 1;
  return T;
}

// Solve (H + lambda I) x = -b: symmetric-indefinite-safe LDL^T with diagonal pivoting (the reference calls Eigen's ldlt()).
static void solve_damped(const double H[36], const double b[6], double lambda, double x[6]) {
  double A[6][6];
  int p[6];
  for (int i = 0; i < 6; i++) {
    p[i] = i;
    for (int j = 0; j < 6; j++) A[i][j] = H[6 * i + j] + (i == j ? lambda : 0.0);
  }
  for (int k = 0; k < 6; k++) {
    int piv = k;
    for (int i = k + 1; i < 6; i++)
      if (std::fabs(A[i][i]) > std::fabs(A[piv][piv])) piv = i;
    if (piv != k) {
      for (int j = 0; j < 6; j++) std::swap(A[k][j], A[piv][j]);
      for (int i = 0; i < 6; i++) std::swap(A[i][k], A[i][piv]);
      std::swap(p[k], p[piv]);
    }
    const double dk = A[k][k];
    if (dk == 0.0) continue;
    for (int i = k + 1; i < 6; i++) A[i][k] /= dk;
    for (int i = k + 1; i < 6; i++)
      for (int j = k + 1; j <= i; j++) {
        A[i][j] -= A[i][k] * dk * A[j][k];
        A[j][i] = A[i][j];
      }
  }
  double y[6];
  for (int i = 0; i < 6; i++) y[i] = -b[p[i]];
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < i; j++) y[i] -= A[i][j] * y[j];
  for (int i = 0; i < 6; i++) y[i] = A[i][i] != 0.0 ? y[i] / A[i][i] : 0.0;
  for (int i = 5; i >= 0; i--)
    for (int j = i + 1; j < 6; j++) y[i] -= A[j][i] * y[j];
  for (int i = 0; i < 6; i++) x[p[i]] = y[i];
}

static bool converged(const sga_registration_setting& s, const double d[6]) {
  return std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) <= s.rotation_eps && std::sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]) <= s.translation_eps;
}

static void apply_general_factor(const sga_registration_setting& s, double H[36]) {
  // general_factor.hpp:66: *H += lambda * (mask - 1).abs().asDiagonal()
  if (s.restrict_dof_lambda > 0)
    for (int i = 0; i < 6; i++) H[7 * i] += s.restrict_dof_lambda * std::fabs(s.restrict_dof_mask[i] - 1.0);
}

static int optimize_impl(const sga_registration_setting& s, const double init_T[16], sga_linearize_fn lin, sga_error_fn err, void* user, sga_result* out) {
  M4 T;
  for (int i = 0; i < 16; i++) T.a[i] = init_T[i];
  out->converged = 0;
  out->iterations = 0;
  out->num_inliers = 0;
  for (int i = 0; i < 36; i++) out->H[i] = 0;
  for (int i = 0; i < 6; i++) out->b[i] = 0;
  out->error = 0;
  double H[36], b[6], e = 0;
  uint64_t inliers = 0;
  if (s.optimizer == SGA_GAUSS_NEWTON) {
    if (s.verbose) std::printf("--- GN optimization ---\n");
    for (int i = 0; i < s.max_iterations && !out->converged; i++) {
      if (lin(user, T.a, H, b, &e, &inliers)) return fail(SGA_ERR_CALLBACK, "linearize callback failed");
      apply_general_factor(s, H);
      double delta[6];
      solve_damped(H, b, s.gn_lambda, delta);
      if (s.verbose)
        std::printf("iter=%d e=%g lambda=%g dt=%g dr=%g\n", i, e, s.gn_lambda, std::sqrt(delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5]), std::sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]));
      out->converged = converged(s, delta);
      T = mul(T, se3_exp(delta));
      out->iterations = i;
      memcpy(out->H, H, sizeof(H));
      memcpy(out->b, b, sizeof(b));
      out->error = e;
    }
  } else {
    if (s.verbose) std::printf("--- LM optimization ---\n");
    double lambda = s.init_lambda;
    for (int i = 0; i < s.max_iterations && !out->converged; i++) {
      if (lin(user, T.a, H, b, &e, &inliers)) return fail(SGA_ERR_CALLBACK, "linearize callback failed");
      apply_general_factor(s, H);
      bool success = false;
      for (int j = 0; j < s.max_inner_iterations; j++) {
        double delta[6];
        solve_damped(H, b, lambda, delta);
        const M4 new_T = mul(T, se3_exp(delta));
        double new_e = 0;
        if (err(user, new_T.a, &new_e)) return fail(SGA_ERR_CALLBACK, "error callback failed");
        if (s.verbose)
          std::printf(
            "iter=%d inner=%d e=%g new_e=%g lambda=%g dt=%g dr=%g\n", i, j, e, new_e, lambda, std::sqrt(delta[3] * delta[3] + delta[4] * delta[4] + delta[5] * delta[5]),
            std::sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]));
        if (new_e <= e) {
          out->converged = converged(s, delta);
          T = new_T;
          lambda /= s.lambda_factor;
          success = true;
          e = new_e;
          break;
        }
        lambda *= s.lambda_factor;
      }
      out->iterations = i;
      memcpy(out->H, H, sizeof(H));
      memcpy(out->b, b, sizeof(b));
      out->error = e;
      if (!success) break;
    }
  }
  out->num_inliers = inliers;  // == count_if(factors, inlier()) after the last linearize (optimizer.hpp:146)
  memcpy(out->T_target_source, T.a, sizeof(T.a));
  return SGA_OK;
}

// ---- the same loop for `count` independent pairs in lock-step ROUNDS -----------------------------------------------------------------
// Every pair runs optimize_impl's loop as a state machine: it waits for a linearization (kLinearize), then — LM — for the error of its
// trial pose (kError), any number of times, and so on until it is done.  A round serves all pairs that wait for the same thing with ONE
// batched callback; a pair that is done appears in no later request.  Per pair the sequence of requests, their poses and the result are
// exactly those of optimize_impl over that pair alone (tests/test_batch_optimizer.py compares them bit for bit).
struct PairState {
  enum Phase { kLinearize, kError, kDone } phase = kDone;
  M4 T, new_T;
  double lambda = 0, delta[6] = {0};
  int i = 0, j = 0;  // outer / inner iteration
  double H[36] = {0}, b[6] = {0}, e = 0;  // the accumulators of optimize_impl: a callback that leaves one untouched leaves the previous value
  uint64_t inliers = 0;
};

static int optimize_batch_impl(const sga_registration_setting& s, size_t count, const double* init_T, sga_batch_linearize_fn lin, sga_batch_error_fn err, void* user, sga_result* out) {
  static const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  const bool gn = s.optimizer == SGA_GAUSS_NEWTON;
  std::vector<PairState> st(count);
  std::vector<unsigned char> mask(count);
  std::vector<double> Ts(16 * count), Hs(36 * count), bs(6 * count), es(count);
  std::vector<uint64_t> inl(count);
  for (size_t k = 0; k < count; k++) {
    PairState& p = st[k];
    sga_result& r = out[k];
    memcpy(p.T.a, init_T ? init_T + 16 * k : I16, sizeof(p.T.a));
    r.converged = 0;
    r.iterations = 0;
    r.num_inliers = 0;
    for (int i = 0; i < 36; i++) r.H[i] = 0;
    for (int i = 0; i < 6; i++) r.b[i] = 0;
    r.error = 0;
    p.lambda = s.init_lambda;
    p.phase = s.max_iterations > 0 ? PairState::kLinearize : PairState::kDone;
    if (s.verbose) std::printf("pair=%zu --- %s optimization ---\n", k, gn ? "GN" : "LM");
  }
  // the end of outer iteration p.i (optimizer.hpp: after the inner loop)
  auto end_iteration = [&](PairState& p, sga_result& r, bool success) {
    r.iterations = p.i;
    memcpy(r.H, p.H, sizeof(p.H));
    memcpy(r.b, p.b, sizeof(p.b));
    r.error = p.e;
    p.i++;
    p.phase = (success && p.i < s.max_iterations && !r.converged) ? PairState::kLinearize : PairState::kDone;
  };
  // LM: the next trial of the inner loop, or its unsuccessful end
  auto next_trial = [&](PairState& p, sga_result& r) {
    if (p.j >= s.max_inner_iterations) return end_iteration(p, r, false);
    solve_damped(p.H, p.b, p.lambda, p.delta);
    p.new_T = mul(p.T, se3_exp(p.delta));
    p.phase = PairState::kError;
  };
  auto gather = [&](PairState::Phase ph) {
    bool any = false;
    for (size_t k = 0; k < count; k++) {
      mask[k] = st[k].phase == ph ? 1 : 0;
      any = any || mask[k];
    }
    return any;
  };
  for (;;) {
    if (!gather(PairState::kLinearize)) break;  // (no pair waits for an error between rounds)
    for (size_t k = 0; k < count; k++) {
      if (!mask[k]) continue;
      const PairState& p = st[k];
      memcpy(&Ts[16 * k], p.T.a, sizeof(p.T.a));
      memcpy(&Hs[36 * k], p.H, sizeof(p.H));
      memcpy(&bs[6 * k], p.b, sizeof(p.b));
      es[k] = p.e;
      inl[k] = p.inliers;
    }
    if (lin(user, count, mask.data(), Ts.data(), Hs.data(), bs.data(), es.data(), inl.data())) return fail(SGA_ERR_CALLBACK, "linearize callback failed");
    for (size_t k = 0; k < count; k++) {
      if (!mask[k]) continue;
      PairState& p = st[k];
      sga_result& r = out[k];
      memcpy(p.H, &Hs[36 * k], sizeof(p.H));
      memcpy(p.b, &bs[6 * k], sizeof(p.b));
      p.e = es[k];
      p.inliers = inl[k];
      apply_general_factor(s, p.H);
      if (gn) {
        solve_damped(p.H, p.b, s.gn_lambda, p.delta);
        const double* d = p.delta;
        if (s.verbose) std::printf("pair=%zu iter=%d e=%g lambda=%g dt=%g dr=%g\n", k, p.i, p.e, s.gn_lambda, std::sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]), std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
        r.converged = converged(s, p.delta);
        p.T = mul(p.T, se3_exp(p.delta));
        end_iteration(p, r, true);
      } else {
        p.j = 0;
        next_trial(p, r);
      }
    }
    while (gather(PairState::kError)) {  // the LM inner loops, trial by trial
      for (size_t k = 0; k < count; k++)
        if (mask[k]) {
          memcpy(&Ts[16 * k], st[k].new_T.a, sizeof(st[k].new_T.a));
          es[k] = 0;
        }
      if (err(user, count, mask.data(), Ts.data(), es.data())) return fail(SGA_ERR_CALLBACK, "error callback failed");
      for (size_t k = 0; k < count; k++) {
        if (!mask[k]) continue;
        PairState& p = st[k];
        sga_result& r = out[k];
        const double new_e = es[k];
        const double* d = p.delta;
        if (s.verbose)
          std::printf(
            "pair=%zu iter=%d inner=%d e=%g new_e=%g lambda=%g dt=%g dr=%g\n", k, p.i, p.j, p.e, new_e, p.lambda, std::sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]), std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]));
        if (new_e <= p.e) {
          r.converged = converged(s, p.delta);
          p.T = p.new_T;
          p.lambda /= s.lambda_factor;
          p.e = new_e;
          end_iteration(p, r, true);
        } else {
          p.lambda *= s.lambda_factor;
          p.j++;
          next_trial(p, r);
        }
      }
    }
  }
  for (size_t k = 0; k < count; k++) {
    out[k].num_inliers = st[k].inliers;
    memcpy(out[k].T_target_source, st[k].T.a, sizeof(st[k].T.a));
  }
  return SGA_OK;
}

// sga_align_batch's reductions: the batched round on the device, the error model of each pair's last linearization on the host
struct GpuBatchReduction {
  sga_context* ctx;
  sga_batch* bt;
  const sga_factor_params* fp;
  bool first;  // the first round of a registration walks without the neighbours of earlier calls
};

static int gpu_batch_linearize(void* user, size_t count, const unsigned char* active, const double* T, double* H, double* b, double* e, uint64_t* inl) {
  auto* g = static_cast<GpuBatchReduction*>(user);
  const int rc = batch_round(g->ctx, g->bt, g->fp, T, active, g->first);
  g->first = false;
  if (rc != SGA_OK) return rc;
  for (size_t k = 0; k < count; k++) {
    if (!active[k]) continue;
    batch_unpack(g->bt, k, H + 36 * k, b + 6 * k, e + k, inl + k);
  }
  return SGA_OK;
}
static int gpu_batch_error(void* user, size_t count, const unsigned char* active, const double* T, double* e) {
  auto* g = static_cast<GpuBatchReduction*>(user);
  for (size_t k = 0; k < count; k++) {
    if (!active[k]) continue;
    const sga_problem* pb = g->bt->problems[k];
    double Tdev[16];
    e[k] = error_model_value(pb->model, pb->model_T, problem_pose(pb, T + 16 * k, Tdev));  // what sga_error answers after sga_linearize
  }
  return SGA_OK;
}

struct GpuReduction {
  sga_context* ctx;
  sga_problem* pb;
  const sga_factor_params* fp;
};

static int gpu_linearize(void* user, const double T[16], double H[36], double b[6], double* e, uint64_t* inl) {
  auto* g = static_cast<GpuReduction*>(user);
  return sga_linearize(g->ctx, g->pb, g->fp, T, H, b, e, inl);
}
static int gpu_error(void* user, const double T[16], double* e) {
  auto* g = static_cast<GpuReduction*>(user);
  return sga_error(g->ctx, g->pb, g->fp, T, e);
}

}  // namespace sga

using namespace sga;

extern "C" {

void sga_registration_setting_default(sga_registration_setting* s) {
  if (!s) return;
  sga_factor_params_default(&s->factor);
  s->optimizer = SGA_LEVENBERG_MARQUARDT;
  s->max_iterations = 20;
  s->max_inner_iterations = 10;
  s->init_lambda = 1e-3;
  s->lambda_factor = 10.0;
  s->gn_lambda = 1e-6;
  s->translation_eps = 1e-3;
  s->rotation_eps = 0.1 * M_PI / 180.0;
  s->verbose = 0;
  s->restrict_dof_lambda = 0.0;
  for (int i = 0; i < 6; i++) s->restrict_dof_mask[i] = 1.0;
}

// The public exponential and its inverse are evaluated without cancellation (lie.hpp).  The optimizer keeps
// se3_exp above — the reference's expressions, whose (1 - cos) / theta^2 loses digits at small angles — so that a registration's poses
// stay the reference's.
void sga_se3_exp(const double twist[6], double T[16]) {
  static const double zero[3] = {0, 0, 0};
  const TwistConst c = twist_const(twist, zero);
  double r[9], t[3];
  twist_pose(c, 1.0, r, t);
  for (int col = 0; col < 4; col++)
    for (int row = 0; row < 4; row++) T[4 * col + row] = row == 3 ? (col == 3 ? 1.0 : 0.0) : col == 3 ? t[row] : r[3 * row + col];
}

// T (a rigid transform with rotation angle theta < pi) -> the twist whose exponential it is.  omega = (theta / sin theta) w with
// w = vee(R - R^T) / 2 and theta = atan2(|w|, (tr R - 1) / 2): a quotient of two accurate numbers, or the series of asin(s) / s below
// s = 0.01; what is lost towards pi is what R itself no longer holds, a factor 1 / (pi - theta).  v solves V v = t with
// V = I + (1 - cos) / theta K + (theta - sin) / theta K^2 from lie.hpp's coefficients; V's condition number is at most pi / 2.
void sga_se3_log(const double T[16], double twist[6]) {
  auto R = [&](int row, int col) { return T[4 * col + row]; };
  const double w[3] = {0.5 * (R(2, 1) - R(1, 2)), 0.5 * (R(0, 2) - R(2, 0)), 0.5 * (R(1, 0) - R(0, 1))};
  const double m = std::fmax(std::fabs(w[0]), std::fmax(std::fabs(w[1]), std::fabs(w[2])));
  double s = 0.0;
  if (m > 0.0) s = m * std::sqrt((w[0] / m) * (w[0] / m) + (w[1] / m) * (w[1] / m) + (w[2] / m) * (w[2] / m));
  const double c = 0.5 * (R(0, 0) + R(1, 1) + R(2, 2) - 1.0);
  const double q = s * s;
  const double factor = (c > 0.0 && s < 1e-2) ? 1.0 + q * (1.0 / 6.0 + q * (3.0 / 40.0 + q * (15.0 / 336.0 + q * (105.0 / 3456.0)))) : std::atan2(s, c) / s;
  double xi[6] = {factor * w[0], factor * w[1], factor * w[2], 0.0, 0.0, 0.0};
  static const double zero[3] = {0, 0, 0};
  const TwistConst k = twist_const(xi, zero);
  double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  if (k.theta > 0.0) {
    const RotCoef f = rot_coef(k.theta);
    const double b = f.c2 / k.theta, d = f.f3 / k.theta;
    const double K[3][3] = {{0, -k.k[2], k.k[1]}, {k.k[2], 0, -k.k[0]}, {-k.k[1], k.k[0], 0}};
    const double KK[3][3] = {{k.kk[0], k.kk[1], k.kk[2]}, {k.kk[1], k.kk[3], k.kk[4]}, {k.kk[2], k.kk[4], k.kk[5]}};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) V[i][j] += b * K[i][j] + d * KK[i][j];
  }
  // v = adj(V) t / det V
  const double A[3][3] = {{V[1][1] * V[2][2] - V[1][2] * V[2][1], V[0][2] * V[2][1] - V[0][1] * V[2][2], V[0][1] * V[1][2] - V[0][2] * V[1][1]},
                          {V[1][2] * V[2][0] - V[1][0] * V[2][2], V[0][0] * V[2][2] - V[0][2] * V[2][0], V[0][2] * V[1][0] - V[0][0] * V[1][2]},
                          {V[1][0] * V[2][1] - V[1][1] * V[2][0], V[0][1] * V[2][0] - V[0][0] * V[2][1], V[0][0] * V[1][1] - V[0][1] * V[1][0]}};
  const double det = V[0][0] * A[0][0] + V[0][1] * A[1][0] + V[0][2] * A[2][0];
  for (int i = 0; i < 3; i++) xi[3 + i] = (A[i][0] * T[12] + A[i][1] * T[13] + A[i][2] * T[14]) / det;
  for (int i = 0; i < 6; i++) twist[i] = xi[i];
}

int sga_optimize(const sga_registration_setting* setting, const double init_T[16], sga_linearize_fn linearize, sga_error_fn error, void* user, sga_result* out) {
  if (!setting || !init_T || !linearize || !out) return fail(SGA_ERR_INVALID, "null argument");
  if (setting->optimizer == SGA_LEVENBERG_MARQUARDT && !error) return fail(SGA_ERR_INVALID, "LM needs an error callback");
  return optimize_impl(*setting, init_T, linearize, error, user, out);
}

int sga_align_problem(sga_context* ctx, sga_problem* problem, const double init_T[16], const sga_registration_setting* setting, sga_result* out) {
  if (!ctx || !problem || !setting || !out) return fail(SGA_ERR_INVALID, "null argument");
  static const double I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  // registration.hpp:34-39 warns (does not fail) on tiny clouds
  if (problem->target->n <= 10) std::fprintf(stderr, "warning: target point cloud is too small. |target|=%zu\n", problem->target->n);
  if (problem->n <= 10) std::fprintf(stderr, "warning: source point cloud is too small. |source|=%zu\n", problem->n);
  // every registration starts without search hints: its result must not depend on earlier calls on the same problem
  // (with the canonical tie rule of kd_search.hpp they could not change it anyway; what this guarantees is that no search work is
  // carried over from one registration to the next)
  if (!problem->state_fresh) {  // (a problem nothing has searched yet holds no hints: two fills less for every scan of an odometry stream)
    SGA_HIP(hipSetDevice(ctx->device));
    if (problem->n > 0) SGA_HIP(hipMemsetAsync(problem->hint.p, 0xff, problem->n * sizeof(int), ctx->stream));
    if (problem->n > 0 && problem->hint2.n >= problem->n) SGA_HIP(hipMemsetAsync(problem->hint2.p, 0xff, problem->n * sizeof(int), ctx->stream));
  }
  problem->prev_valid = false;
  GpuReduction g{ctx, problem, &setting->factor};
  return optimize_impl(*setting, init_T ? init_T : I16, gpu_linearize, gpu_error, &g, out);
}

int sga_optimize_batch(const sga_registration_setting* setting, size_t count, const double* init_T, sga_batch_linearize_fn linearize, sga_batch_error_fn error, void* user, sga_result* out) {
  if (!setting || !linearize) return fail(SGA_ERR_INVALID, "null argument");
  if (setting->optimizer == SGA_LEVENBERG_MARQUARDT && !error) return fail(SGA_ERR_INVALID, "LM needs an error callback");
  if (count == 0) return SGA_OK;
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  return optimize_batch_impl(*setting, count, init_T, linearize, error, user, out);
}

int sga_align_batch(sga_context* ctx, sga_batch* batch, const double* init_T, const sga_registration_setting* setting, sga_result* out) {
  if (!setting) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(batch_check(ctx, batch, &setting->factor));
  const size_t count = batch->problems.size();
  if (count == 0) return SGA_OK;
  if (!out) return fail(SGA_ERR_INVALID, "null argument");
  for (size_t k = 0; k < count; k++) {  // registration.hpp:34-39 warns (does not fail) on tiny clouds
    const sga_problem* pb = batch->problems[k];
    if (pb->target->n <= 10) std::fprintf(stderr, "warning: target point cloud is too small. |target|=%zu\n", pb->target->n);
    if (pb->n <= 10) std::fprintf(stderr, "warning: source point cloud is too small. |source|=%zu\n", pb->n);
  }
  SGA_ENTER(ctx);
  // like sga_align_problem, every pair starts without search state of earlier calls: the first round's walks take no seed (no fill per pair)
  GpuBatchReduction g{ctx, batch, &setting->factor, true};
  return optimize_batch_impl(*setting, count, init_T, gpu_batch_linearize, gpu_batch_error, &g, out);
}

int sga_align(sga_context* ctx, const sga_index* target, const sga_cloud* source, const double init_T[16], const sga_registration_setting* setting, sga_result* out) {
  if (!ctx || !target || !source || !setting || !out) return fail(SGA_ERR_INVALID, "null argument");
  sga_problem* pb = nullptr;
  SGA_TRY(sga_problem_create(ctx, target, source, init_T, &pb));
  const int rc = sga_align_problem(ctx, pb, init_T, setting, out);
  sga_problem_destroy(pb);
  return rc;
}

}  // extern "C"

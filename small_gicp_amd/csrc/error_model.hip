// The reduced row of a linearization pass on the host (pass_layout.hpp): the system in its first columns unpacked, and the quadratic
// error model in the others evaluated at a trial pose.  Pure host arithmetic: no kernel, no device call.
#include <utility>

#include "batch.hpp"
#include "pass_layout.hpp"

namespace sga {

// e(T_n) from the quadratic error model of the last linearization (accumulate_model): a few hundred flops on the host
static double evaluate_error_model(const double* acc, const double T[16], const double Tn[16]) {
  // Y = [R^T R_n - I | R^T (tau_n - tau)], column-major 4x4 inputs
  double Y[3][4];
  for (int r = 0; r < 3; r++) {
    for (int a = 0; a < 3; a++) {
      double v = 0.0;
      for (int k = 0; k < 3; k++) v += T[4 * r + k] * Tn[4 * a + k];  // (R^T R_n)[r][a] = sum_k R[k][r] R_n[k][a]
      Y[r][a] = v - (r == a ? 1.0 : 0.0);
    }
    double v = 0.0;
    for (int k = 0; k < 3; k++) v += T[4 * r + k] * (Tn[12 + k] - T[12 + k]);
    Y[r][3] = v;
  }
  // S1[a][j] = sum p_h,a g_j; a = 3: sum g = -b_t
  double S1[4][3];
  for (int a = 0; a < 3; a++)
    for (int j = 0; j < 3; j++) S1[a][j] = acc[kModelOff + 3 * a + j];
  for (int j = 0; j < 3; j++) S1[3][j] = -acc[24 + j];
  // S2[a][b] = sum p_h,a p_h,b M' as symmetric 3x3 (xx, xy, xz, yy, yz, zz)
  auto S2 = [&](int a, int b) -> const double* {
    if (a > b) std::swap(a, b);
    if (b == 3) return a == 3 ? acc + 15 : acc + kModelOff + 9 + 6 * a;
    static const int pair_of[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    return acc + kModelOff + 27 + 6 * pair_of[a][b];
  };
  double lin = 0.0, quad = 0.0;
  for (int a = 0; a < 4; a++) {
    for (int j = 0; j < 3; j++) lin += Y[j][a] * S1[a][j];
    for (int b2 = 0; b2 < 4; b2++) {
      const double* m = S2(a, b2);
      const double ya[3] = {Y[0][a], Y[1][a], Y[2][a]}, yb[3] = {Y[0][b2], Y[1][b2], Y[2][b2]};
      const double mv[3] = {m[0] * yb[0] + m[1] * yb[1] + m[2] * yb[2], m[1] * yb[0] + m[3] * yb[1] + m[4] * yb[2], m[2] * yb[0] + m[4] * yb[1] + m[5] * yb[2]};
      quad += ya[0] * mv[0] + ya[1] * mv[1] + ya[2] * mv[2];
    }
  }
  return acc[27] - lin + 0.5 * quad;
}

double error_model_value(const double* acc96, const double T_lin[16], const double T[16]) { return evaluate_error_model(acc96, T_lin, T); }

}  // namespace sga

using namespace sga;

extern "C" {

void sga_unpack_accumulator(const double acc[SGA_ACCUM_DOUBLES], double H[36], double b[6], double* e, uint64_t* num_inliers) {
  int k = 0;
  for (int i = 0; i < 6; i++)
    for (int j = i; j < 6; j++) {
      H[6 * i + j] = acc[k];
      H[6 * j + i] = acc[k];
      k++;
    }
  for (int i = 0; i < 6; i++) b[i] = acc[21 + i];
  if (e) *e = acc[27];
  if (num_inliers) *num_inliers = static_cast<uint64_t>(acc[28] + 0.5);
}

int sga_error_model_eval(const double acc96[SGA_MODEL_DOUBLES], const double T_lin[16], const double T[16], double* e) {
  if (!acc96 || !T_lin || !T || !e) return fail(SGA_ERR_INVALID, "null argument");
  *e = evaluate_error_model(acc96, T_lin, T);
  return SGA_OK;
}

}  // extern "C"

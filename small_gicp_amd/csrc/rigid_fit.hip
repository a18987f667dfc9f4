// The least-squares rigid motion of point pairs from their sums (host code): Horn's closed form — the rotation is
// the eigenvector of the greatest eigenvalue of a symmetric 4x4 matrix built from the cross-covariance, taken as a unit quaternion — over
// a cyclic Jacobi eigen-solver.  The refit of sga_ransac_correspondences; sga_debug_rigid_from_sums exposes it to tests without a device.
#include "ransac.hpp"

#include <cmath>

namespace sga {
namespace {

// Eigenvalues (the diagonal of A on return) and eigenvectors (the columns of V) of the symmetric N x N matrix A, by cyclic Jacobi
// rotations: every sweep annihilates each off-diagonal entry once; the sum of their squares falls quadratically.
template <int N>
void jacobi_eigen(double A[N][N], double V[N][N]) {
  for (int r = 0; r < N; r++)
    for (int c = 0; c < N; c++) V[r][c] = r == c ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; sweep++) {
    double off = 0.0, diag = 0.0;
    for (int r = 0; r < N; r++)
      for (int c = 0; c < N; c++) (r == c ? diag : off) += A[r][c] * A[r][c];
    if (off <= 1e-60 * diag || off == 0.0) break;
    for (int p = 0; p < N - 1; p++)
      for (int q = p + 1; q < N; q++) {
        if (A[p][q] == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < N; k++) {  // A <- A J
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < N; k++) {  // A <- J^T A
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        for (int k = 0; k < N; k++) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  }
}

}  // namespace

void sym3_eigen(const double S[6], double values[3], double vectors[3][3]) {
  double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}}, V[3][3];
  jacobi_eigen<3>(A, V);
  int order[3] = {0, 1, 2};
  for (int a = 0; a < 2; a++)
    for (int b = a + 1; b < 3; b++)
      if (A[order[b]][order[b]] < A[order[a]][order[a]]) {
        const int x = order[a];
        order[a] = order[b];
        order[b] = x;
      }
  for (int k = 0; k < 3; k++) {
    const int c = order[k];
    values[k] = A[c][c];
    const double len = std::sqrt((V[0][c] * V[0][c] + V[1][c] * V[1][c]) + V[2][c] * V[2][c]);
    for (int r = 0; r < 3; r++) vectors[k][r] = len > 0.0 ? V[r][c] / len : 0.0;
  }
}

bool rigid_from_sums(uint64_t n, const double sum_s[3], const double sum_t[3], const double cross[9], double T[16]) {
  if (n < 3) return false;
  const double inv = 1.0 / static_cast<double>(n);
  double ms[3], mt[3], S[3][3];
  for (int a = 0; a < 3; a++) ms[a] = sum_s[a] * inv, mt[a] = sum_t[a] * inv;
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) S[r][c] = cross[3 * r + c] - sum_s[r] * mt[c];  // sum (p_s - ms)[r] (p_t - mt)[c]
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++)
      if (!(S[r][c] - S[r][c] == 0.0)) return false;
  // rank: the singular values of S by one-sided Jacobi rotations (the columns are turned against each other until they are orthogonal;
  // their lengths are then the singular values) — accurate to an ulp of the greatest, which the eigenvalues of S^T S are not
  double U[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) U[r][c] = S[r][c];
  for (int sweep = 0; sweep < 64; sweep++) {
    bool turned = false;
    for (int p = 0; p < 2; p++)
      for (int q = p + 1; q < 3; q++) {
        double alpha = 0.0, beta = 0.0, gamma = 0.0;
        for (int k = 0; k < 3; k++) alpha += U[k][p] * U[k][p], beta += U[k][q] * U[k][q], gamma += U[k][p] * U[k][q];
        if (gamma == 0.0 || gamma * gamma <= 1e-32 * alpha * beta) continue;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 3; k++) {
          const double up = U[k][p], uq = U[k][q];
          U[k][p] = c * up - s * uq;
          U[k][q] = s * up + c * uq;
        }
        turned = true;
      }
    if (!turned) break;
  }
  double sv[3];
  for (int c = 0; c < 3; c++) sv[c] = std::sqrt((U[0][c] * U[0][c] + U[1][c] * U[1][c]) + U[2][c] * U[2][c]);
  for (int a = 0; a < 2; a++)
    for (int b = a + 1; b < 3; b++)
      if (sv[b] > sv[a]) {
        const double x = sv[a];
        sv[a] = sv[b];
        sv[b] = x;
      }
  if (!(sv[0] > 0.0) || !(sv[1] > 1e-12 * sv[0])) return false;
  double Nm[4][4] = {{(S[0][0] + S[1][1]) + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                     {0.0, (S[0][0] - S[1][1]) - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                     {0.0, 0.0, (-S[0][0] + S[1][1]) - S[2][2], S[1][2] + S[2][1]},
                     {0.0, 0.0, 0.0, (-S[0][0] - S[1][1]) + S[2][2]}};
  for (int r = 1; r < 4; r++)
    for (int c = 0; c < r; c++) Nm[r][c] = Nm[c][r];
  double V[4][4];
  jacobi_eigen<4>(Nm, V);
  int best = 0;
  for (int k = 1; k < 4; k++)
    if (Nm[k][k] > Nm[best][best]) best = k;
  double q[4] = {V[0][best], V[1][best], V[2][best], V[3][best]};
  const double qn = std::sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
  if (!(qn > 0.0)) return false;
  for (int k = 0; k < 4; k++) q[k] /= qn;
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double R[3][3] = {{1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)},
                          {2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)},
                          {2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)}};
  for (int k = 0; k < 16; k++) T[k] = 0.0;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * c + r] = R[r][c];
    T[12 + r] = mt[r] - ((R[r][0] * ms[0] + R[r][1] * ms[1]) + R[r][2] * ms[2]);
  }
  T[15] = 1.0;
  return true;
}

}  // namespace sga

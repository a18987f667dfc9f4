// exp(a xi) of a twist xi = (omega, v) (rotation first, util/lie.hpp:73-96) scaled by a number a, evaluated WITHOUT cancellation for every
// angle, a = 0 and |omega| = 0 included: what sga_cloud_deskew applies to every point with its own a, what
// sga_se3_exp returns at a = 1 and what sga_se3_log inverts.  With the unit axis k = omega / theta, K = skew(k) and phi = a theta,
//     R(a) = I + sin(phi) K + 2 sin^2(phi / 2) K^2
//     t(a) = a v + 2 sin^2(phi / 2) (k x v) / theta + (phi - sin(phi)) (k x (k x v)) / theta
// No coefficient is a difference of nearly equal numbers ((1 - cos)/theta^2 and (theta - sin)/theta^3 of the textbook form are: about
// 1e-6 relative at theta = 1e-5) and none is divided by phi: phi - sin(phi) is a series up to |phi| = 1 and loses less than three bits
// beyond.  Everything that depends on xi alone is formed once (TwistConst: on the host, read by a kernel with scalar loads); what is
// left for every a is one sincos, the series and a few multiplications.  theta = 0 gives k = 0, so R = I and t = a v exactly, and a = 0
// gives R = I, t = 0 exactly.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define SGA_HD __host__ __device__
#else
#define SGA_HD
#endif

namespace sga {

struct RotCoef {
  double s1, c2, f3;  // sin(phi), 1 - cos(phi), phi - sin(phi)
};
SGA_HD inline RotCoef rot_coef(double phi) {
  double sh, ch;
  sincos(0.5 * phi, &sh, &ch);
  RotCoef c;
  c.s1 = 2.0 * sh * ch;
  c.c2 = 2.0 * sh * sh;
  // phi^3 (1/3! - q/5! + q^2/7! - ... + q^8/19!), q = phi^2: at |phi| = 1 the first term left out is 6/21! = 1.2e-19 of the sum
  const double q = phi * phi;
  double s = 1.0 / 121645100408832000.0;
  s = 1.0 / 355687428096000.0 - q * s;
  s = 1.0 / 1307674368000.0 - q * s;
  s = 1.0 / 6227020800.0 - q * s;
  s = 1.0 / 39916800.0 - q * s;
  s = 1.0 / 362880.0 - q * s;
  s = 1.0 / 5040.0 - q * s;
  s = 1.0 / 120.0 - q * s;
  s = 1.0 / 6.0 - q * s;
  c.f3 = fabs(phi) <= 1.0 ? phi * q * s : phi - c.s1;  // (a NaN takes the second branch and stays one)
  return c;
}

// What exp(a xi), seen from a frame whose origin lies at o, needs of xi and o: the pose of a point P = r + o written for the record r,
//     R(a) r + (R(a) o + t(a) - o) = R(a) r + (a v + s1 a1 + c2 a2 + f3 a3),
// a1 = k x o, a2 = K^2 o + (k x v) / theta, a3 = (k x (k x v)) / theta — (R - I) o is formed from its own terms, never as R o - o.
struct TwistConst {
  double theta;
  double k[3];
  double kk[6];  // K^2 = k k^T - |k|^2 I: xx xy xz yy yz zz
  double v[3], a1[3], a2[3], a3[3];
};
inline void cross3(const double a[3], const double b[3], double out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
inline TwistConst twist_const(const double xi[6], const double o[3]) {
  TwistConst c{};
  const double m = std::fmax(std::fabs(xi[0]), std::fmax(std::fabs(xi[1]), std::fabs(xi[2])));
  if (m > 0.0) {  // |omega| = m |omega / m|: no entry's square leaves the range of a double
    const double u[3] = {xi[0] / m, xi[1] / m, xi[2] / m};
    const double nu = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
    c.theta = m * nu;
    for (int i = 0; i < 3; i++) c.k[i] = u[i] / nu;
  }
  const double* k = c.k;
  c.kk[0] = -(k[1] * k[1] + k[2] * k[2]), c.kk[1] = k[0] * k[1], c.kk[2] = k[0] * k[2];
  c.kk[3] = -(k[0] * k[0] + k[2] * k[2]), c.kk[4] = k[1] * k[2], c.kk[5] = -(k[0] * k[0] + k[1] * k[1]);
  double kv[3] = {0, 0, 0}, kkv[3] = {0, 0, 0};
  for (int i = 0; i < 3; i++) c.v[i] = xi[3 + i];
  if (c.theta > 0.0) {
    cross3(k, c.v, kv);
    cross3(k, kv, kkv);
    for (int i = 0; i < 3; i++) kv[i] /= c.theta, kkv[i] /= c.theta;
  }
  cross3(k, o, c.a1);
  c.a2[0] = (c.kk[0] * o[0] + c.kk[1] * o[1] + c.kk[2] * o[2]) + kv[0];
  c.a2[1] = (c.kk[1] * o[0] + c.kk[3] * o[1] + c.kk[4] * o[2]) + kv[1];
  c.a2[2] = (c.kk[2] * o[0] + c.kk[4] * o[1] + c.kk[5] * o[2]) + kv[2];
  for (int i = 0; i < 3; i++) c.a3[i] = kkv[i];
  return c;
}

// (R row-major, t) of exp(a xi) for the records of the frame at o
SGA_HD inline void twist_pose(const TwistConst& c, double a, double r[9], double t[3]) {
  const RotCoef f = rot_coef(a * c.theta);
  r[0] = 1.0 + f.c2 * c.kk[0];
  r[1] = f.c2 * c.kk[1] - f.s1 * c.k[2];
  r[2] = f.c2 * c.kk[2] + f.s1 * c.k[1];
  r[3] = f.c2 * c.kk[1] + f.s1 * c.k[2];
  r[4] = 1.0 + f.c2 * c.kk[3];
  r[5] = f.c2 * c.kk[4] - f.s1 * c.k[0];
  r[6] = f.c2 * c.kk[2] - f.s1 * c.k[1];
  r[7] = f.c2 * c.kk[4] + f.s1 * c.k[0];
  r[8] = 1.0 + f.c2 * c.kk[5];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = a * c.v[i] + f.s1 * c.a1[i] + f.c2 * c.a2[i] + f.f3 * c.a3[i];
}

}  // namespace sga

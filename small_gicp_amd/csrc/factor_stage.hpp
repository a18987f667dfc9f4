// The factor stage of a linearization pass in MOMENT form (pass_layout.hpp: the row): the device functions the pass kernels of
// linearize.hip share, from one pair's M' and g to the wave's fp64 row.
#pragma once
#include <utility>

#include "pass_layout.hpp"
#include "projective.hpp"

namespace sga {

template <typename Real>
__device__ __forceinline__ Sym3<Real> load_sym(const Cov8* __restrict__ c, int i) {
  const float4 a = reinterpret_cast<const float4*>(c)[2 * i];
  const float4 b = reinterpret_cast<const float4*>(c)[2 * i + 1];
  return {Real(a.x), Real(a.y), Real(a.z), Real(a.w), Real(b.x), Real(b.y)};
}

// (declared ahead of their definitions: the default arguments live here)
template <typename Real, int FACTOR, int TARGET, int PTS, bool FRESH_NN = false, bool CERT = false, bool STAGED = false>
__device__ __forceinline__ void linearize_group(const LinParams<Real>& p, int first, int stride, int limit, double* __restrict__ acc_row, int lane, unsigned long long* __restrict__ failed_masks = nullptr,
                                                const ProjView* __restrict__ proj = nullptr);
template <typename Real, int FACTOR, bool OWN_D2 = true>
__device__ __forceinline__ bool pair_moments(const LinParams<Real>& p, int i, int j, bool within_bound, Real qx, Real qy, Real qz, Real tx, Real ty, Real tz, Sym3<Real>& Mp, Real* g, Real& e, Sym3<Real>& M_out,
                                             const float4* nn_pre = nullptr);
template <typename Real, int PTS>
__device__ __forceinline__ void accumulate_moments(const Real (&P)[PTS][3], const Sym3<Real> (&Mp)[PTS], const Real (&G)[PTS][3], const Real (&E)[PTS], int inliers, double* __restrict__ acc_row, int lane);

// One correspondence the pass has kept (source point i, its target j or -1, the residual r = t_j - T p_i): fused mahalanobis, robust
// weight, the 28 values of the pair's system.  Returns whether there is a pair; caches the mahalanobis (GICP).
template <typename Real, int FACTOR>
__device__ __forceinline__ bool pair_factor(const LinParams<Real>& p, int i, int j, Real px, Real py, Real pz, Real rx, Real ry, Real rz, Real* vals, Sym3<Real>* Mp_out = nullptr, Real* g_out = nullptr) {
  const bool inlier = j >= 0;
  if (inlier) {
    Sym3<Real> M;
    if constexpr (FACTOR == SGA_GICP) {
      const Sym3<Real> Cs = load_sym<Real>(p.src_cov, i);
      const Sym3<Real> Ct = load_sym<Real>(p.tgt_cov, j);
      const Sym3<Real> RCR = rotate_sym(p.T.r, Cs);
      M = inverse_sym<Real>({Ct.xx + RCR.xx, Ct.xy + RCR.xy, Ct.xz + RCR.xz, Ct.yy + RCR.yy, Ct.yz + RCR.yz, Ct.zz + RCR.zz});
      Real* m = p.maha + static_cast<size_t>(i) * 6;
      m[0] = M.xx;
      m[1] = M.xy;
      m[2] = M.xz;
      m[3] = M.yy;
      m[4] = M.yz;
      m[5] = M.zz;
    } else if constexpr (FACTOR == SGA_PLANE_ICP) {
      const float4 nn = p.tgt_nrm[j];
      M = {Real(nn.x) * Real(nn.x), Real(0), Real(0), Real(nn.y) * Real(nn.y), Real(0), Real(nn.z) * Real(nn.z)};
    } else {
      M = {Real(1), Real(0), Real(0), Real(1), Real(0), Real(1)};
    }
    Real w = Real(1);
    if (p.robust_kind != SGA_ROBUST_NONE) {
      const Real vx = M.xx * rx + M.xy * ry + M.xz * rz, vy = M.xy * rx + M.yy * ry + M.yz * rz, vz = M.xz * rx + M.yz * ry + M.zz * rz;
      w = robust_weight<Real>(p.robust_kind, p.robust_c, Real(0.5) * (rx * vx + ry * vy + rz * vz));
    }
    pair_system<Real>(p.T.r, px, py, pz, rx, ry, rz, M, w, vals, Mp_out, g_out);
  }
  return inlier;
}

// M' and g of one correspondence (weighted by the robust kernel), its error, and whether it is an inlier; caches the mahalanobis
// matrix for the error pass.  (The direct form — the 28 values of pair_system — is pair_factor below; the per-point export uses it.)
// nn_pre (PLANE_ICP): the target normal when the caller has fetched it already (linearize_group over a flat map), else it is read here.
// OWN_D2 = false: the caller's within_bound already is the rejector's verdict on the search's own distance (a projective target)
template <typename Real, int FACTOR, bool OWN_D2>
__device__ __forceinline__ bool pair_moments(const LinParams<Real>& p, int i, int j, bool within_bound, Real qx, Real qy, Real qz, Real tx, Real ty, Real tz, Sym3<Real>& Mp, Real* g, Real& e, Sym3<Real>& M_out,
                                             const float4* nn_pre) {
  const Real rx = tx - qx, ry = ty - qy, rz = tz - qz;
  const Real d2 = rx * rx + ry * ry + rz * rz;
  const bool inlier = (j >= 0) && within_bound && (!OWN_D2 || !(d2 > p.max_sq));
  Mp = Sym3<Real>{};
  g[0] = g[1] = g[2] = Real(0);
  e = Real(0);
  if (inlier) {
    Sym3<Real> M;
    if constexpr (FACTOR == SGA_GICP) {
      const Sym3<Real> Cs = load_sym<Real>(p.src_cov, i);
      const Sym3<Real> Ct = load_sym<Real>(p.tgt_cov, j);
      const Sym3<Real> RCR = rotate_sym(p.T.r, Cs);
      M = inverse_sym<Real>({Ct.xx + RCR.xx, Ct.xy + RCR.xy, Ct.xz + RCR.xz, Ct.yy + RCR.yy, Ct.yz + RCR.yz, Ct.zz + RCR.zz});
      M_out = M;  // the caller caches it for the error pass (gicp_factor.hpp:80-89)
    } else if constexpr (FACTOR == SGA_PLANE_ICP) {
      const float4 nn = nn_pre != nullptr ? *nn_pre : p.tgt_nrm[j];
      M = {Real(nn.x) * Real(nn.x), Real(0), Real(0), Real(nn.y) * Real(nn.y), Real(0), Real(nn.z) * Real(nn.z)};
    } else {
      M = {Real(1), Real(0), Real(0), Real(1), Real(0), Real(1)};
    }
    const Real vx = M.xx * rx + M.xy * ry + M.xz * rz, vy = M.xy * rx + M.yy * ry + M.yz * rz, vz = M.xz * rx + M.yz * ry + M.zz * rz;
    const Real e0 = Real(0.5) * (rx * vx + ry * vy + rz * vz);
    const Real w = p.robust_kind != SGA_ROBUST_NONE ? robust_weight<Real>(p.robust_kind, p.robust_c, e0) : Real(1);
    const Real* R = p.T.r;
    g[0] = w * (R[0] * vx + R[3] * vy + R[6] * vz);
    g[1] = w * (R[1] * vx + R[4] * vy + R[7] * vz);
    g[2] = w * (R[2] * vx + R[5] * vy + R[8] * vz);
    Mp = rotate_sym_t(R, M);
    Mp = {w * Mp.xx, w * Mp.xy, w * Mp.xz, w * Mp.yy, w * Mp.yz, w * Mp.zz};
    e = w * e0;
  }
  return inlier;
}

// Adds the moments of PTS points per lane (zero M' / g / e for the points that are no inliers) to the wave's fp64 row in LDS.  The
// lane adds its points up in registers; the 72 fp32 sums then go through ONE transposing wave reduction (device_math.hpp:
// wave_transpose_sum, ~3 instructions per sum instead of a 6-step DPP chain each) that leaves the totals spread over the lanes —
// lane l holds the sums number `slot` and 64 + slot — and every lane adds its own two to the row.  e is summed in fp64.
// Must be called by all 64 lanes of the wave (cross-lane operations).
// Sum number s -> row column: s < 6: H_tt (15 + s); s < 9: b_t (24 + s - 6); else the error-model block (kModelOff + s - 9).
constexpr int kMomentSums = 72;
__host__ __device__ constexpr int moment_column(int s) { return s < 6 ? 15 + s : (s < 9 ? 18 + s : kModelOff - 9 + s); }

// the S-th sum of one lane's PTS points (S is a template parameter: every index below is a compile-time constant, so the 72 values
// live in registers — a run-time-indexed array of them would be placed in scratch memory)
template <typename Real, int PTS, int S>
__device__ __forceinline__ Real moment_sum(const Real (&P)[PTS][3], const Sym3<Real> (&Mp)[PTS], const Real (&G)[PTS][3]) {
  auto m6 = [&](int u, int c) -> Real { return c == 0 ? Mp[u].xx : (c == 1 ? Mp[u].xy : (c == 2 ? Mp[u].xz : (c == 3 ? Mp[u].yy : (c == 4 ? Mp[u].yz : Mp[u].zz)))); };
  Real v = Real(0);
  if constexpr (S < 6) {
#pragma unroll
    for (int u = 0; u < PTS; u++) v += m6(u, S);
  } else if constexpr (S < 9) {
#pragma unroll
    for (int u = 0; u < PTS; u++) v -= G[u][S - 6];
  } else if constexpr (S < 18) {
    constexpr int a = (S - 9) / 3, j = (S - 9) % 3;
#pragma unroll
    for (int u = 0; u < PTS; u++) v += P[u][a] * G[u][j];
  } else if constexpr (S < 36) {
    constexpr int a = (S - 18) / 6, c = (S - 18) % 6;
#pragma unroll
    for (int u = 0; u < PTS; u++) v += P[u][a] * m6(u, c);
  } else {
    constexpr int pair = (S - 36) / 6, c = (S - 36) % 6;
    constexpr int a = pair < 3 ? 0 : (pair < 5 ? 1 : 2), b = pair < 3 ? pair : (pair < 5 ? pair - 2 : 2);
#pragma unroll
    for (int u = 0; u < PTS; u++) v += (P[u][a] * P[u][b]) * m6(u, c);
  }
  return v;
}
template <typename Real, int PTS, int BASE, int... S>  // v[S] = sum number BASE + S
__device__ __forceinline__ void moment_sums(const Real (&P)[PTS][3], const Sym3<Real> (&Mp)[PTS], const Real (&G)[PTS][3], Real (&v)[sizeof...(S)], std::integer_sequence<int, S...>) {
  ((v[S] = moment_sum<Real, PTS, BASE + S>(P, Mp, G)), ...);
}

template <typename Real, int PTS>
__device__ __forceinline__ void accumulate_moments(const Real (&P)[PTS][3], const Sym3<Real> (&Mp)[PTS], const Real (&G)[PTS][3], const Real (&E)[PTS], int inliers, double* __restrict__ acc_row, int lane) {
  double es = 0.0;
#pragma unroll
  for (int u = 0; u < PTS; u++) es += static_cast<double>(E[u]);
  const double et = wave_sum_f64(es);
  if (lane == 0) {
    acc_row[27] += et;
    acc_row[28] += static_cast<double>(inliers);
  }
  if constexpr (sizeof(Real) == 4 && PTS == 1) {
    // inside the one-query-per-lane search kernels (64 VGPRs): two reductions of 36 sums each — all 72 at once do not fit the register
    // budget there, and the spills (60 bytes per lane through scratch memory) showed up as 60 MB of HBM traffic per pass
    constexpr int kHalf = kMomentSums / 2;
#pragma unroll
    for (int part = 0; part < 2; part++) {
      float v[kHalf];
      if (part == 0)
        moment_sums<float, PTS, 0>(P, Mp, G, v, std::make_integer_sequence<int, kHalf>{});
      else
        moment_sums<float, PTS, kHalf>(P, Mp, G, v, std::make_integer_sequence<int, kHalf>{});
      float lo, hi;
      int slot;
      wave_transpose_sum<kHalf>(v, lane, lo, hi, slot);
      if (slot < kHalf) acc_row[moment_column(part * kHalf + slot)] += static_cast<double>(lo);
    }
    return;
  }
  Real v[kMomentSums];
  moment_sums<Real, PTS, 0>(P, Mp, G, v, std::make_integer_sequence<int, kMomentSums>{});
  if constexpr (sizeof(Real) == 4) {
    float lo, hi;
    int slot;
    wave_transpose_sum<kMomentSums>(v, lane, lo, hi, slot);
    acc_row[moment_column(slot)] += static_cast<double>(lo);
    if (slot + 64 < kMomentSums) acc_row[moment_column(slot + 64)] += static_cast<double>(hi);
  } else {
#pragma unroll
    for (int s = 0; s < kMomentSums; s++) {
      const double t = wave_sum_f64(v[s]);
      if (lane == 0) acc_row[moment_column(s)] += t;
    }
  }
}

// The kernel's FIRST argument (a LinParams) read again from the kernel-argument segment through a pointer the compiler cannot see through:
// the scalar loads of the fields a stage uses are issued in that stage and their registers die with it.  Without this the compiler loads
// every field at the kernel's start and keeps all of them for its whole length — more than the 100 scalar registers a wave has, so it
// parks them in the lanes of vector registers and fetches them back one v_readlane at a time (certify_linearize_kernel: 448 of its ~3 200
// vector instructions per wave).  Only valid inside a kernel whose first parameter is the LinParams<Real> passed by value.
template <typename Real>
__device__ __forceinline__ const LinParams<Real>& kernarg_lin_params() {
  using Args = const __attribute__((address_space(4))) LinParams<Real>;
  Args* a = (Args*)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(a));
  return *(const LinParams<Real>*)a;
}

// The factor stage as a kernel of its own.  TARGET: 0 kd-tree (the neighbours come from the search kernel), 1 Gaussian voxel map, 2 flat voxel map, 3 projective
// search (`proj`: ann/projective_search.hpp; the lookup of these targets happens right here).  Streaming + two gathers; a lane handles PTS points (PTS x kTile consecutive points per
// workgroup step), their products are added up in registers, reduced with DPP inside the wave, in fp64 across waves.
// The factors of PTS points per lane — points first, first + stride, ... below `limit` — added to the wave's row.
// FRESH_NN: hint[] was written earlier in this very kernel (by any lane of this wave): read it past the vector L1.
// STAGED (the caller is a kernel whose first argument is `p0` itself): every stage reads the parameters it uses afresh (kernarg_lin_params).
template <typename Real, int FACTOR, int TARGET, int PTS, bool FRESH_NN, bool CERT, bool STAGED>
__device__ __forceinline__ void linearize_group(const LinParams<Real>& p0, int first, int stride, int limit, double* __restrict__ acc_row, int lane, unsigned long long* __restrict__ failed_masks,
                                                const ProjView* __restrict__ proj) {
#define SGA_STAGE_PARAMS(name) const LinParams<Real>& name = STAGED ? kernarg_lin_params<Real>() : p0
  SGA_STAGE_PARAMS(p);
  Real P[PTS][3], G[PTS][3], E[PTS];
  Sym3<Real> Mp[PTS];
  int inliers = 0;
  // The PTS points of a lane go through the stages TOGETHER — source point + neighbour index, neighbour point, covariances — so
  // that the loads of a stage are in flight at once (one latency per stage, not per point); the stores (mahalanobis cache,
  // correspondence) come after the last load, or they would pin the loads of the next point behind them.
  float4 ps4[PTS];
  int jn[PTS];
  bool act[PTS];
#pragma unroll
  for (int u = 0; u < PTS; u++) {
    const int i = first + u * stride;
    act[u] = i < limit;
    ps4[u] = act[u] ? p.src_pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    jn[u] = -1;
    if constexpr (TARGET == 0 && CERT)
      jn[u] = act[u] ? p.cert_nn[i] : -1;  // (the same array as hint[]: read through the pointer it is written through)
    else if constexpr (TARGET == 0)
      jn[u] = act[u] ? (FRESH_NN ? __hip_atomic_load(&p.hint[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : p.hint[i]) : -1;
  }
  Real Q[PTS][3], Tg[PTS][3];
  bool within[PTS];
  {
  SGA_STAGE_PARAMS(p);
#pragma unroll
  for (int u = 0; u < PTS; u++) {
    P[u][0] = ps4[u].x, P[u][1] = ps4[u].y, P[u][2] = ps4[u].z;  // multiplied by zero M' / g when the point is no inlier
    Q[u][0] = Q[u][1] = Q[u][2] = Real(0);
    if (act[u]) transform_point(p.T, P[u][0], P[u][1], P[u][2], Q[u][0], Q[u][1], Q[u][2]);
    Tg[u][0] = Tg[u][1] = Tg[u][2] = Real(0);
    within[u] = true;
    if constexpr (TARGET == 2) {
      if (act[u]) {
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
        jn[u] = flat_nearest<Real>(p.flat, p.tgt_pts, Q[u][0], Q[u][1], Q[u][2], m);
        Tg[u][0] = m.x, Tg[u][1] = m.y, Tg[u][2] = m.z;
      }
    } else if constexpr (TARGET == 3) {
      // the windowed scan of projective_search.hpp:107-140 (projective.hpp); the rejector (rejector.hpp:19-28) judges the scan's own
      // distance, in Real, so pair_moments does not measure the pair again
      if (act[u]) {
        Real d2 = Real(0);
        jn[u] = projective_nearest<Real>(*proj, p.tgt_pts, Q[u][0], Q[u][1], Q[u][2], d2);
        within[u] = jn[u] >= 0 && !(d2 > p.max_sq);
        const float4 m = jn[u] >= 0 ? p.tgt_pts[jn[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
        Tg[u][0] = m.x, Tg[u][1] = m.y, Tg[u][2] = m.z;
      }
    } else if constexpr (TARGET == 1) {
      if (act[u]) {
        if (p.vox.offsets == 1)  // (wave-uniform) the default: the query's own voxel, no distance to compare
          jn[u] = voxel_lookup<Real>(p.vox, Q[u][0], Q[u][1], Q[u][2]);
        else
          jn[u] = voxel_nearest<Real>(p.vox, p.tgt_pts, Q[u][0], Q[u][1], Q[u][2]);
      }
    }
  }
  }
  if constexpr (TARGET != 2 && TARGET != 3) {
    float4 m4[PTS];
    if constexpr (CERT && TARGET == 0) {
      // The certificate check of the warm pass (search_lane / nn_search_queue_kernel: the same arithmetic, bit for bit) on the way through:
      // both candidates of the previous pass are fetched, the nearer one (canonical rule) is the neighbour if its new distance is
      // below the exclusion radius minus the point's motion; otherwise the point is flagged for the walkers' kernel and skipped here.
      int c2[PTS];
      float rx[PTS];
      float4 m4b[PTS];
      {
        SGA_STAGE_PARAMS(p);
#pragma unroll
        for (int u = 0; u < PTS; u++) {
          const int i = first + u * stride;
          c2[u] = act[u] ? p.cert_nn2[i] : -1;
          rx[u] = act[u] ? p.cert_rex[i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < PTS; u++) {
          m4[u] = jn[u] >= 0 ? p.tgt_pts[jn[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
          m4b[u] = c2[u] >= 0 ? p.tgt_pts[c2[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
      SGA_STAGE_PARAMS(p);
#pragma unroll
      for (int u = 0; u < PTS; u++) {
        const int i = first + u * stride;
        bool failed = false;
        if (act[u]) {
          const float fx = static_cast<float>(Q[u][0]), fy = static_cast<float>(Q[u][1]), fz = static_cast<float>(Q[u][2]);
          Real ox, oy, oz;
          transform_point<Real>(p.T_prev, P[u][0], P[u][1], P[u][2], ox, oy, oz);
          const float moved = sqrtf(kd_dist2(static_cast<float>(ox), static_cast<float>(oy), static_cast<float>(oz), fx, fy, fz));
          const float d1 = jn[u] >= 0 ? kd_dist2(m4[u].x, m4[u].y, m4[u].z, fx, fy, fz) : INFINITY;
          const float d2 = c2[u] >= 0 ? kd_dist2(m4b[u].x, m4b[u].y, m4b[u].z, fx, fy, fz) : INFINITY;
          const bool swap = c2[u] >= 0 && (d2 < d1 || (d2 == d1 && c2[u] < jn[u]));  // the canonical rule: equidistant -> lower position
          const int best = swap ? c2[u] : jn[u];
          const float r = certify(rx[u], moved, best >= 0, swap ? d2 : d1, p.cert_within2, p.cert_pad);
          failed = !(r >= 0.f);
          // settled: the shrunken radius; failed: the flag of the walkers' kernel, which is also the exploration slack of the re-walk
          p.cert_rex[i] = failed ? -fminf(fmaxf(moved, p.cert_slack_min), p.cert_slack_max) : r;
          if (swap) {  // (for a walker: its seed is the nearer candidate)
            p.cert_nn[i] = c2[u];
            p.cert_nn2[i] = jn[u];
            m4[u] = m4b[u];
          }
          jn[u] = failed ? -1 : best;
        }
        const unsigned long long fm = __ballot(failed);
        if (lane == 0) {
          failed_masks[u] = fm;  // (LDS) which of this wave's 64 points of sub-step u walk
          if (fm != 0ull) p.cert_walked[i >> 6] += static_cast<uint32_t>(__popcll(fm));  // the 64 points belong to this wave: no atomic
        }
        if (failed) act[u] = false;  // the walk phase writes its correspondence
      }
    } else {
#pragma unroll
      for (int u = 0; u < PTS; u++) m4[u] = jn[u] >= 0 ? p.tgt_pts[jn[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    bool decided64[PTS];
#pragma unroll
    for (int u = 0; u < PTS; u++) decided64[u] = false;
    if constexpr (TARGET == 0 && !CERT && sizeof(Real) == 8) {
      // fp64 per-pair arithmetic: the reference compares DOUBLE distances (ann/knn_result.hpp:80-100, double queries against the stored
      // points).  The walk compared fp32 distances of the fp32-rounded query; it also kept its runner-up — the only other point that can
      // be the nearest in double when the two agree to fp32 rounding.  Both candidates are measured again here, in double, against the
      // double query: the nearer one is the correspondence (equidistant: the lower kd position, the canonical rule), and the rejector's
      // test (rejector.hpp:19-28: reject iff sq_dist > max_dist_sq) runs on that double distance.  hint[] / hint2[] / rex[] — the state of
      // the SEARCH — stay what the walk wrote.
      if (p.cert_nn2 != nullptr) {
#pragma unroll
        for (int u = 0; u < PTS; u++) {
          const int i = first + u * stride;
          if (!act[u] || jn[u] < 0) continue;
          const int j2 = p.cert_nn2[i];
          const double ax = static_cast<double>(m4[u].x) - Q[u][0], ay = static_cast<double>(m4[u].y) - Q[u][1], az = static_cast<double>(m4[u].z) - Q[u][2];
          double d1 = ax * ax + ay * ay + az * az;
          if (j2 >= 0) {
            const float4 c = p.tgt_pts[j2];
            const double bx = static_cast<double>(c.x) - Q[u][0], by = static_cast<double>(c.y) - Q[u][1], bz = static_cast<double>(c.z) - Q[u][2];
            const double d2 = bx * bx + by * by + bz * bz;
            if (d2 < d1 || (d2 == d1 && j2 < jn[u])) {
              d1 = d2;
              jn[u] = j2;
              m4[u] = c;
            }
          }
          within[u] = d1 <= p.max_sq;
          if (p.reject != nullptr) within[u] = within[u] && p.reject[__float_as_uint(ps4[u].w)] == 0;
          decided64[u] = true;
        }
      }
    }
    SGA_STAGE_PARAMS(p);
#pragma unroll
    for (int u = 0; u < PTS; u++) {
      Tg[u][0] = m4[u].x, Tg[u][1] = m4[u].y, Tg[u][2] = m4[u].z;
      if constexpr (TARGET == 0) {
        if (jn[u] >= 0 && !decided64[u]) {
          // the search reaches a little beyond the rejector (kSearchMargin) and a certified neighbour may have drifted out of
          // reach: a neighbour counts only inside the reach of a plain search, whichever way it was found
          within[u] = kd_dist2(m4[u].x, m4[u].y, m4[u].z, static_cast<float>(Q[u][0]), static_cast<float>(Q[u][1]), static_cast<float>(Q[u][2])) < p.bound2;
          if (p.reject != nullptr) within[u] = within[u] && p.reject[__float_as_uint(ps4[u].w)] == 0;
        }
      }
    }
  }
  Sym3<Real> Mh[PTS];  // the mahalanobis matrices, stored after the last load
  bool inl[PTS];
  // point-to-plane over a flat map: the normals of the PTS slots the search has just found, one 16-byte gather each, in flight together
  constexpr bool kFlatNormals = TARGET == 2 && FACTOR == SGA_PLANE_ICP;
  float4 nn4[kFlatNormals ? PTS : 1];
  if constexpr (kFlatNormals) {
    SGA_STAGE_PARAMS(p);
#pragma unroll
    for (int u = 0; u < PTS; u++) nn4[u] = act[u] && jn[u] >= 0 ? p.tgt_nrm[jn[u]] : make_float4(0.f, 0.f, 0.f, 0.f);
  }
  {
  SGA_STAGE_PARAMS(p);
#pragma unroll
  for (int u = 0; u < PTS; u++) {
    const int i = first + u * stride;
    inl[u] = false;
    Mp[u] = Sym3<Real>{};
    Mh[u] = Sym3<Real>{};
    G[u][0] = G[u][1] = G[u][2] = E[u] = Real(0);
    if (act[u]) inl[u] = pair_moments<Real, FACTOR, TARGET != 3>(p, i, jn[u], within[u], Q[u][0], Q[u][1], Q[u][2], Tg[u][0], Tg[u][1], Tg[u][2], Mp[u], G[u], E[u], Mh[u], kFlatNormals ? &nn4[u] : nullptr);
    inliers += __popcll(__ballot(inl[u]));
  }
  }
  SGA_STAGE_PARAMS(pw);
#pragma unroll
  for (int u = 0; u < PTS; u++) {
    const int i = first + u * stride;
    if (act[u]) {
      pw.corr[i] = inl[u] ? jn[u] : -1;
      if constexpr (FACTOR == SGA_GICP) {
        if (inl[u] && pw.store_maha) {  // only robust factors read it back (error kernel); otherwise it is recomputed on demand
          Real* m = pw.maha + static_cast<size_t>(i) * 6;
          m[0] = Mh[u].xx, m[1] = Mh[u].xy, m[2] = Mh[u].xz, m[3] = Mh[u].yy, m[4] = Mh[u].yz, m[5] = Mh[u].zz;
        }
      }
    }
  }
  if (inliers == 0) return;  // wave-uniform
  accumulate_moments<Real, PTS>(P, Mp, G, E, inliers, acc_row, lane);
#undef SGA_STAGE_PARAMS
}

}  // namespace sga

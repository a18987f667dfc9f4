// The search stage of a linearization pass: the device functions the pass kernels of linearize.hip share (the kernels themselves,
// and so every compile-time knob, stay there).
//
// The search: exact nearest neighbour of every transformed source point: nn[i] = its kd position (or -1 when nothing lies within the
// search bound), rex[i] = the exclusion radius the walk certifies (kd_search.hpp: every OTHER target point is farther than rex[i]).
//
// COLD pass (check = 0): the full walk for every point, seeded with the previous neighbour.
// WARM pass (check = 1): nn[] / rex[] describe the previous linearization pose T_prev.  The query has moved by
// delta = |T p - T_prev p| since; if the old neighbour is now closer than rex[i] - delta, no other point can be closer (triangle
// inequality): it is still the exact nearest neighbour, the lane shrinks the radius by delta and is done — no tree access at all.
// Only the lanes whose certificate fails walk (seeded with the old neighbour, which usually is the answer).  A small relative margin
// covers the rounding of the fp32 distances; it only ever sends a lane into the walk, never changes a result.  Late LM iterations
// move the points by micrometres: their passes are a stream over 40 bytes per point.
//
// One wave per workgroup (a finished wave frees its slot and its 4 KB of stack at once; the hardware dispatcher balances the uneven
// walks) at 7 - 8 waves per SIMD (72 / 64 VGPRs), which the walk needs.  The factor stage either follows inside the same wave
// (search_linearize_kernel: the moment form needs 42 VGPRs at one point per lane) or runs as linearize_kernel over nn[].
#pragma once
#include "pass_layout.hpp"

namespace sga {

// XCD-aware tile schedule: workgroup b runs on XCD b % 8 (observed placement; used for L2 affinity only).  Each XCD
// gets one contiguous 1/8th of the (spatially sorted) tiles so that neighbouring tiles share an L2.
__device__ __forceinline__ void tile_schedule(int num_tiles, int& first, int& stride, int& end, int nblocks = 0) {
  if (nblocks == 0) nblocks = gridDim.x;
  if (nblocks % 8 == 0 && num_tiles >= nblocks) {
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd_blocks = nblocks >> 3;
    const int t0 = static_cast<int>((static_cast<long long>(num_tiles) * xcd) >> 3);
    const int t1 = static_cast<int>((static_cast<long long>(num_tiles) * (xcd + 1)) >> 3);
    first = t0 + slot;
    stride = per_xcd_blocks;
    end = t1;
  } else {
    first = blockIdx.x;
    stride = nblocks;
    end = num_tiles;
  }
}

// exclusion radius stored per point: sqrt of the walk's exclusion bound, rounded down
__device__ __forceinline__ float rex_from_r2(float r2) { return sqrtf(r2) * 0.9999995f; }

// The walks search a little farther than the rejector reaches: a source point without a neighbour inside max_dist then carries the
// certificate "nothing within max_dist * (1 + margin)" and stays settled while it moves by less than the margin — without it those
// points (isolated clutter: the longest walks there are) would be searched again in every pass.
constexpr float kSearchMargin = 0.05f;

// Returns the shrunken radius (relative to the new pose) or a negative value if the certificate fails.
// Headroom (round 5): the DECISION asks for pad * moved metres more than the certificate needs, the radius handed on is the true one.
// A point that is sent into the walk although its certificate holds is found again exactly, so nothing but the number of walkers
// depends on it.  Why: the steps of an LM run shrink geometrically, and a certificate that survives this pass by less than the motion
// still to come fails in one of the LATE passes — where the streaming kernel pays for the tail of a single walk —
// whereas this pass walks thousands of points anyway and the re-walk (exploration slack = this pass's motion) buys a certificate that
// lasts.  Measured on C3 (profiles/r05_cert_pad.txt): walkers of the passes after 1.7 / 0.29 / 0.05 mm 14 021 / 2 625 / 413 -> 2 091 /
// 89 / 6 at pad 0.6, those passes 128 / 96 / 68 -> 92 / 78 / 62 us.  pad = 0: the plain check, bit for bit.
__device__ __forceinline__ float certify(float rex, float moved, bool has_neighbour, float d2_new, float within2, float pad) {
  const float lim = rex - moved * 1.000001f;
  const float lim_d = lim - moved * pad;
  const float lim2 = lim_d > 0.f ? lim_d * lim_d * 0.999995f : -1.f;
  const bool ok = has_neighbour ? d2_new < lim2 : lim2 > within2;  // no neighbour within reach before: still none
  return ok ? lim * 0.9999995f : -1.f;
}

// The walk of ONE source point, top-down and seeded, with the fast leaf scan (kd_search.hpp); the rare query it cannot decide (two
// candidates within 1e-6 of each other, or of the search bound) is searched again with the exact keys.  Stores nn / nn2 / rex.
// `tid` = the lane's column of kd_stack ([level][BLOCK] words): threadIdx.x in the kernels whose workgroup is BLOCK wide; a kernel that gives
// every wave of a wider workgroup its own stack passes the lane number (with threadIdx.x there, wave w's rows were shifted by w
// and a full stack of wave 3 reached past the allocation).
template <typename Real, int BLOCK>
__device__ __forceinline__ int walk_lane(const NNParams<Real>& p, int i, float fx, float fy, float fz, int seed, float slack, uint32_t* __restrict__ kd_stack, int tid) {
  KdBest nb{};
  bool exact = p.fast == 0;
  if (!exact) {
    const KdBestFast f = kd_nearest_fast<BLOCK>(p.kd, fx, fy, fz, p.bound2, seed, kd_stack, tid, slack);
    nb = f.best;
    exact = f.ambiguous;
  }
  if (exact) nb = kd_nearest<BLOCK>(p.kd, fx, fy, fz, p.bound2, seed, kd_stack, tid, slack);
  p.nn[i] = nb.idx;
  p.nn2[i] = nb.idx2;
  p.rex[i] = rex_from_r2(nb.r2);
  if (p.leaves != nullptr) p.leaves[i] = nb.leaves;
  return nb.idx;
}

// The search of ONE source point (a lane of a one-query-per-lane kernel): certificate check (warm) or walk, results stored to nn[] /
// nn2[] / rex[]; returns the neighbour's kd position or -1.  Called by every lane of the wave that holds a point (`i < n`), also
// under divergence: the wave-level steps inside kd_nearest only involve the lanes that walk.
template <typename Real, int BLOCK, bool CHECK>  // CHECK: warm pass (two instantiations: the cold one carries no certificate / margin state in registers)
__device__ __forceinline__ int search_lane(const NNParams<Real>& p, int tile, int i, const float4& ps, float fx, float fy, float fz, uint32_t* __restrict__ kd_stack) {
  int seed = p.nn[i];
  float slack = 0.f;
  if constexpr (CHECK) {
    Real ox, oy, oz;
    transform_point<Real>(p.T_prev, ps.x, ps.y, ps.z, ox, oy, oz);
    const float moved = sqrtf(kd_dist2(static_cast<float>(ox), static_cast<float>(oy), static_cast<float>(oz), fx, fy, fz));
    const int cand2 = p.nn2[i];
    float d1 = INFINITY, d2 = INFINITY;
    if (seed >= 0) {
      const float4 c = p.kd.pts[seed];
      d1 = kd_dist2(c.x, c.y, c.z, fx, fy, fz);
    }
    if (cand2 >= 0) {
      const float4 c = p.kd.pts[cand2];
      d2 = kd_dist2(c.x, c.y, c.z, fx, fy, fz);
    }
    // the nearer of the two candidates (the canonical rule again: equidistant -> lower position)
    const bool swap = cand2 >= 0 && (d2 < d1 || (d2 == d1 && cand2 < seed));
    const int best = swap ? cand2 : seed;
    const float r = certify(p.rex[i], moved, best >= 0, swap ? d2 : d1, p.within2, p.cert_pad);
    if (r >= 0.f) {
      p.rex[i] = r;
      if (swap) {
        p.nn[i] = cand2;
        p.nn2[i] = seed;
      }
      return best;
    }
    seed = best;
    // this point's certificate did not survive: walk again, and explore a margin around the new neighbour proportional to the motion,
    // so that the certificate survives the following (smaller) steps
    slack = fminf(fmaxf(moved, p.slack_min), p.slack_max);
    const unsigned long long walking = __ballot(true);
    if (threadIdx.x == __ffsll(static_cast<long long>(walking)) - 1) p.walked[tile] += static_cast<uint32_t>(__popcll(walking));  // the tile belongs to this wave: no atomic
    // A point whose certificate failed sits next to a surface (isolated points carry wide certificates and rarely fail): ring 1 of the
    // cell grid (cell_grid.hpp) settles it exactly with two dependent loads and gives the new certificate the tightest radius there is
    // (the third-nearest distance); the walk — with its exploration margin — only for what the ring does not settle.
    if (p.grid_walk & 2) {
      int g_nn, g_nn2;
      float g_rex, g_seen;
      bool g_face = false;
      // (a radius that ends at the ring's face with less than the re-walk's slack to spare is left to the walk: see certify_linearize_kernel)
      if (grid_ring1_lane(p.grid, fx, fy, fz, p.bound2, g_nn, g_nn2, g_rex, g_seen, &g_face) && !(g_face && g_nn >= 0 && (p.grid_walk & 32) && g_rex - g_seen < slack)) {
        p.nn[i] = g_nn;
        p.nn2[i] = g_nn2;
        p.rex[i] = g_rex;
        return g_nn;
      }
    }
  }
  return walk_lane<Real, BLOCK>(p, i, fx, fy, fz, seed, CHECK ? slack : 0.f, kd_stack, threadIdx.x);
}

// XCD-aware tile order: workgroup b runs on XCD b % 8 (observed placement; only speed depends on it), and the source is sorted by
// target leaf, so giving each XCD one contiguous eighth of the tiles makes its L2 hold one eighth of the target instead of all of it
__device__ __forceinline__ int search_tile_of_block(int nblk = 0) {
  if (nblk == 0) nblk = gridDim.x;
  const int per_xcd = nblk >> 3, b = blockIdx.x;
  return b < 8 * per_xcd ? (b & 7) * per_xcd + (b >> 3) : b;
}

#ifdef SGA_KD_TRIPS
static __device__ unsigned long long g_kd_wave_times[2 * 32768];  // diagnostics build: start / end (100 MHz wall clock) of every search wave
#endif

}  // namespace sga

// The occupancy grid of a mapping loop on the device: sga_occupancy_* — a dense, caller-placed volume of
// {stamp, log-odds} cells that posed scans are ray-cast into (a voxel traversal per beam: free space along the beam, an endpoint at the
// return), and the queries over it (the state of a posed cloud's points with the crop's stable compaction over the kept ones, the cell
// counts, the export of the selected cells as a cloud of cell centres, the raw arrays).  The rule is stated in include/small_gicp_amd.h and
// restated in tests/occupancy_ref.py.  Integer atomics only; every log-odds value has one writer per scan, so two runs give the same bytes.
#include "cloud_ops.hpp"
#include "notes.hpp"
#include "projective.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kOccBlock = 64;          // beams / points of a workgroup: one lane each, one wave
constexpr int kOccCellBlock = 256;     // threads of a workgroup of the kernels over cells
constexpr int kOccCellsPerBlock = 1024;  // ... and its cells: four rounds of kOccCellBlock consecutive cells
constexpr int kOccScanThreads = 1024;  // the one workgroup that turns the blocks' counts into offsets
constexpr int kOccMaxSteps = 3 * (4096 + 2);  // the longest walk of a beam within max_range (max_range / leaf <= 4096)
constexpr int kOccCounters = 8;        // the grid's counter block: words 0 .. 6 counts, word 7 the arrival counter; zero between launches

struct OccCell {
  uint32_t stamp;  // 0: never observed; else 2 epoch + (1 if the cell was an endpoint of that scan)
  float L;         // log-odds
};
static_assert(sizeof(OccCell) == 8, "a cell is 8 bytes");

// What the kernels of an integration receive (kernel arguments: read with scalar loads)
struct OccBeamArgs {
  const float4* pts;  // the scan's records
  uint32_t n;
  double oc[3];   // the scan's origin
  double R[9];    // row-major
  double q[3];    // (R o_c + t) - g
  double q0[3];   // t - g
  double go[3];   // q0 * inv_leaf: the sensor in grid coordinates
  double inv_leaf, min_range, max_range;
  OccCell* cells;
  int nx, ny, nz;
  uint32_t stamp_free;  // 2 epoch; the endpoints' stamp is one more
  float l_hit, l_miss, l_min, l_max;
  unsigned long long* counters;  // the grid's counter block, or null: no statistics
  unsigned long long* slot;      // the note the last workgroup publishes the counts in, or null: another launch follows
  unsigned long long seq;
};

__device__ __forceinline__ bool occ_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// a value the compiler may not fuse into the operation that consumes it (projective.hpp: proj_sq)
__device__ __forceinline__ double occ_rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}

// The wave's counts into the counter block (one integer atomic per wave and non-zero count); with a slot, the last workgroup to arrive
// hands the block's totals to the host (payload word k = count k), zeroes the block and publishes.  Reached by EVERY thread of the launch.
template <int K>
__device__ __forceinline__ void occ_counts(uint32_t (&c)[K], unsigned long long* __restrict__ counters, unsigned long long* __restrict__ slot, unsigned long long seq, int first = 0) {
  if (counters == nullptr) return;  // (uniform)
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c[k] += __shfl_xor(c[k], off);
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; k++)
      if (c[k] != 0u) atomicAdd(&counters[first + k], static_cast<unsigned long long>(c[k]));
  }
  if (slot == nullptr) return;  // (uniform)
  __threadfence();
  __syncthreads();
  if (threadIdx.x != 0) return;
  const unsigned arrived = __hip_atomic_fetch_add(reinterpret_cast<unsigned*>(&counters[kOccCounters - 1]), 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
  if (arrived != gridDim.x - 1) return;
  for (int k = 0; k < kOccCounters - 1; k++) {
    slot[1 + k] = __hip_atomic_load(&counters[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&counters[k], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __hip_atomic_store(&counters[kOccCounters - 1], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  note_publish(slot, seq);
}

// Step 1 and 2 of the rule (small_gicp_amd.h: sga_occupancy_integrate): 0 — the return is ignored, 1 — a hit, 2 — truncated; ge: the
// beam's end in grid coordinates
__device__ __forceinline__ int occ_beam(const OccBeamArgs& a, const float4 p, double& gx, double& gy, double& gz) {
  gx = gy = gz = 0.0;
  const double rx = static_cast<double>(p.x), ry = static_cast<double>(p.y), rz = static_cast<double>(p.z);
  const double sx = rx + a.oc[0], sy = ry + a.oc[1], sz = rz + a.oc[2];
  if (!(occ_finite(sx) && occ_finite(sy) && occ_finite(sz))) return 0;
  const double rho = sqrt((proj_sq(sx) + proj_sq(sy)) + proj_sq(sz));
  if (!occ_finite(rho) || rho < a.min_range) return 0;
  int kind = 1;
  double wx, wy, wz;
  if (rho > a.max_range) {
    kind = 2;
    const double scale = a.max_range / rho;
    const double px = sx * scale, py = sy * scale, pz = sz * scale;
    wx = ((a.R[0] * px + a.R[1] * py) + a.R[2] * pz) + a.q0[0];
    wy = ((a.R[3] * px + a.R[4] * py) + a.R[5] * pz) + a.q0[1];
    wz = ((a.R[6] * px + a.R[7] * py) + a.R[8] * pz) + a.q0[2];
  } else {
    wx = ((a.R[0] * rx + a.R[1] * ry) + a.R[2] * rz) + a.q[0];
    wy = ((a.R[3] * rx + a.R[4] * ry) + a.R[5] * rz) + a.q[1];
    wz = ((a.R[6] * rx + a.R[7] * ry) + a.R[8] * rz) + a.q[2];
  }
  // (rounded products: the walk's d = ge - go must not fuse with them under -ffp-contract=fast)
  gx = occ_rounded(wx * a.inv_leaf), gy = occ_rounded(wy * a.inv_leaf), gz = occ_rounded(wz * a.inv_leaf);
  if (!(occ_finite(gx) && occ_finite(gy) && occ_finite(gz))) return 0;  // (a pose that is no rigid motion)
  return kind;
}

__device__ __forceinline__ bool occ_inside(const OccBeamArgs& a, int cx, int cy, int cz) {
  return static_cast<unsigned>(cx) < static_cast<unsigned>(a.nx) && static_cast<unsigned>(cy) < static_cast<unsigned>(a.ny) && static_cast<unsigned>(cz) < static_cast<unsigned>(a.nz);
}
__device__ __forceinline__ OccCell* occ_cell(const OccBeamArgs& a, int cx, int cy, int cz) {
  return a.cells + ((static_cast<size_t>(cz) * static_cast<size_t>(a.ny) + static_cast<size_t>(cy)) * static_cast<size_t>(a.nx) + static_cast<size_t>(cx));
}

// A free candidate: the plain load skips the atomic where this scan has touched the cell already (stamps only grow: a stale value costs
// one atomic, never correctness); the lane that raises the stamp to 2 e is the cell's only writer of L in this launch.  1 iff it was.
__device__ __forceinline__ uint32_t occ_free(const OccBeamArgs& a, int cx, int cy, int cz) {
  if (!occ_inside(a, cx, cy, cz)) return 0u;
  OccCell* cell = occ_cell(a, cx, cy, cz);
  if (__hip_atomic_load(&cell->stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT) >= a.stamp_free) return 0u;
  const uint32_t old = atomicMax(&cell->stamp, a.stamp_free);
  if (old >= a.stamp_free) return 0u;  // (2 e: another beam was first; 2 e + 1: this scan's endpoint, left alone)
  cell->L = fmaxf(cell->L + a.l_miss, a.l_min);
  return 1u;
}

}  // namespace

// The endpoints: one lane per return.  The one lane that raises a cell's stamp to 2 e + 1 is its only writer of L in this launch.
// Counts: beams, ignored, hits, truncated (words 0 .. 3) and the cells hit (word 4).
__global__ __launch_bounds__(kOccBlock) void occupancy_hit_kernel(const OccBeamArgs a) {
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kOccBlock) + threadIdx.x;
  uint32_t c[5] = {0u, 0u, 0u, 0u, 0u};
  if (i < a.n) {
    double gx, gy, gz;
    const int kind = occ_beam(a, a.pts[i], gx, gy, gz);
    c[0] = 1u, c[1] = kind == 0 ? 1u : 0u, c[2] = kind == 1 ? 1u : 0u, c[3] = kind == 2 ? 1u : 0u;
    if (kind == 1) {
      const int cx = static_cast<int>(floor(gx)), cy = static_cast<int>(floor(gy)), cz = static_cast<int>(floor(gz));
      if (occ_inside(a, cx, cy, cz)) {
        OccCell* cell = occ_cell(a, cx, cy, cz);
        const uint32_t old = atomicMax(&cell->stamp, a.stamp_free + 1u);
        if (old < a.stamp_free + 1u) {
          cell->L = fminf(cell->L + a.l_hit, a.l_max);
          c[4] = 1u;
        }
      }
    }
  }
  occ_counts(c, a.counters, a.slot, a.seq);
}

// The free space: one lane per beam walks the cells from the sensor's to the beam's end (step 3 of the rule), after the endpoints'
// launch has finished.  The loop is counted down on the INTEGER Manhattan distance of the two cells.  Beam lengths diverge within a wave:
// accepted for this first form.  Count: the cells freed (word 5).
__global__ __launch_bounds__(kOccBlock) void occupancy_ray_kernel(const OccBeamArgs a) {
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kOccBlock) + threadIdx.x;
  uint32_t c[1] = {0u};
  double gx = 0.0, gy = 0.0, gz = 0.0;
  const int kind = i < a.n ? occ_beam(a, a.pts[i], gx, gy, gz) : 0;
  if (kind != 0) {
    int cx = static_cast<int>(floor(a.go[0])), cy = static_cast<int>(floor(a.go[1])), cz = static_cast<int>(floor(a.go[2]));
    const int ex = static_cast<int>(floor(gx)), ey = static_cast<int>(floor(gy)), ez = static_cast<int>(floor(gz));
    const double dx = gx - a.go[0], dy = gy - a.go[1], dz = gz - a.go[2];
    const double inf = static_cast<double>(INFINITY);
    // per axis: the steps left, their direction, the beam parameter of the next face and its increment
    long long remx = ex > cx ? static_cast<long long>(ex) - cx : static_cast<long long>(cx) - ex;
    long long remy = ey > cy ? static_cast<long long>(ey) - cy : static_cast<long long>(cy) - ey;
    long long remz = ez > cz ? static_cast<long long>(ez) - cz : static_cast<long long>(cz) - ez;
    const int stx = ex > cx ? 1 : (ex < cx ? -1 : 0), sty = ey > cy ? 1 : (ey < cy ? -1 : 0), stz = ez > cz ? 1 : (ez < cz ? -1 : 0);
    double tmx = stx > 0 ? (static_cast<double>(cx + 1) - a.go[0]) / dx : (stx < 0 ? (a.go[0] - static_cast<double>(cx)) / (-dx) : inf);
    double tmy = sty > 0 ? (static_cast<double>(cy + 1) - a.go[1]) / dy : (sty < 0 ? (a.go[1] - static_cast<double>(cy)) / (-dy) : inf);
    double tmz = stz > 0 ? (static_cast<double>(cz + 1) - a.go[2]) / dz : (stz < 0 ? (a.go[2] - static_cast<double>(cz)) / (-dz) : inf);
    const double tdx = stx > 0 ? 1.0 / dx : (stx < 0 ? 1.0 / (-dx) : 0.0);
    const double tdy = sty > 0 ? 1.0 / dy : (sty < 0 ? 1.0 / (-dy) : 0.0);
    const double tdz = stz > 0 ? 1.0 / dz : (stz < 0 ? 1.0 / (-dz) : 0.0);
    const long long total = remx + remy + remz;
    bool left = false;  // the rest of the walk, its end included, lies outside the box
    if (total <= kOccMaxSteps) {  // (more: no beam within max_range — a pose that is no rigid motion; nothing is touched)
      int rx = static_cast<int>(remx), ry = static_cast<int>(remy), rz = static_cast<int>(remz);
      for (int steps = static_cast<int>(total); steps > 0; steps--) {
        // an axis that is outside the box and does not come back: every cell still to come is outside
        if ((cx < 0 && (stx <= 0 || rx == 0)) || (cx >= a.nx && (stx >= 0 || rx == 0)) || (cy < 0 && (sty <= 0 || ry == 0)) || (cy >= a.ny && (sty >= 0 || ry == 0)) || (cz < 0 && (stz <= 0 || rz == 0)) ||
            (cz >= a.nz && (stz >= 0 || rz == 0))) {
          left = true;
          break;
        }
        c[0] += occ_free(a, cx, cy, cz);
        // the axis of least tmax among those with steps left, ties to the lowest axis
        const bool hx = rx > 0, hy = ry > 0, hz = rz > 0;
        const bool px = hx && (!hy || tmx <= tmy) && (!hz || tmx <= tmz);
        const bool py = !px && hy && (!hz || tmy <= tmz);
        if (px) {
          cx += stx, tmx += tdx, rx--;
        } else if (py) {
          cy += sty, tmy += tdy, ry--;
        } else {
          cz += stz, tmz += tdz, rz--;
        }
      }
      if (!left && kind == 2) c[0] += occ_free(a, cx, cy, cz);  // (the walk has ended in the beam's last cell)
    }
  }
  occ_counts(c, a.counters, a.slot, a.seq, 5);
}

namespace {

// What the kernels over a posed cloud and over the cells receive
struct OccQueryArgs {
  const float4* pts;
  uint32_t n;
  double R[9];
  double q[3];  // (R o_c + t) - g
  double inv_leaf, leaf;
  const OccCell* cells;
  unsigned long long ncells;
  int nx, ny, nz;
  double threshold;
  int mask;         // classify: keep_mask; export: which_mask
  double* flag;     // n, or null: 0.0 where the compaction keeps the point, 1.0 where it does not (held against 0.5)
  uint8_t* state_host;  // the states into a slot of the staging ring, by its device address; or null
  unsigned long long* counters;
  unsigned long long* slot;
  unsigned long long seq;
  // export
  uint32_t* blocks;  // per workgroup of kOccCellsPerBlock cells: the selected cells (count), their offset (fill)
  unsigned long long capacity;
  float4* out_pts;
  long long* index_host;
  float* L_host;
};

__device__ __forceinline__ int occ_state(const OccCell c, double threshold) { return c.stamp == 0u ? 0 : (static_cast<double>(c.L) < threshold ? 1 : 2); }

}  // namespace

// The state of every point of a posed cloud, the keep flag and the three counts; one lane per point.
__global__ __launch_bounds__(kOccBlock) void occupancy_classify_kernel(const OccQueryArgs a) {
  const uint32_t i = blockIdx.x * static_cast<uint32_t>(kOccBlock) + threadIdx.x;
  uint32_t c[3] = {0u, 0u, 0u};
  if (i < a.n) {
    const float4 p = a.pts[i];
    const double rx = static_cast<double>(p.x), ry = static_cast<double>(p.y), rz = static_cast<double>(p.z);
    const double gx = (((a.R[0] * rx + a.R[1] * ry) + a.R[2] * rz) + a.q[0]) * a.inv_leaf;
    const double gy = (((a.R[3] * rx + a.R[4] * ry) + a.R[5] * rz) + a.q[1]) * a.inv_leaf;
    const double gz = (((a.R[6] * rx + a.R[7] * ry) + a.R[8] * rz) + a.q[2]) * a.inv_leaf;
    int state = 0;
    // (the comparisons are false for a NaN, and hold the conversions inside int's range)
    if (gx >= 0.0 && gx < static_cast<double>(a.nx) && gy >= 0.0 && gy < static_cast<double>(a.ny) && gz >= 0.0 && gz < static_cast<double>(a.nz)) {
      const size_t cell = (static_cast<size_t>(static_cast<int>(gz)) * static_cast<size_t>(a.ny) + static_cast<size_t>(static_cast<int>(gy))) * static_cast<size_t>(a.nx) + static_cast<size_t>(static_cast<int>(gx));
      state = occ_state(a.cells[cell], a.threshold);
    }
    c[0] = state == 0 ? 1u : 0u, c[1] = state == 1 ? 1u : 0u, c[2] = state == 2 ? 1u : 0u;
    if (a.flag != nullptr) a.flag[i] = ((a.mask >> state) & 1) != 0 ? 0.0 : 1.0;
    if (a.state_host != nullptr) a.state_host[i] = static_cast<uint8_t>(state);
  }
  if (a.state_host != nullptr) __threadfence_system();
  occ_counts(c, a.counters, a.slot, a.seq);
}

// The cells per state (words 0 .. 2), the selected cells (word 3) and, for the export, the selected cells of every workgroup's own
// kOccCellsPerBlock consecutive cells.
__global__ __launch_bounds__(kOccCellBlock) void occupancy_count_kernel(const OccQueryArgs a) {
  __shared__ uint32_t sh_sel;
  if (threadIdx.x == 0) sh_sel = 0u;
  __syncthreads();
  uint32_t c[4] = {0u, 0u, 0u, 0u};
  const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kOccCellsPerBlock;
#pragma unroll
  for (int r = 0; r < kOccCellsPerBlock / kOccCellBlock; r++) {
    const unsigned long long cell = base + static_cast<unsigned long long>(r * kOccCellBlock) + threadIdx.x;
    if (cell < a.ncells) {
      const int state = occ_state(a.cells[cell], a.threshold);
      c[0] += state == 0 ? 1u : 0u, c[1] += state == 1 ? 1u : 0u, c[2] += state == 2 ? 1u : 0u;
      c[3] += static_cast<uint32_t>((a.mask >> state) & 1);
    }
  }
  if (a.blocks != nullptr) {
    uint32_t s = c[3];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) atomicAdd(&sh_sel, s);
    __syncthreads();
    if (threadIdx.x == 0) a.blocks[blockIdx.x] = sh_sel;
  }
  occ_counts(c, a.counters, a.slot, a.seq);
}

// The workgroups' counts become their offsets (an exclusive sum in place), by ONE workgroup: thread t sums its own run of consecutive
// entries, the runs' sums are added up in order, then every thread writes its run's offsets.
__global__ __launch_bounds__(kOccScanThreads) void occupancy_offsets_kernel(uint32_t* __restrict__ blocks, uint32_t nb) {
  __shared__ unsigned long long sh[kOccScanThreads];
  const uint32_t run = (nb + kOccScanThreads - 1) / kOccScanThreads;
  const uint32_t lo = threadIdx.x * run < nb ? threadIdx.x * run : nb, hi = lo + run < nb ? lo + run : nb;
  unsigned long long s = 0;
  for (uint32_t k = lo; k < hi; k++) s += blocks[k];
  sh[threadIdx.x] = s;
  __syncthreads();
  // (an inclusive sum over the 1024 runs, doubling strides)
  for (int off = 1; off < kOccScanThreads; off <<= 1) {
    const unsigned long long v = static_cast<int>(threadIdx.x) >= off ? sh[threadIdx.x - off] : 0ull;
    __syncthreads();
    sh[threadIdx.x] += v;
    __syncthreads();
  }
  unsigned long long at = sh[threadIdx.x] - s;
  for (uint32_t k = lo; k < hi; k++) {
    const uint32_t v = blocks[k];
    blocks[k] = static_cast<uint32_t>(at < 0xffffffffull ? at : 0xffffffffull);  // (beyond any capacity the fill writes at)
    at += v;
  }
}

// The selected cells in ascending linear index: the cell's rank is its workgroup's offset plus its rank inside the workgroup; entries
// below the capacity are written — the centre's record, the index, the log-odds.
__global__ __launch_bounds__(kOccCellBlock) void occupancy_fill_kernel(const OccQueryArgs a) {
  __shared__ uint32_t sh_wave[kOccCellBlock / 64];
  const unsigned long long base = static_cast<unsigned long long>(blockIdx.x) * kOccCellsPerBlock;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned long long at = a.blocks[blockIdx.x];
  for (int r = 0; r < kOccCellsPerBlock / kOccCellBlock; r++) {
    const unsigned long long cell = base + static_cast<unsigned long long>(r * kOccCellBlock) + threadIdx.x;
    OccCell v{0u, 0.f};
    bool sel = false;
    if (cell < a.ncells) {
      v = a.cells[cell];
      sel = ((a.mask >> occ_state(v, a.threshold)) & 1) != 0;
    }
    const unsigned long long ballot = __ballot(sel);
    const uint32_t before = static_cast<uint32_t>(__popcll(ballot & ((1ull << lane) - 1ull)));
    if (lane == 0) sh_wave[wave] = static_cast<uint32_t>(__popcll(ballot));
    __syncthreads();
    uint32_t waves_before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kOccCellBlock / 64; w++) {
      waves_before += w < wave ? sh_wave[w] : 0u;
      all += sh_wave[w];
    }
    __syncthreads();
    const unsigned long long pos = at + waves_before + before;
    if (sel && pos < a.capacity) {
      const unsigned long long plane = static_cast<unsigned long long>(a.nx) * static_cast<unsigned long long>(a.ny);
      const unsigned long long z = cell / plane, rest = cell - z * plane, y = rest / static_cast<unsigned long long>(a.nx), x = rest - y * static_cast<unsigned long long>(a.nx);
      float4 rec;
      rec.x = static_cast<float>((static_cast<double>(x) + 0.5) * a.leaf);
      rec.y = static_cast<float>((static_cast<double>(y) + 0.5) * a.leaf);
      rec.z = static_cast<float>((static_cast<double>(z) + 0.5) * a.leaf);
      rec.w = __uint_as_float(static_cast<uint32_t>(pos));
      if (a.out_pts != nullptr) a.out_pts[pos] = rec;
      if (a.index_host != nullptr) a.index_host[pos] = static_cast<long long>(cell);
      if (a.L_host != nullptr) a.L_host[pos] = v.L;
    }
    at += all;
  }
  if (a.index_host != nullptr || a.L_host != nullptr) __threadfence_system();
}

}  // namespace sga

struct sga_occupancy {
  int device = 0;
  mutable sga::Ready ready;  // recorded behind EVERY call that touches the grid: an integration returns with its kernels in flight
  sga_occupancy_params params{};
  size_t cells = 0;
  double inv_leaf = 0.0;
  uint32_t epoch = 0;
  sga::DevBuf<sga::OccCell> grid;
  sga::DevBuf<unsigned long long> counters;
};

namespace sga {
namespace {

inline bool is_finite(double v) { return v - v == 0.0; }
inline void count_wait() { count_launch(Chain::OccupancyWait); }

int occupancy_params_check(const sga_occupancy_params& p) {
  for (int k = 0; k < 3; k++)
    if (!is_finite(p.origin[k])) return fail(SGA_ERR_INVALID, "occupancy: origin has a non-finite entry");
  if (!is_finite(p.leaf) || !(p.leaf > 0.0)) return fail(SGA_ERR_INVALID, "occupancy: leaf must be finite and > 0");
  unsigned long long cells = 1;
  for (int k = 0; k < 3; k++) {
    if (p.dims[k] < 1) return fail(SGA_ERR_INVALID, "occupancy: dims %d x %d x %d: each must be >= 1", p.dims[0], p.dims[1], p.dims[2]);
    cells *= static_cast<unsigned long long>(p.dims[k]);  // (at most 2^27 * 2^31 before the test below)
    if (cells > (1ull << 27)) return fail(SGA_ERR_INVALID, "occupancy: dims %d x %d x %d have more than 2^27 cells", p.dims[0], p.dims[1], p.dims[2]);
  }
  const float l[4] = {p.l_hit, p.l_miss, p.l_min, p.l_max};
  for (int k = 0; k < 4; k++)
    if (!is_finite(static_cast<double>(l[k]))) return fail(SGA_ERR_INVALID, "occupancy: l_hit, l_miss, l_min and l_max must be finite");
  if (!(p.l_hit > 0.f)) return fail(SGA_ERR_INVALID, "occupancy: l_hit must be > 0");
  if (!(p.l_miss < 0.f)) return fail(SGA_ERR_INVALID, "occupancy: l_miss must be < 0");
  if (!(p.l_min < p.l_max)) return fail(SGA_ERR_INVALID, "occupancy: l_min must be below l_max");
  return SGA_OK;
}

int occupancy_pose_check(const double* T) {
  for (int k = 0; T != nullptr && k < 16; k++)
    if (!is_finite(T[k])) return fail(SGA_ERR_INVALID, "occupancy: T has a non-finite entry");
  return SGA_OK;
}

int occupancy_threshold_check(double threshold) { return threshold != threshold ? fail(SGA_ERR_INVALID, "occupancy: threshold is NaN") : SGA_OK; }

// R (row-major), q = (R o_c + t) - g and q0 = t - g of a pose (column-major, or null: the identity), formed once in double
void occupancy_pose(const sga_occupancy* grid, const double* T, const double oc[3], double R[9], double q[3], double q0[3]) {
  for (int k = 0; k < 3; k++) {
    for (int j = 0; j < 3; j++) R[3 * k + j] = T ? T[4 * j + k] : (j == k ? 1.0 : 0.0);
    const double t = T ? T[12 + k] : 0.0;
    const double ro = (R[3 * k] * oc[0] + R[3 * k + 1] * oc[1]) + R[3 * k + 2] * oc[2];
    q[k] = (ro + t) - grid->params.origin[k];
    q0[k] = t - grid->params.origin[k];
  }
}

// behind every call that touches the grid, whatever the context's mode: a call on another context orders itself behind it (wait_ready)
int occupancy_touched(sga_context* ctx, const sga_occupancy* grid) {
  Ready& r = grid->ready;
  if (!r.event) SGA_HIP(hipEventCreateWithFlags(&r.event, hipEventDisableTiming));
  SGA_HIP(hipEventRecord(r.event, ctx->stream));
  r.stream = ctx->stream;
  r.pending = true;
  return SGA_OK;
}

void occupancy_query_args(const sga_occupancy* grid, double threshold, int mask, OccQueryArgs* a) {
  std::memset(a, 0, sizeof(*a));
  a->inv_leaf = grid->inv_leaf, a->leaf = grid->params.leaf;
  a->cells = grid->grid.p, a->ncells = grid->cells;
  a->nx = grid->params.dims[0], a->ny = grid->params.dims[1], a->nz = grid->params.dims[2];
  a->threshold = threshold, a->mask = mask;
  a->counters = grid->counters.p;
}

inline unsigned occupancy_cell_blocks(const sga_occupancy* grid) { return static_cast<unsigned>((grid->cells + kOccCellsPerBlock - 1) / kOccCellsPerBlock); }

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_occupancy_params_default(sga_occupancy_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->l_hit = 0.85f, p->l_miss = -0.4f, p->l_min = -2.0f, p->l_max = 3.5f;
}

int sga_occupancy_create(sga_context* ctx, const sga_occupancy_params* params, sga_occupancy** out) {
  if (out) *out = nullptr;
  if (!ctx || !params || !out) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(occupancy_params_check(*params));
  SGA_ENTER(ctx);
  auto grid = std::make_unique<sga_occupancy>();
  grid->device = ctx->device;
  grid->params = *params;
  grid->params.reserved = 0;
  grid->cells = static_cast<size_t>(params->dims[0]) * static_cast<size_t>(params->dims[1]) * static_cast<size_t>(params->dims[2]);
  grid->inv_leaf = 1.0 / params->leaf;
  SGA_TRY(grid->grid.alloc(grid->cells));
  SGA_TRY(grid->counters.alloc(kOccCounters));
  count_launch(Chain::Occupancy);
  SGA_HIP(hipMemsetAsync(grid->grid.p, 0, grid->cells * sizeof(OccCell), ctx->stream));
  count_launch(Chain::Occupancy);
  SGA_HIP(hipMemsetAsync(grid->counters.p, 0, kOccCounters * sizeof(unsigned long long), ctx->stream));
  SGA_TRY(occupancy_touched(ctx, grid.get()));
  *out = grid.release();
  return SGA_OK;
}

int sga_occupancy_destroy(sga_occupancy* grid) {
  delete grid;
  return SGA_OK;
}

int sga_occupancy_get(const sga_occupancy* grid, sga_occupancy_params* params, uint64_t* epoch) {
  if (!grid || (!params && !epoch)) return fail(SGA_ERR_INVALID, "null argument");
  if (params) *params = grid->params;
  if (epoch) *epoch = grid->epoch;
  return SGA_OK;
}

int sga_occupancy_clear(sga_context* ctx, sga_occupancy* grid) {
  if (!ctx || !grid) return fail(SGA_ERR_INVALID, "null argument");
  // ---- (from here on the handles are read)
  if (grid->device != ctx->device) return fail(SGA_ERR_INVALID, "the grid lives on another device");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, grid->ready));
  count_launch(Chain::Occupancy);
  SGA_HIP(hipMemsetAsync(grid->grid.p, 0, grid->cells * sizeof(OccCell), ctx->stream));
  grid->epoch = 0;
  return occupancy_touched(ctx, grid);
}

int sga_occupancy_integrate(sga_context* ctx, sga_occupancy* grid, const sga_cloud* scan, const double T[16], double min_range, double max_range, int mode, sga_occupancy_scan_stats* stats) {
  if (!ctx || !grid || !scan) return fail(SGA_ERR_INVALID, "null argument");
  if (!is_finite(min_range) || min_range < 0.0) return fail(SGA_ERR_INVALID, "occupancy: min_range must be finite and >= 0");
  if (!is_finite(max_range) || !(max_range >= min_range)) return fail(SGA_ERR_INVALID, "occupancy: max_range must be finite and >= min_range");
  if (mode != 0 && mode != 1) return fail(SGA_ERR_INVALID, "occupancy: mode %d is not 0 (free space and endpoints) or 1 (endpoints only)", mode);
  SGA_TRY(occupancy_pose_check(T));
  // ---- (from here on the handles are read)
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (grid->device != ctx->device) return fail(SGA_ERR_INVALID, "the grid lives on another device");
  if (scan->device != ctx->device) return fail(SGA_ERR_INVALID, "scan lives on another device");
  const size_t n = scan->n;
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many scan points (%zu; limit 2^31-1)", n);
  if (!(max_range * grid->inv_leaf <= 4096.0)) return fail(SGA_ERR_INVALID, "occupancy: max_range %g is more than 4096 cells of %g", max_range, grid->params.leaf);
  if (grid->epoch >= 0x7fffffffu) return fail(SGA_ERR_INVALID, "occupancy: the grid has seen 2^31-1 scans; clear it");
  OccBeamArgs a;
  std::memset(&a, 0, sizeof(a));
  occupancy_pose(grid, T, scan->origin, a.R, a.q, a.q0);
  // the box against the sensor: farther than max_range (or not comparable: an overflow), and no beam reaches it
  double d2 = 0.0;
  for (int k = 0; k < 3; k++) {
    a.oc[k] = scan->origin[k];
    a.go[k] = a.q0[k] * grid->inv_leaf;
    const double hi = static_cast<double>(grid->params.dims[k]) * grid->params.leaf;  // the box's extent along k
    const double d = a.q0[k] < 0.0 ? -a.q0[k] : (a.q0[k] > hi ? a.q0[k] - hi : 0.0);
    d2 += d * d;
  }
  const bool reachable = d2 <= max_range * max_range;  // (false for a NaN)
  if (stats) stats->beams = n;
  if (n == 0 || !reachable) {  // the epoch advances; nothing is enqueued
    grid->epoch++;
    return SGA_OK;
  }
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, grid->ready));
  SGA_TRY(wait_ready(ctx, scan->ready));  // made on another context that returned before its kernels had run
  grid->epoch++;
  a.pts = scan->pts.p, a.n = static_cast<uint32_t>(n);
  a.inv_leaf = grid->inv_leaf, a.min_range = min_range, a.max_range = max_range;
  a.cells = grid->grid.p;
  a.nx = grid->params.dims[0], a.ny = grid->params.dims[1], a.nz = grid->params.dims[2];
  a.stamp_free = 2u * grid->epoch;
  a.l_hit = grid->params.l_hit, a.l_miss = grid->params.l_miss, a.l_min = grid->params.l_min, a.l_max = grid->params.l_max;
  a.counters = stats ? grid->counters.p : nullptr;
  unsigned long long* note = nullptr;
  const unsigned long long seq = stats ? note_begin(ctx, &note) : 0ull;
  const dim3 blocks(static_cast<unsigned>((n + kOccBlock - 1) / kOccBlock));
  a.slot = mode == 1 ? note : nullptr, a.seq = seq;
  count_launch(Chain::Occupancy);
  hipLaunchKernelGGL(occupancy_hit_kernel, blocks, dim3(kOccBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  if (mode == 0) {
    a.slot = note;
    count_launch(Chain::Occupancy);
    hipLaunchKernelGGL(occupancy_ray_kernel, blocks, dim3(kOccBlock), 0, ctx->stream, a);
    SGA_HIP(hipGetLastError());
  }
  SGA_TRY(occupancy_touched(ctx, grid));
  if (stats) {
    unsigned long long payload[kNoteWords - 1];
    count_wait();
    SGA_TRY(note_wait(ctx, seq, payload));  // the call's one wait
    stats->beams = static_cast<size_t>(payload[0]), stats->ignored = static_cast<size_t>(payload[1]), stats->hits = static_cast<size_t>(payload[2]);
    stats->truncated = static_cast<size_t>(payload[3]), stats->cells_hit = static_cast<size_t>(payload[4]), stats->cells_freed = static_cast<size_t>(payload[5]);
  }
  return SGA_OK;
}

int sga_occupancy_classify(sga_context* ctx, const sga_occupancy* grid, const sga_cloud* cloud, const double T[16], double threshold, int keep_mask, uint8_t* state, int64_t* kept, sga_occupancy_counts* counts,
                           sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !grid || !cloud) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(occupancy_threshold_check(threshold));
  if (keep_mask < 0 || keep_mask > 7) return fail(SGA_ERR_INVALID, "occupancy: keep_mask %d is outside 0 .. 7 (bit 0 unknown, bit 1 free, bit 2 occupied)", keep_mask);
  if (keep_mask == 0 && out != nullptr) return fail(SGA_ERR_INVALID, "occupancy: keep_mask is 0 but an output cloud is asked for");
  if (keep_mask != 0 && out == nullptr) return fail(SGA_ERR_INVALID, "occupancy: keep_mask is %d but there is no place for the output cloud", keep_mask);
  if (keep_mask == 0 && kept != nullptr) return fail(SGA_ERR_INVALID, "occupancy: kept is given but keep_mask is 0");
  SGA_TRY(occupancy_pose_check(T));
  // ---- (from here on the handles are read)
  if (counts) std::memset(counts, 0, sizeof(*counts));
  if (grid->device != ctx->device) return fail(SGA_ERR_INVALID, "the grid lives on another device");
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  const size_t n = cloud->n;
  if (n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", n);
  if (counts) counts->epoch = grid->epoch;
  CropStat cs{nullptr, nullptr, 0.5, Chain::Occupancy, true};  // the states alone decide: a non-finite record is unknown, and kept with bit 0
  if (n == 0) return out ? cloud_crop_stat(ctx, cloud, cs, kept, out) : SGA_OK;  // an empty cloud, zeroed counts; nothing is enqueued
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, grid->ready));
  SGA_TRY(wait_ready(ctx, cloud->ready));
  DevBuf<double> flag;  // lives to the end of the call (then: the stream's free list)
  if (out) SGA_TRY(flag.alloc(n));
  // the counts and the states leave through ONE slot of the staging ring: word 0 the publication, words 1 .. 7 the counts, then the states
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, kNoteWords * 8 + (state != nullptr ? (n + 7) / 8 * 8 : 0), &slot));
  unsigned long long* slot_dev = static_cast<unsigned long long*>(slot->dev);
  OccQueryArgs a;
  occupancy_query_args(grid, threshold, keep_mask, &a);
  double q0[3];
  occupancy_pose(grid, T, cloud->origin, a.R, a.q, q0);
  a.pts = cloud->pts.p, a.n = static_cast<uint32_t>(n);
  a.flag = flag.p;
  a.state_host = state != nullptr ? reinterpret_cast<uint8_t*>(slot_dev + kNoteWords) : nullptr;
  a.slot = slot_dev, a.seq = 1ull;
  count_launch(Chain::Occupancy);
  hipLaunchKernelGGL(occupancy_classify_kernel, dim3(static_cast<unsigned>((n + kOccBlock - 1) / kOccBlock)), dim3(kOccBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  SGA_TRY(occupancy_touched(ctx, grid));  // (the counter block is the grid's)
  sga_cloud* made = nullptr;
  if (out) {
    cs.d = flag.p;
    count_wait();
    SGA_TRY(cloud_crop_stat(ctx, cloud, cs, kept, &made));  // (its wait shows that everything above has run)
  } else {
    count_wait();
    SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait: the counts are in the slot
  }
  const unsigned long long* host = static_cast<const unsigned long long*>(slot->host);
  if (counts) {
    counts->total = n;
    counts->unknown = static_cast<size_t>(host[1]), counts->free = static_cast<size_t>(host[2]), counts->occupied = static_cast<size_t>(host[3]);
  }
  if (state) std::memcpy(state, host + kNoteWords, n);
  if (out) *out = made;
  return SGA_OK;
}

int sga_occupancy_stats(sga_context* ctx, const sga_occupancy* grid, double threshold, sga_occupancy_counts* counts) {
  if (!ctx || !grid || !counts) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(occupancy_threshold_check(threshold));
  // ---- (from here on the handles are read)
  std::memset(counts, 0, sizeof(*counts));
  if (grid->device != ctx->device) return fail(SGA_ERR_INVALID, "the grid lives on another device");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, grid->ready));
  OccQueryArgs a;
  occupancy_query_args(grid, threshold, 0, &a);
  a.seq = note_begin(ctx, &a.slot);
  count_launch(Chain::Occupancy);
  hipLaunchKernelGGL(occupancy_count_kernel, dim3(occupancy_cell_blocks(grid)), dim3(kOccCellBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  SGA_TRY(occupancy_touched(ctx, grid));
  unsigned long long payload[kNoteWords - 1];
  count_wait();
  SGA_TRY(note_wait(ctx, a.seq, payload));  // the call's one wait
  counts->total = grid->cells, counts->epoch = grid->epoch;
  counts->unknown = static_cast<size_t>(payload[0]), counts->free = static_cast<size_t>(payload[1]), counts->occupied = static_cast<size_t>(payload[2]);
  return SGA_OK;
}

int sga_occupancy_export(sga_context* ctx, const sga_occupancy* grid, double threshold, int which_mask, size_t capacity, int64_t* indices, float* log_odds, size_t* count, sga_cloud** out) {
  if (out) *out = nullptr;
  if (!ctx || !grid || !count) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(occupancy_threshold_check(threshold));
  if (which_mask < 1 || which_mask > 7) return fail(SGA_ERR_INVALID, "occupancy: which_mask %d is outside 1 .. 7 (bit 0 unknown, bit 1 free, bit 2 occupied)", which_mask);
  // ---- (from here on the handles are read)
  *count = 0;
  if (grid->device != ctx->device) return fail(SGA_ERR_INVALID, "the grid lives on another device");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, grid->ready));
  const unsigned nb = occupancy_cell_blocks(grid);
  DevBuf<uint32_t> blocks;  // lives to the end of the call (then: the stream's free list)
  SGA_TRY(blocks.alloc(nb));
  OccQueryArgs a;
  occupancy_query_args(grid, threshold, which_mask, &a);
  a.blocks = blocks.p;
  a.seq = note_begin(ctx, &a.slot);
  count_launch(Chain::Occupancy);
  hipLaunchKernelGGL(occupancy_count_kernel, dim3(nb), dim3(kOccCellBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  SGA_TRY(occupancy_touched(ctx, grid));
  unsigned long long payload[kNoteWords - 1];
  count_wait();
  SGA_TRY(note_wait(ctx, a.seq, payload));  // the first wait: the count sizes the outputs
  const size_t total = static_cast<size_t>(payload[3]), m = total < capacity ? total : capacity;
  std::unique_ptr<sga_cloud> made;
  if (out) SGA_TRY(cloud_make(ctx, grid->params.origin, m, false, false, &made));
  if (m > 0 && (out || indices || log_odds)) {
    const size_t i_bytes = indices ? m * sizeof(int64_t) : 0, l_bytes = log_odds ? (m * sizeof(float) + 7) / 8 * 8 : 0;
    sga_context::StageSlot* slot = nullptr;
    if (i_bytes + l_bytes > 0) SGA_TRY(stage_acquire(ctx, i_bytes + l_bytes, &slot));
    a.slot = nullptr, a.counters = nullptr;
    a.capacity = m;
    a.out_pts = made ? made->pts.p : nullptr;
    a.index_host = indices ? static_cast<long long*>(slot->dev) : nullptr;
    a.L_host = log_odds ? reinterpret_cast<float*>(static_cast<unsigned char*>(slot->dev) + i_bytes) : nullptr;
    count_launch(Chain::Occupancy);
    hipLaunchKernelGGL(occupancy_offsets_kernel, dim3(1), dim3(kOccScanThreads), 0, ctx->stream, blocks.p, nb);
    SGA_HIP(hipGetLastError());
    count_launch(Chain::Occupancy);
    hipLaunchKernelGGL(occupancy_fill_kernel, dim3(nb), dim3(kOccCellBlock), 0, ctx->stream, a);
    SGA_HIP(hipGetLastError());
    if (slot != nullptr || !ctx->stream_ordered) {
      count_wait();
      SGA_HIP(hipStreamSynchronize(ctx->stream));  // the second wait: the fill has run
    }
    if (indices) std::memcpy(indices, slot->host, i_bytes);
    if (log_odds) std::memcpy(log_odds, static_cast<const unsigned char*>(slot->host) + i_bytes, m * sizeof(float));
    if (made) SGA_TRY(mark_ready(ctx, made->ready));
  }
  *count = total;
  if (out) *out = made.release();
  return SGA_OK;
}

int sga_occupancy_download(sga_context* ctx, const sga_occupancy* grid, uint32_t* stamp, float* log_odds) {
  if (!ctx || !grid || (!stamp && !log_odds)) return fail(SGA_ERR_INVALID, "null argument");
  // ---- (from here on the handles are read)
  if (grid->device != ctx->device) return fail(SGA_ERR_INVALID, "the grid lives on another device");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, grid->ready));
  constexpr size_t kChunk = 1u << 20;  // cells per copy
  std::vector<OccCell> host(grid->cells < kChunk ? grid->cells : kChunk);
  for (size_t first = 0; first < grid->cells; first += kChunk) {
    const size_t m = grid->cells - first < kChunk ? grid->cells - first : kChunk;
    SGA_HIP(hipMemcpyAsync(host.data(), grid->grid.p + first, m * sizeof(OccCell), hipMemcpyDeviceToHost, ctx->stream));
    count_wait();
    SGA_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < m; k++) {
      if (stamp) stamp[first + k] = host[k].stamp;
      if (log_odds) log_odds[first + k] = host[k].L;
    }
  }
  return SGA_OK;
}

int sga_debug_occupancy_launches(unsigned long long* launches) { return report_launches(Chain::Occupancy, launches); }
int sga_debug_occupancy_waits(unsigned long long* waits) { return report_launches(Chain::OccupancyWait, waits); }

}  // extern "C"

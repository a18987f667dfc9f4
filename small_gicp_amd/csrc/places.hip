// Place recognition on the device: the Scan Context descriptor of a cloud (a polar rings x sectors image of the
// greatest height per cell, by an atomicMax on the bits of the non-negative fp32 value, first in LDS, then one global atomic per non-zero
// cell: the pattern of cloud_visibility.hip's range image), the database of descriptors with their column norms, the exhaustive search
// (every candidate at every column shift, a workgroup per entry) and the selection of the k best.  The rule is stated in
// include/small_gicp_amd.h and restated in tests/place_ref.py.  Double arithmetic from the fp32 records, integer atomics only, every
// sum in a fixed order: two calls give the same bytes.
#include "cloud_ops.hpp"

#include <cmath>
#include <memory>

namespace sga {
namespace {

constexpr int kPlBlock = 256;
constexpr uint32_t kPlPointsPerBlock = 2048;  // records of a descriptor workgroup: 8 per thread, so that the image is zeroed and handed over once per 2048 records
constexpr int kPlMaxRings = 64, kPlMaxSectors = 256, kPlMaxCells = 4096, kPlMaxK = 32;
constexpr int kPlSlices = 4;  // the columns j of a shift are summed in four fixed slices, which meet in order
constexpr size_t kPlInitialCapacity = 64;

// The polar grid and the frame (kernel arguments: read with scalar loads)
struct PlGrid {
  int R, S;
  double L, height;
  double origin[3], center[3];  // p = (record + origin) - center
};

__device__ __forceinline__ bool pl_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// The cell and the value of a record, stated once (small_gicp_amd.h: place recognition); false: the record is skipped.  0 <= cell < R S.
__device__ __forceinline__ bool pl_cell(const PlGrid& g, const float4 p, int& cell, float& v) {
  const double px = (static_cast<double>(p.x) + g.origin[0]) - g.center[0];
  const double py = (static_cast<double>(p.y) + g.origin[1]) - g.center[1];
  const double pz = (static_cast<double>(p.z) + g.origin[2]) - g.center[2];
  if (!(pl_finite(px) && pl_finite(py) && pl_finite(pz))) return false;
  const double rho = sqrt(px * px + py * py);
  if (!(rho < g.L)) return false;
  const double rf = floor(rho / g.L * static_cast<double>(g.R));
  const int ring = rf >= static_cast<double>(g.R) ? g.R - 1 : (rf > 0.0 ? static_cast<int>(rf) : 0);
  double theta = atan2(py, px);
  if (theta < 0.0) theta += 2.0 * M_PI;
  const double sf = floor(theta / (2.0 * M_PI) * static_cast<double>(g.S));
  const int sector = sf >= static_cast<double>(g.S) ? g.S - 1 : (sf > 0.0 ? static_cast<int>(sf) : 0);  // (keeps the index inside the image whatever atan2 returns)
  const double h = pz + g.height;
  v = h > 0.0 ? static_cast<float>(h) : 0.f;  // (never -0: the bits of the values order as the values)
  cell = ring * g.S + sector;
  return true;
}

}  // namespace

// The descriptor: a workgroup takes kPlPointsPerBlock records into an image in LDS, then raises the cells of `img` (zeroed by the fill
// ahead of this launch) that it found non-zero.  Non-negative floats order as their bits, and a maximum does not depend on the order
// in which its operands arrive.
__global__ __launch_bounds__(kPlBlock) void places_descriptor_kernel(const float4* __restrict__ pts, uint32_t n, const PlGrid g, uint32_t* __restrict__ img) {
  __shared__ uint32_t sh[kPlMaxCells];
  const int cells = g.R * g.S;  // <= kPlMaxCells (place_params_check)
  for (int c = threadIdx.x; c < cells; c += kPlBlock) sh[c] = 0u;
  __syncthreads();
  const uint32_t begin = blockIdx.x * kPlPointsPerBlock;  // (n < 2^31: no wrap)
  const uint32_t end = n - begin < kPlPointsPerBlock ? n : begin + kPlPointsPerBlock;
  for (uint32_t i = begin + threadIdx.x; i < end; i += kPlBlock) {
    int c;
    float v;
    if (pl_cell(g, pts[i], c, v) && v > 0.f) atomicMax(&sh[c], __float_as_uint(v));
  }
  __syncthreads();
  for (int c = threadIdx.x; c < cells; c += kPlBlock) {
    const uint32_t b = sh[c];
    if (b != 0u) atomicMax(&img[c], b);
  }
}

// The column norms of an image, one thread per column, rings ascending; dst_img != src: the image is copied as well (an image that came
// through the staging ring).  One workgroup.
__global__ __launch_bounds__(kPlBlock) void places_norms_kernel(const float* __restrict__ src, float* __restrict__ dst_img, double* __restrict__ dst_norm, int R, int S) {
  const int j = threadIdx.x;
  if (j < S) {
    double s = 0.0;
    for (int r = 0; r < R; r++) {
      const double x = static_cast<double>(src[r * S + j]);
      s += x * x;
    }
    dst_norm[j] = sqrt(s);
  }
  if (dst_img != src)
    for (int c = threadIdx.x; c < R * S; c += kPlBlock) dst_img[c] = src[c];
}

namespace {

// An entry of the database: S doubles (the column norms), then R x S floats (the image); `stride` bytes, a multiple of 8
struct PlMatchArgs {
  const float* q;                // the query image: scratch memory, or a slot of the staging ring by its device address
  const unsigned char* entries;  // the database's first candidate
  size_t stride;
  uint32_t count;
  int R, S;
  double* d;  // count: what the selection reads
  int* shift;
  double* d_host;  // the same into the staging ring, or null
  int* shift_host;
};

// (d, i) < (e, j) in the order of the result: ascending distance, then ascending index.  No distance is NaN.
__device__ __forceinline__ bool pl_before(double d, unsigned i, double e, unsigned j) { return d < e || (d == e && i < j); }

}  // namespace

// The search: workgroup e compares the query with candidate e at every shift.  The query, the entry and both norms sit in LDS; the
// entry is read once.  Work item (slice, s) adds the terms of its quarter of the columns j, ascending; thread s then adds the four
// slices in order, and wave 0 takes the least d(s), ties to the lowest s.
__global__ __launch_bounds__(kPlBlock) void places_match_kernel(const PlMatchArgs a) {
  __shared__ float q[kPlMaxCells], c[kPlMaxCells];
  __shared__ double nq[kPlMaxSectors], nc[kPlMaxSectors];
  __shared__ double part[kPlSlices][kPlMaxSectors];
  __shared__ int cnt[kPlSlices][kPlMaxSectors];
  const int R = a.R, S = a.S, cells = R * S, tid = threadIdx.x;
  const unsigned char* entry = a.entries + static_cast<size_t>(blockIdx.x) * a.stride;
  const double* __restrict__ enorm = reinterpret_cast<const double*>(entry);
  const float* __restrict__ eimg = reinterpret_cast<const float*>(entry + static_cast<size_t>(S) * sizeof(double));
  for (int i = tid; i < cells; i += kPlBlock) q[i] = a.q[i], c[i] = eimg[i];
  if (tid < S) nc[tid] = enorm[tid];
  __syncthreads();
  if (tid < S) {
    double s = 0.0;
    for (int r = 0; r < R; r++) {
      const double x = static_cast<double>(q[r * S + tid]);
      s += x * x;
    }
    nq[tid] = sqrt(s);
  }
  __syncthreads();
  const int per = (S + kPlSlices - 1) / kPlSlices;
  for (int w = tid; w < kPlSlices * S; w += kPlBlock) {
    const int slice = w / S, s = w - slice * S;
    const int j0 = slice * per, j1 = j0 + per < S ? j0 + per : S;
    double sum = 0.0;
    int n = 0;
    for (int j = j0; j < j1; j++) {
      int jj = j + s;
      if (jj >= S) jj -= S;
      const double x = nq[j], y = nc[jj];
      if (x > 0.0 && y > 0.0) {
        double dot = 0.0;
        for (int r = 0; r < R; r++) dot += static_cast<double>(q[r * S + j]) * static_cast<double>(c[r * S + jj]);
        sum += dot / (x * y);
        n++;
      }
    }
    part[slice][s] = sum;
    cnt[slice][s] = n;
  }
  __syncthreads();
  if (tid < S) {
    const double total = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
    const int n = ((cnt[0][tid] + cnt[1][tid]) + cnt[2][tid]) + cnt[3][tid];
    nq[tid] = n > 0 ? 1.0 - (1.0 / static_cast<double>(n)) * total : 1.0;  // d(s), where the query's norms were (all of them have been read)
  }
  __syncthreads();
  if (tid < 64) {
    double best = static_cast<double>(INFINITY);
    unsigned bs = 0xffffffffu;
    for (int s = tid; s < S; s += 64) {
      const double d = nq[s];
      if (pl_before(d, static_cast<unsigned>(s), best, bs)) best = d, bs = static_cast<unsigned>(s);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(best, off);
      const unsigned os = __shfl_xor(bs, off);
      if (pl_before(od, os, best, bs)) best = od, bs = os;
    }
    if (tid == 0) {  // (S >= 1: lane 0 has seen shift 0, so bs is a shift)
      a.d[blockIdx.x] = best;
      a.shift[blockIdx.x] = static_cast<int>(bs);
      if (a.d_host != nullptr) a.d_host[blockIdx.x] = best;
      if (a.shift_host != nullptr) a.shift_host[blockIdx.x] = static_cast<int>(bs);
      if (a.d_host != nullptr || a.shift_host != nullptr) __threadfence_system();
    }
  }
}

// The k best candidates by ascending (d, index), by ONE workgroup: round t takes the least pair behind the one round t - 1 took.  The
// pairs are distinct and a minimum does not depend on the order of its operands.  out: k records {index, shift, distance} (sga_place_match)
// in a slot of the staging ring.  k <= count.
__global__ __launch_bounds__(kPlBlock) void places_select_kernel(const double* __restrict__ d, const int* __restrict__ shift, uint32_t count, unsigned long long first, int k, unsigned long long* __restrict__ out) {
  __shared__ double wd[kPlBlock / 64];
  __shared__ unsigned wi[kPlBlock / 64];
  __shared__ double prev_d;
  __shared__ unsigned prev_i;
  const int tid = threadIdx.x;
  for (int t = 0; t < k; t++) {
    const double pd = t > 0 ? prev_d : 0.0;
    const unsigned pi = t > 0 ? prev_i : 0u;
    double best = static_cast<double>(INFINITY);
    unsigned bi = 0xffffffffu;
    for (uint32_t i = tid; i < count; i += kPlBlock) {
      const double x = d[i];
      if (t > 0 && !pl_before(pd, pi, x, i)) continue;  // taken in an earlier round
      if (pl_before(x, i, best, bi)) best = x, bi = i;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(best, off);
      const unsigned oi = __shfl_xor(bi, off);
      if (pl_before(od, oi, best, bi)) best = od, bi = oi;
    }
    __syncthreads();  // (round t - 1's prev_d / prev_i have been read by everyone)
    if ((tid & 63) == 0) wd[tid >> 6] = best, wi[tid >> 6] = bi;
    __syncthreads();
    if (tid == 0) {
      for (int w = 1; w < kPlBlock / 64; w++)
        if (pl_before(wd[w], wi[w], best, bi)) best = wd[w], bi = wi[w];
      prev_d = best, prev_i = bi;
      // (k <= count and the distances are finite: bi < count)
      out[3 * t + 0] = first + bi;
      out[3 * t + 1] = static_cast<unsigned long long>(static_cast<uint32_t>(bi < count ? shift[bi] : 0));
      out[3 * t + 2] = static_cast<unsigned long long>(__double_as_longlong(best));
    }
    __syncthreads();
  }
  if (tid == 0) __threadfence_system();
}

namespace {

inline bool is_finite(double v) { return v - v == 0.0; }

// what the calls refuse of their parameters (no handle is read)
int place_params_check(const sga_place_params& p) {
  if (p.rings < 1 || p.rings > kPlMaxRings) return fail(SGA_ERR_INVALID, "places: rings %d outside [1, %d]", p.rings, kPlMaxRings);
  if (p.sectors < 1 || p.sectors > kPlMaxSectors) return fail(SGA_ERR_INVALID, "places: sectors %d outside [1, %d]", p.sectors, kPlMaxSectors);
  if (p.rings * p.sectors > kPlMaxCells) return fail(SGA_ERR_INVALID, "places: %d rings x %d sectors are more than %d cells", p.rings, p.sectors, kPlMaxCells);
  if (!is_finite(p.max_range) || !(p.max_range > 0.0)) return fail(SGA_ERR_INVALID, "places: max_range must be finite and > 0");
  if (!is_finite(p.height)) return fail(SGA_ERR_INVALID, "places: height must be finite");
  return SGA_OK;
}
int place_center_check(const double* center) {
  for (int k = 0; center != nullptr && k < 3; k++)
    if (!is_finite(center[k])) return fail(SGA_ERR_INVALID, "places: center has a non-finite entry");
  return SGA_OK;
}
int place_k_check(int k) { return k < 1 || k > kPlMaxK ? fail(SGA_ERR_INVALID, "places: k %d outside [1, %d]", k, kPlMaxK) : SGA_OK; }
// a host image: every value finite and >= 0 (the bits of such values order as the values; a norm of them is a number)
int place_image_check(const sga_place_params& p, const float* image) {
  const size_t cells = static_cast<size_t>(p.rings) * static_cast<size_t>(p.sectors);
  for (size_t i = 0; i < cells; i++) {
    const float v = image[i];
    if (!(v >= 0.f) || !(v <= 3.4028234663852886e38f))
      return fail(SGA_ERR_INVALID, "places: image value %zu (ring %zu, sector %zu) is %g: not finite or negative", i, i / static_cast<size_t>(p.sectors), i % static_cast<size_t>(p.sectors), static_cast<double>(v));
  }
  return SGA_OK;
}

inline void count_wait() { count_launch(Chain::PlacesWait); }

}  // namespace
}  // namespace sga

struct sga_places {
  int device = 0;
  mutable sga::Ready ready;
  sga_place_params params{};
  size_t n = 0, cap = 0;
  size_t stride = 0;  // bytes of an entry: S doubles, R x S floats, rounded up to 8
  sga::DevBuf<unsigned char> entries;
  size_t cells() const { return static_cast<size_t>(params.rings) * static_cast<size_t>(params.sectors); }
  unsigned char* entry(size_t i) const { return entries.p + i * stride; }
  double* norms(size_t i) const { return reinterpret_cast<double*>(entry(i)); }
  float* image(size_t i) const { return reinterpret_cast<float*>(entry(i) + static_cast<size_t>(params.sectors) * sizeof(double)); }
};

namespace sga {
namespace {

PlGrid place_grid(const sga_place_params& p, const sga_cloud* cloud, const double* center) {
  PlGrid g;
  g.R = p.rings, g.S = p.sectors, g.L = p.max_range, g.height = p.height;
  for (int k = 0; k < 3; k++) g.origin[k] = cloud->origin[k], g.center[k] = center ? center[k] : 0.0;
  return g;
}

// The descriptor of `cloud` into `img` (R x S floats of device memory inside the `fill_bytes` at `fill`) on the context's stream: the
// fill, and the kernel when there are records
int place_describe(sga_context* ctx, Chain chain, const sga_place_params& p, const sga_cloud* cloud, const double* center, float* img, void* fill, size_t fill_bytes) {
  count_launch(chain);
  SGA_HIP(hipMemsetAsync(fill, 0, fill_bytes, ctx->stream));
  if (cloud->n == 0) return SGA_OK;
  SGA_TRY(wait_ready(ctx, cloud->ready));  // made on another context that returned before its kernels had run
  const uint32_t n = static_cast<uint32_t>(cloud->n);
  count_launch(chain);
  hipLaunchKernelGGL(places_descriptor_kernel, dim3((n + kPlPointsPerBlock - 1) / kPlPointsPerBlock), dim3(kPlBlock), 0, ctx->stream, cloud->pts.p, n, place_grid(p, cloud, center), reinterpret_cast<uint32_t*>(img));
  SGA_HIP(hipGetLastError());
  return SGA_OK;
}

// room for one more entry: doubling, a device-to-device copy on the context's stream (the old block goes to the stream's free list)
int place_reserve(sga_context* ctx, sga_places* db) {
  if (db->n < db->cap) return SGA_OK;
  const size_t cap = db->cap ? 2 * db->cap : kPlInitialCapacity;
  DevBuf<unsigned char> grown;
  SGA_TRY(grown.alloc(cap * db->stride));
  if (db->n > 0) {
    count_launch(Chain::PlacesAdd);
    SGA_HIP(hipMemcpyAsync(grown.p, db->entries.p, db->n * db->stride, hipMemcpyDeviceToDevice, ctx->stream));
  }
  db->entries.swap(grown);
  db->cap = cap;
  return SGA_OK;
}

// an add's end: a blocking context waits for what it enqueued, a stream-ordered one marks the database
int place_added(sga_context* ctx, sga_places* db, size_t* index) {
  if (!ctx->stream_ordered) {
    count_wait();
    SGA_HIP(hipStreamSynchronize(ctx->stream));
  }
  SGA_TRY(mark_ready(ctx, db->ready));
  *index = db->n++;
  return SGA_OK;
}

// The search and the selection over [first, first + count) for the query image `q` (device memory, or a slot by its device address);
// slot: the matches, then all_dist, then all_shift.  The call's one wait.
int place_search(sga_context* ctx, const sga_places* db, const float* q, sga_context::StageSlot* slot, size_t first, size_t count, int k, sga_place_match* out, size_t* found, double* all_dist, int32_t* all_shift) {
  const int kk = static_cast<size_t>(k) < count ? k : static_cast<int>(count);
  DevBuf<unsigned long long> buf;  // the distances, behind them the shifts; lives to the end of the call (then: the stream's free list)
  SGA_TRY(buf.alloc(count + (count + 1) / 2));
  unsigned long long* slot_dev = static_cast<unsigned long long*>(slot->dev);
  const size_t m_words = 3 * static_cast<size_t>(kPlMaxK), d_words = all_dist ? count : 0;
  PlMatchArgs a;
  std::memset(&a, 0, sizeof(a));
  a.q = q;
  a.entries = db->entry(first), a.stride = db->stride, a.count = static_cast<uint32_t>(count);
  a.R = db->params.rings, a.S = db->params.sectors;
  a.d = reinterpret_cast<double*>(buf.p), a.shift = reinterpret_cast<int*>(buf.p + count);
  a.d_host = all_dist ? reinterpret_cast<double*>(slot_dev + m_words) : nullptr;
  a.shift_host = all_shift ? reinterpret_cast<int*>(slot_dev + m_words + d_words) : nullptr;
  count_launch(Chain::PlacesQuery);
  hipLaunchKernelGGL(places_match_kernel, dim3(a.count), dim3(kPlBlock), 0, ctx->stream, a);
  SGA_HIP(hipGetLastError());
  count_launch(Chain::PlacesQuery);
  hipLaunchKernelGGL(places_select_kernel, dim3(1), dim3(kPlBlock), 0, ctx->stream, a.d, a.shift, a.count, static_cast<unsigned long long>(first), kk, slot_dev);
  SGA_HIP(hipGetLastError());
  count_wait();
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait: the matches are in the slot
  const unsigned long long* host = static_cast<const unsigned long long*>(slot->host);
  for (int t = 0; t < kk; t++) {
    out[t].index = static_cast<int64_t>(host[3 * t]);
    out[t].shift = static_cast<int32_t>(host[3 * t + 1]);
    out[t].reserved = 0;
    std::memcpy(&out[t].distance, &host[3 * t + 2], sizeof(double));
  }
  if (all_dist) std::memcpy(all_dist, host + m_words, count * sizeof(double));
  if (all_shift) std::memcpy(all_shift, host + m_words + d_words, count * sizeof(int32_t));
  *found = static_cast<size_t>(kk);
  return SGA_OK;
}

// 8-byte words of a query's slot: the matches, all_dist, all_shift (rounded up to 8); a query image travels behind them
inline size_t place_slot_words(size_t count, bool all_dist, bool all_shift) { return 3 * static_cast<size_t>(kPlMaxK) + (all_dist ? count : 0) + (all_shift ? (count + 1) / 2 : 0); }

int place_range_check(const sga_places* db, size_t first, size_t count) {
  if (first > db->n || count > db->n - first) return fail(SGA_ERR_INVALID, "places: entries [%zu, %zu + %zu) reach beyond the database's %zu", first, first, count, db->n);
  return SGA_OK;
}

}  // namespace
}  // namespace sga

using namespace sga;

extern "C" {

void sga_place_params_default(sga_place_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->rings = 20, p->sectors = 60;
  p->max_range = 80.0, p->height = 2.0;
}

int sga_places_create(sga_context* ctx, const sga_place_params* params, sga_places** out) {
  if (!ctx || !params || !out) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(place_params_check(*params));
  auto db = std::make_unique<sga_places>();
  db->device = ctx->device;
  db->params = *params;
  db->stride = (static_cast<size_t>(params->sectors) * sizeof(double) + db->cells() * sizeof(float) + 7) / 8 * 8;
  *out = db.release();
  return SGA_OK;
}

int sga_places_destroy(sga_places* db) {
  delete db;
  return SGA_OK;
}

int sga_places_size(const sga_places* db, size_t* n) {
  if (!db || !n) return fail(SGA_ERR_INVALID, "null argument");
  *n = db->n;
  return SGA_OK;
}

int sga_places_params(const sga_places* db, sga_place_params* params) {
  if (!db || !params) return fail(SGA_ERR_INVALID, "null argument");
  *params = db->params;
  return SGA_OK;
}

int sga_places_add(sga_context* ctx, sga_places* db, const sga_cloud* cloud, const double center[3], size_t* index) {
  if (!ctx || !db || !cloud || !index) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(place_center_check(center));
  // ---- (from here on the handles are read)
  if (db->device != ctx->device) return fail(SGA_ERR_INVALID, "the database lives on another device");
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (cloud->n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", cloud->n);
  if (db->n >= (1ull << 31) - 1) return fail(SGA_ERR_INVALID, "places: the database is full (2^31-1 entries)");
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, db->ready));
  SGA_TRY(place_reserve(ctx, db));
  // the fill zeroes the norms as well: an empty cloud's entry is complete with it
  SGA_TRY(place_describe(ctx, Chain::PlacesAdd, db->params, cloud, center, db->image(db->n), db->entry(db->n), db->stride));
  if (cloud->n > 0) {
    count_launch(Chain::PlacesAdd);
    hipLaunchKernelGGL(places_norms_kernel, dim3(1), dim3(kPlBlock), 0, ctx->stream, db->image(db->n), db->image(db->n), db->norms(db->n), db->params.rings, db->params.sectors);
    SGA_HIP(hipGetLastError());
  }
  return place_added(ctx, db, index);
}

int sga_places_add_descriptor(sga_context* ctx, sga_places* db, const float* image, size_t* index) {
  if (!ctx || !db || !image || !index) return fail(SGA_ERR_INVALID, "null argument");
  // ---- (from here on the handles are read)
  if (db->device != ctx->device) return fail(SGA_ERR_INVALID, "the database lives on another device");
  if (db->n >= (1ull << 31) - 1) return fail(SGA_ERR_INVALID, "places: the database is full (2^31-1 entries)");
  SGA_TRY(place_image_check(db->params, image));
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, db->ready));
  SGA_TRY(place_reserve(ctx, db));
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, db->cells() * sizeof(float), &slot));
  std::memcpy(slot->host, image, db->cells() * sizeof(float));
  count_launch(Chain::PlacesAdd);
  hipLaunchKernelGGL(places_norms_kernel, dim3(1), dim3(kPlBlock), 0, ctx->stream, static_cast<const float*>(slot->dev), db->image(db->n), db->norms(db->n), db->params.rings, db->params.sectors);
  SGA_HIP(hipGetLastError());
  SGA_TRY(stage_release(ctx, slot));  // behind its reader
  return place_added(ctx, db, index);
}

int sga_places_download(sga_context* ctx, const sga_places* db, size_t first, size_t count, float* images) {
  if (!ctx || !db || (!images && count > 0)) return fail(SGA_ERR_INVALID, "null argument");
  // ---- (from here on the handles are read)
  if (db->device != ctx->device) return fail(SGA_ERR_INVALID, "the database lives on another device");
  SGA_TRY(place_range_check(db, first, count));
  if (count == 0) return SGA_OK;
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, db->ready));
  const size_t row = db->cells() * sizeof(float);
  SGA_HIP(hipMemcpy2DAsync(images, row, db->image(first), db->stride, row, count, hipMemcpyDeviceToHost, ctx->stream));
  count_wait();
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

int sga_cloud_scan_context(sga_context* ctx, const sga_cloud* cloud, const sga_place_params* params, const double center[3], float* image) {
  if (!ctx || !cloud || !params || !image) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(place_params_check(*params));
  SGA_TRY(place_center_check(center));
  // ---- (from here on the handles are read)
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (cloud->n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", cloud->n);
  SGA_ENTER(ctx);
  const size_t bytes = static_cast<size_t>(params->rings) * static_cast<size_t>(params->sectors) * sizeof(float);
  DevBuf<float> img;  // lives to the end of the call (then: the stream's free list)
  SGA_TRY(img.alloc(bytes / sizeof(float)));
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, bytes, &slot));
  SGA_TRY(place_describe(ctx, Chain::PlacesAdd, *params, cloud, center, img.p, img.p, bytes));
  count_launch(Chain::PlacesAdd);
  SGA_HIP(hipMemcpyAsync(slot->host, img.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
  count_wait();
  SGA_HIP(hipStreamSynchronize(ctx->stream));  // the call's one wait
  std::memcpy(image, slot->host, bytes);
  return SGA_OK;
}

int sga_places_query(sga_context* ctx, const sga_places* db, const sga_cloud* cloud, const double center[3], size_t first, size_t count, int k, sga_place_match* out, size_t* found, double* all_dist, int32_t* all_shift) {
  if (!ctx || !db || !cloud || !out || !found) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(place_center_check(center));
  SGA_TRY(place_k_check(k));
  // ---- (from here on the handles are read)
  if (db->device != ctx->device) return fail(SGA_ERR_INVALID, "the database lives on another device");
  if (cloud->device != ctx->device) return fail(SGA_ERR_INVALID, "cloud lives on another device");
  if (cloud->n >= (1ull << 31)) return fail(SGA_ERR_INVALID, "too many points (%zu; limit 2^31-1)", cloud->n);
  SGA_TRY(place_range_check(db, first, count));
  if (count == 0) {  // nothing is launched
    *found = 0;
    return SGA_OK;
  }
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, db->ready));
  DevBuf<float> q;  // lives to the end of the call (then: the stream's free list)
  SGA_TRY(q.alloc(db->cells()));
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, place_slot_words(count, all_dist != nullptr, all_shift != nullptr) * 8, &slot));
  SGA_TRY(place_describe(ctx, Chain::PlacesQuery, db->params, cloud, center, q.p, q.p, db->cells() * sizeof(float)));
  return place_search(ctx, db, q.p, slot, first, count, k, out, found, all_dist, all_shift);
}

int sga_places_query_descriptor(sga_context* ctx, const sga_places* db, const float* image, size_t first, size_t count, int k, sga_place_match* out, size_t* found, double* all_dist, int32_t* all_shift) {
  if (!ctx || !db || !image || !out || !found) return fail(SGA_ERR_INVALID, "null argument");
  SGA_TRY(place_k_check(k));
  // ---- (from here on the handles are read)
  if (db->device != ctx->device) return fail(SGA_ERR_INVALID, "the database lives on another device");
  SGA_TRY(place_range_check(db, first, count));
  SGA_TRY(place_image_check(db->params, image));
  if (count == 0) {  // nothing is launched
    *found = 0;
    return SGA_OK;
  }
  SGA_ENTER(ctx);
  SGA_TRY(wait_ready(ctx, db->ready));
  // the query image travels behind the results in the call's slot; the match kernel reads it there by its device address
  const size_t words = place_slot_words(count, all_dist != nullptr, all_shift != nullptr);
  sga_context::StageSlot* slot = nullptr;
  SGA_TRY(stage_acquire(ctx, words * 8 + db->cells() * sizeof(float), &slot));
  std::memcpy(static_cast<unsigned long long*>(slot->host) + words, image, db->cells() * sizeof(float));
  return place_search(ctx, db, reinterpret_cast<const float*>(static_cast<unsigned long long*>(slot->dev) + words), slot, first, count, k, out, found, all_dist, all_shift);
}

int sga_debug_places_add_launches(unsigned long long* launches) { return report_launches(Chain::PlacesAdd, launches); }
int sga_debug_places_query_launches(unsigned long long* launches) { return report_launches(Chain::PlacesQuery, launches); }
int sga_debug_places_waits(unsigned long long* waits) { return report_launches(Chain::PlacesWait, waits); }

}  // extern "C"

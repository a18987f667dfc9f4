// Context (one GPU + one stream): its lifecycle, error plumbing, profiling getters and the host side of notes (notes.hpp).
#include "common.hpp"
#include "notes.hpp"

#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>

// HIP streams share a small pool of hardware queues (4 per device by default), and two streams that land on one queue run their
// kernels one after the other.  The library's unit of concurrency is a context = a stream (pipelined preprocessing, several registrations
// side by side, one context per policy thread): measured in round 6, two side-by-side C3 registrations gave 10 800 iterations/s on
// distinct queues and 8 600 (nothing) when the runtime had put their streams on one — which depended on how many streams the process had
// created before.  Unless the user has set it, ask for 8 queues before the HIP runtime initialises (it reads the variable once).
namespace {
struct HwQueuesDefault {
  HwQueuesDefault() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }
} g_hw_queues_default;
}  // namespace

namespace sga {
void preload_hot_kernels();  // linearize.hip

// The first kernel of a queue that needs scratch memory (a few spilled registers are enough: certify_linearize_kernel has 20 bytes per
// lane) makes the runtime allocate the queue's scratch arena: ~0.2 ms, paid in the middle of somebody's first registration.  A context
// pays it when it is created instead: one tiny launch with 256 bytes of private memory per lane on its stream.
__global__ void scratch_prime_kernel(int* out, int n) {
  volatile int buf[64];
  for (int i = 0; i < 64; i++) buf[i] = i * n;
  int t = 0;
  for (int i = 0; i < 64; i++) t += buf[(i * 7 + n) & 63];
  if (n < 0) *out = t;  // never taken: the array must not be optimised away
}

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int ensure_temp(sga_context* ctx, size_t bytes) { return ctx->d_temp.reserve(bytes); }

}  // namespace sga

void sga_profile_collect_pending(sga_context* ctx);

using namespace sga;

extern "C" {

const char* sga_last_error(void) { return g_err; }

const char* sga_version(void) { return "small_gicp_amd 0.1.0 (gfx950)"; }

int sga_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

constexpr int kNotesAt = 160;  // h_accum: doubles [0, 129) results + sequence word, [136, 144) scratch ints, [160, 192) notes
constexpr int kPinnedDoubles = kNotesAt + sga::kNoteSlots * sga::kNoteWords;
static int context_create_impl(int device, void* stream, bool borrow, sga_context** out) {
  if (!out) return fail(SGA_ERR_INVALID, "null out");
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) return fail(SGA_ERR_NO_DEVICE, "no HIP device available (%s): small_gicp_amd has no CPU fallback", e == hipSuccess ? "count=0" : hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(SGA_ERR_INVALID, "device %d out of range [0,%d)", device, n);
  SGA_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  SGA_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return fail(SGA_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
  auto* ctx = new sga_context;
  ctx->device = device;
  ctx->num_cus = prop.multiProcessorCount;
  if (borrow) {
    ctx->stream = static_cast<hipStream_t>(stream);
    ctx->owns_stream = false;
  } else {
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
      delete ctx;
      return fail(SGA_ERR_HIP, "hipStreamCreate failed");
    }
    ctx->owns_stream = true;
  }
  dev_cache_context_created(device, ctx->stream);
  ctx->registered = true;
  StreamScope scope(ctx->stream);
  int rc = ctx->d_accum.alloc(128);
  if (rc == SGA_OK) rc = ctx->d_ticket.alloc(16);
  if (rc == SGA_OK && hipMemsetAsync(ctx->d_ticket.p, 0, 16 * sizeof(unsigned), ctx->stream) != hipSuccess) rc = fail(SGA_ERR_HIP, "hipMemsetAsync failed");
  if (rc == SGA_OK && hipHostMalloc(reinterpret_cast<void**>(&ctx->h_accum), kPinnedDoubles * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) rc = fail(SGA_ERR_HIP, "hipHostMalloc failed");
  if (rc == SGA_OK) {
    std::memset(ctx->h_accum, 0, kPinnedDoubles * sizeof(double));
    ctx->h_scratch = reinterpret_cast<int*>(ctx->h_accum + 136);  // doubles [136, 144) of the pinned block
    if (hipHostGetDevicePointer(reinterpret_cast<void**>(&ctx->h_accum_dev), ctx->h_accum, 0) != hipSuccess) rc = fail(SGA_ERR_HIP, "hipHostGetDevicePointer failed");
    ctx->h_notes = reinterpret_cast<unsigned long long*>(ctx->h_accum + kNotesAt);  // words [160, 192): the notes (notes.hpp)
    ctx->h_notes_dev = reinterpret_cast<unsigned long long*>(ctx->h_accum_dev + kNotesAt);
  }
  if (rc == SGA_OK) rc = ctx->d_spacing.alloc(4);
  if (rc == SGA_OK && hipMemsetAsync(ctx->d_spacing.p, 0, 4 * sizeof(unsigned long long), ctx->stream) != hipSuccess) rc = fail(SGA_ERR_HIP, "hipMemsetAsync failed");
  if (rc == SGA_OK) rc = ctx->d_box.alloc(8);
  if (rc == SGA_OK) {
    const int init[8] = {kBoxEncPosInf, kBoxEncPosInf, kBoxEncPosInf, kBoxEncNegInf, kBoxEncNegInf, kBoxEncNegInf, 0, 0};
    if (hipMemcpyAsync(ctx->d_box.p, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) rc = fail(SGA_ERR_HIP, "box accumulator init failed");
  }
  if (rc == SGA_OK && (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess || hipEventCreate(&ctx->ev2) != hipSuccess || hipEventCreate(&ctx->ev3) != hipSuccess || hipEventCreate(&ctx->ev_mid) != hipSuccess || hipEventCreate(&ctx->ev_comm) != hipSuccess || hipEventCreateWithFlags(&ctx->ev_aux, hipEventDisableTiming) != hipSuccess)) rc = fail(SGA_ERR_HIP, "hipEventCreate failed");
  if (rc != SGA_OK) {
    sga_context_destroy(ctx);
    return rc;
  }
  hipLaunchKernelGGL(scratch_prime_kernel, dim3(1), dim3(64), 0, ctx->stream, static_cast<int*>(nullptr), 1);
  (void)hipGetLastError();
  {  // once per process: resolve the hot kernels now instead of in the middle of the first registration (linearize.hip)
    static std::once_flag preload_once;
    std::call_once(preload_once, [] { preload_hot_kernels(); });
  }
  *out = ctx;
  return SGA_OK;
}

int sga_context_create(int device, sga_context** out) { return context_create_impl(device, nullptr, false, out); }
int sga_context_create_on_stream(int device, void* hip_stream, sga_context** out) { return context_create_impl(device, hip_stream, true, out); }

int sga_context_destroy(sga_context* ctx) {
  if (!ctx) return SGA_OK;
  (void)hipSetDevice(ctx->device);
  (void)sga_comm_destroy(ctx);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
  if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
  if (ctx->ev2) (void)hipEventDestroy(ctx->ev2);
  if (ctx->ev3) (void)hipEventDestroy(ctx->ev3);
  if (ctx->ev_mid) (void)hipEventDestroy(ctx->ev_mid);
  if (ctx->ev_comm) (void)hipEventDestroy(ctx->ev_comm);
  if (ctx->ev_aux) (void)hipEventDestroy(ctx->ev_aux);
  if (ctx->ev_io_in) (void)hipEventDestroy(ctx->ev_io_in);
  if (ctx->ev_io_out) (void)hipEventDestroy(ctx->ev_io_out);
  if (ctx->ev_t0) (void)hipEventDestroy(ctx->ev_t0);
  if (ctx->ev_t1) (void)hipEventDestroy(ctx->ev_t1);
  if (ctx->h_accum) (void)hipHostFree(ctx->h_accum);
  if (ctx->h_forest) (void)hipHostFree(ctx->h_forest);
  for (auto& slot : ctx->stage) {
    if (slot.host) (void)hipHostFree(slot.host);
    if (slot.done) (void)hipEventDestroy(slot.done);
  }
  const int device = ctx->device;
  const hipStream_t stream = ctx->stream;
  const bool registered = ctx->registered, owns = ctx->owns_stream;
  {
    StreamScope scope(stream);  // the context's own buffers: the stream is idle (synchronised above)
    delete ctx;
  }
  if (registered) dev_cache_context_destroyed(device, stream);  // the last context gives the cached device memory back
  if (owns && stream) (void)hipStreamDestroy(stream);
  return SGA_OK;
}

int sga_context_synchronize(sga_context* ctx) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  SGA_HIP(hipStreamSynchronize(ctx->stream));
  return SGA_OK;
}

void* sga_context_stream(sga_context* ctx) { return ctx ? static_cast<void*>(ctx->stream) : nullptr; }

}  // extern "C"
namespace sga {
int mark_ready(sga_context* ctx, Ready& r) {
  if (!ctx->stream_ordered) {  // the entry point synchronised its stream before returning: nothing in flight
    r.pending = false;
    return SGA_OK;
  }
  if (!r.event) SGA_HIP(hipEventCreateWithFlags(&r.event, hipEventDisableTiming));
  SGA_HIP(hipEventRecord(r.event, ctx->stream));
  r.stream = ctx->stream;
  r.pending = true;
  return SGA_OK;
}
int wait_ready(sga_context* ctx, const Ready& r) {
  if (r.pending && r.event && r.stream != ctx->stream) SGA_HIP(hipStreamWaitEvent(ctx->stream, r.event, 0));
  return SGA_OK;
}
}  // namespace sga
extern "C" {

int sga_context_set_stream_ordered(sga_context* ctx, int enabled) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  if (!enabled && ctx->stream_ordered) (void)hipStreamSynchronize(ctx->stream);
  ctx->stream_ordered = enabled != 0;
  return SGA_OK;
}

int sga_context_set_profiling(sga_context* ctx, int enabled) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  ctx->profiling = enabled != 0;
  ctx->profile_period = enabled > 1 ? static_cast<unsigned>(enabled) : 1u;
  ctx->lin_seq = ctx->err_seq = 0;
  ctx->lin_ms = ctx->err_ms = 0.0;
  ctx->lin_calls = ctx->err_calls = 0;
  ctx->search_ms = 0.0;
  ctx->search_calls = 0;
  ctx->warm_ms = ctx->cold_ms = ctx->warm_first_ms = 0.0;
  ctx->warm_calls = ctx->cold_calls = 0;
  ctx->comm_ms = 0.0;
  ctx->comm_calls = 0;
  ctx->comm_recorded = false;
  ctx->pending = 0;
  return SGA_OK;
}

// GPU time between two points of the context's stream (bench.py: the per-stage roofline lines of the preprocessing kernels)
int sga_debug_timer_start(sga_context* ctx) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  SGA_HIP(hipSetDevice(ctx->device));
  if (!ctx->ev_t0) SGA_HIP(hipEventCreate(&ctx->ev_t0));
  if (!ctx->ev_t1) SGA_HIP(hipEventCreate(&ctx->ev_t1));
  SGA_HIP(hipEventRecord(ctx->ev_t0, ctx->stream));
  return SGA_OK;
}
int sga_debug_timer_stop(sga_context* ctx, double* ms) {
  if (!ctx || !ms || !ctx->ev_t0) return fail(SGA_ERR_INVALID, "no timer running");
  SGA_HIP(hipEventRecord(ctx->ev_t1, ctx->stream));
  SGA_HIP(hipEventSynchronize(ctx->ev_t1));
  float f = 0.f;
  SGA_HIP(hipEventElapsedTime(&f, ctx->ev_t0, ctx->ev_t1));
  *ms = f;
  return SGA_OK;
}

int sga_context_get_kernel_ms(sga_context* ctx, double* lin_ms, uint64_t* lin_calls, double* err_ms, uint64_t* err_calls) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  sga_profile_collect_pending(ctx);
  if (lin_ms) *lin_ms = ctx->lin_calls ? ctx->lin_ms / ctx->lin_calls : 0.0;
  if (lin_calls) *lin_calls = ctx->lin_calls;
  if (err_ms) *err_ms = ctx->err_calls ? ctx->err_ms / ctx->err_calls : 0.0;
  if (err_calls) *err_calls = ctx->err_calls;
  return SGA_OK;
}

int sga_context_get_pass_ms(sga_context* ctx, double* cold_ms, uint64_t* cold_calls, double* warm_ms, uint64_t* warm_calls, double* warm_search_ms) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  sga_profile_collect_pending(ctx);
  if (cold_ms) *cold_ms = ctx->cold_calls ? ctx->cold_ms / ctx->cold_calls : 0.0;
  if (cold_calls) *cold_calls = ctx->cold_calls;
  if (warm_ms) *warm_ms = ctx->warm_calls ? ctx->warm_ms / ctx->warm_calls : 0.0;
  if (warm_calls) *warm_calls = ctx->warm_calls;
  if (warm_search_ms) *warm_search_ms = ctx->warm_calls ? ctx->warm_first_ms / ctx->warm_calls : 0.0;
  return SGA_OK;
}

int sga_context_get_comm_ms(sga_context* ctx, double* comm_ms, uint64_t* comm_calls) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  sga_profile_collect_pending(ctx);
  if (comm_ms) *comm_ms = ctx->comm_calls ? ctx->comm_ms / ctx->comm_calls : 0.0;
  if (comm_calls) *comm_calls = ctx->comm_calls;
  return SGA_OK;
}

int sga_context_get_search_ms(sga_context* ctx, double* search_ms, uint64_t* search_calls) {
  if (!ctx) return fail(SGA_ERR_INVALID, "null context");
  sga_profile_collect_pending(ctx);
  if (search_ms) *search_ms = ctx->search_calls ? ctx->search_ms / ctx->search_calls : 0.0;
  if (search_calls) *search_calls = ctx->search_calls;
  return SGA_OK;
}

// ---- notes (notes.hpp) -------------------------------------------------------------------------------------------------------
}  // extern "C"
namespace sga {
unsigned long long note_begin(sga_context* ctx, unsigned long long** dev_slot) {
  const unsigned long long seq = ++ctx->note_seq;
  *dev_slot = ctx->h_notes_dev + (seq % kNoteSlots) * kNoteWords;
  return seq;
}
int wait_published(sga_context* ctx, const unsigned long long* word, unsigned long long seq) {
  const auto t0 = std::chrono::steady_clock::now();
  for (unsigned spins = 0;; spins++) {
    if (__atomic_load_n(word, __ATOMIC_ACQUIRE) == seq) return SGA_OK;
#if defined(__x86_64__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
    if (spins > 200000u) std::this_thread::yield();  // a word normally arrives within tens of microseconds; past ~1 ms stop hogging the core
    if ((spins & 0xfffu) == 0xfffu) {
      // the stream has drained without publishing (a fault), or this is taking implausibly long: let the runtime report it
      const hipError_t q = hipStreamQuery(ctx->stream);
      (void)hipGetLastError();  // hipErrorNotReady is sticky in hipGetLastError
      if (q != hipErrorNotReady || std::chrono::steady_clock::now() - t0 > std::chrono::seconds(20)) {
        SGA_HIP(hipStreamSynchronize(ctx->stream));
        return __atomic_load_n(word, __ATOMIC_ACQUIRE) == seq ? SGA_OK : kNotPublished;
      }
    }
  }
}
int note_wait(sga_context* ctx, unsigned long long seq, unsigned long long payload[kNoteWords - 1]) {
  const unsigned long long* slot = ctx->h_notes + (seq % kNoteSlots) * kNoteWords;
  const int rc = wait_published(ctx, slot, seq);
  if (rc == kNotPublished) return fail(SGA_ERR_HIP, "a note was not published by the device");
  SGA_TRY(rc);
  for (int k = 0; k < kNoteWords - 1; k++) payload[k] = slot[1 + k];
  return SGA_OK;
}
}  // namespace sga

namespace sga {
namespace {
struct LateRing {
  std::mutex mu;
  unsigned long long* host = nullptr;
  bool failed = false;
  std::atomic<unsigned long long> seq{0};
};
LateRing& late_ring() {
  static LateRing* r = new LateRing;  // never destroyed: no HIP calls during static destruction
  return *r;
}
}  // namespace
unsigned long long late_note_begin(int device, unsigned long long** dev_slot) {
  LateRing& r = late_ring();
  *dev_slot = nullptr;
  {
    std::lock_guard<std::mutex> lock(r.mu);
    if (r.host == nullptr && !r.failed) {
      void* p = nullptr;
      if (hipHostMalloc(&p, sizeof(unsigned long long) * kLateSlots * kLateWords, hipHostMallocMapped | hipHostMallocPortable | hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        r.failed = true;
      } else {
        std::memset(p, 0, sizeof(unsigned long long) * kLateSlots * kLateWords);
        r.host = static_cast<unsigned long long*>(p);
      }
    }
    if (r.host == nullptr) return 0;
  }
  void* dev = nullptr;
  (void)device;
  if (hipHostGetDevicePointer(&dev, r.host, 0) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  const unsigned long long seq = ++r.seq;
  *dev_slot = static_cast<unsigned long long*>(dev) + (seq % kLateSlots) * kLateWords;
  return seq;
}
int late_note_peek(unsigned long long seq, unsigned long long payload[kLateWords - 1]) {
  LateRing& r = late_ring();
  if (seq == 0 || r.host == nullptr) return -1;
  const unsigned long long* slot = r.host + (seq % kLateSlots) * kLateWords;
  const unsigned long long have = __atomic_load_n(slot + kLateWords - 1, __ATOMIC_ACQUIRE);
  if (have == seq) {
    for (int k = 0; k < kLateWords - 1; k++) payload[k] = slot[k];
    if (__atomic_load_n(slot + kLateWords - 1, __ATOMIC_ACQUIRE) != seq) return -1;  // overwritten while it was being read
    return 1;
  }
  return have < seq ? 0 : -1;
}
}  // namespace sga

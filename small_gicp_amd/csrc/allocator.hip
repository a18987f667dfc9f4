// The caching device allocator, stream ordered (common.hpp: device memory).
#include "common.hpp"

#include <atomic>
#include <map>
#include <mutex>
#include <unordered_map>

namespace sga {

// ---- caching device allocator, stream ordered (see common.hpp) -------------------------------------------------------------------
namespace {
thread_local hipStream_t g_cur_stream = nullptr;  // set by SGA_ENTER for the duration of an entry point
// Every entry-point invocation has a process-wide unique number.  A block that is freed by the invocation that allocated it (a temporary:
// sort keys, scan flags, staging arrays) was never visible to anybody else — no other stream can hold work that touches it — so it goes
// straight back to its stream's list.  (Round 6: the general path asks every other stream of the device whether it is busy and records an
// event on each that is: ~25 us per free with four streams in flight, under the allocator's lock — the pipelined odometry driver spent
// more time there than its kernels took.)
thread_local unsigned long long g_cur_epoch = 0;
std::atomic<unsigned long long> g_epoch_counter{0};

struct FreeKey {
  int device;
  hipStream_t stream;  // nullptr = the shared pool: blocks nobody is using any more
  size_t bucket;
  bool operator<(const FreeKey& o) const {
    if (device != o.device) return device < o.device;
    if (stream != o.stream) return stream < o.stream;
    return bucket < o.bucket;
  }
};
struct PendingBlock {
  void* p;
  int device;
  size_t bucket;
};
// Blocks freed where another stream may still use them wait for events — recorded LAZILY and shared: a free only parks the block
// (`unbatched`); the next allocation that misses the free lists records ONE event on every busy stream of the device for all the blocks
// parked since (an event recorded after the free covers everything that was in flight at the free, and more: conservative), and a
// batch's blocks join the shared pool when its events have completed.  (Round 6: an event per block and stream, recorded at the free,
// cost ~25 us per free with four streams in flight.)
struct PendingBatch {
  int device;
  std::vector<hipEvent_t> events;
  std::vector<PendingBlock> blocks;
};
struct DevCache {
  std::mutex mu;
  struct Live {
    int device;
    size_t bucket;
    unsigned long long epoch;  // the entry-point invocation that allocated it (0: outside any)
    hipStream_t stream;        // ... and its stream
  };
  std::unordered_map<void*, Live> live;  // every block handed out
  std::map<FreeKey, std::vector<void*>> free_blocks;
  std::vector<PendingBlock> unbatched;                     // freed where other streams may be using them; no event recorded yet
  std::vector<PendingBatch> pending;                       // ... with their events: reusable once those have completed
  std::vector<std::pair<int, hipStream_t>> streams;        // the streams of the live contexts
  std::vector<hipEvent_t> event_pool;
  size_t cached_bytes = 0;
  int contexts = 0;
  uint64_t n_malloc = 0, n_stream_hit = 0, n_pool_hit = 0, n_pending_hit = 0, n_deferred = 0;  // statistics (sga_allocator_stats)
};
DevCache& dev_cache() {
  static DevCache* c = new DevCache;  // never destroyed: no HIP calls during static destruction
  return *c;
}
constexpr size_t kCacheLimitBytes = 8ull << 30;

// < 1 MiB: next power of two (>= 256 B); above: 8 buckets per octave (<= 12.5 % slack)
size_t bucket_bytes(size_t bytes) {
  size_t p2 = 256;
  while (p2 < bytes) p2 <<= 1;
  if (p2 <= (1ull << 20)) return p2;
  const size_t step = p2 >> 4;  // p2/2 < bytes <= p2: steps of (p2/2)/8
  return ((bytes + step - 1) / step) * step;
}

void recycle_events(DevCache& c, std::vector<hipEvent_t>& evs) {
  for (hipEvent_t e : evs) c.event_pool.push_back(e);
  evs.clear();
}

// batches whose events have all completed -> the shared pool; the blocks parked since the last call get their batch (one event per busy
// stream of their device; no busy stream: straight to the pool)
void collect_pending_locked(DevCache& c) {
  size_t w = 0;
  for (size_t i = 0; i < c.pending.size(); i++) {
    PendingBatch& b = c.pending[i];
    bool done = true;
    for (hipEvent_t e : b.events)
      if (hipEventQuery(e) == hipErrorNotReady) {
        done = false;
        break;
      }
    if (done) {
      recycle_events(c, b.events);
      for (const PendingBlock& k : b.blocks) c.free_blocks[{k.device, nullptr, k.bucket}].push_back(k.p);
    } else {
      if (w != i) c.pending[w] = std::move(b);
      w++;
    }
  }
  c.pending.resize(w);
  if (!c.unbatched.empty()) {
    int cur = -1;
    (void)hipGetDevice(&cur);
    const int restore = cur;
    std::vector<PendingBatch> fresh;
    for (PendingBlock& k : c.unbatched) {
      PendingBatch* batch = nullptr;
      for (PendingBatch& f : fresh)
        if (f.device == k.device) batch = &f;
      if (batch == nullptr) {
        fresh.push_back(PendingBatch{k.device, {}, {}});
        batch = &fresh.back();
        for (const auto& ds : c.streams) {
          if (ds.first != k.device) continue;
          if (hipStreamQuery(ds.second) != hipErrorNotReady) continue;  // idle: nothing of it can touch the blocks
          if (cur != k.device) {
            (void)hipSetDevice(k.device);
            cur = k.device;
          }
          hipEvent_t e = nullptr;
          if (!c.event_pool.empty()) {
            e = c.event_pool.back();
            c.event_pool.pop_back();
          } else if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            e = nullptr;
          }
          if (e == nullptr || hipEventRecord(e, ds.second) != hipSuccess) {
            (void)hipStreamSynchronize(ds.second);  // cannot track it: wait for it instead
            if (e) c.event_pool.push_back(e);
            continue;
          }
          batch->events.push_back(e);
        }
      }
      batch->blocks.push_back(k);
    }
    c.unbatched.clear();
    if (cur != restore && restore >= 0) (void)hipSetDevice(restore);
    for (PendingBatch& f : fresh) {
      if (f.events.empty()) {
        for (const PendingBlock& k : f.blocks) c.free_blocks[{k.device, nullptr, k.bucket}].push_back(k.p);
      } else {
        c.n_deferred += f.blocks.size();
        c.pending.push_back(std::move(f));
      }
    }
  }
  (void)hipGetLastError();  // hipEventQuery's / hipStreamQuery's hipErrorNotReady is sticky in hipGetLastError
}

void release_cached_locked(DevCache& c) {
  for (PendingBatch& b : c.pending) {
    for (hipEvent_t e : b.events) (void)hipEventSynchronize(e);
    recycle_events(c, b.events);
    for (const PendingBlock& k : b.blocks) (void)hipFree(k.p);
  }
  c.pending.clear();
  for (const PendingBlock& k : c.unbatched) (void)hipFree(k.p);  // (hipFree synchronises the device: safe whatever is in flight)
  c.unbatched.clear();
  for (auto& kv : c.free_blocks)
    for (void* q : kv.second) (void)hipFree(q);
  c.free_blocks.clear();
  c.cached_bytes = 0;
}

void* take_locked(DevCache& c, const FreeKey& key) {
  auto it = c.free_blocks.find(key);
  if (it == c.free_blocks.end() || it->second.empty()) return nullptr;
  void* p = it->second.back();
  it->second.pop_back();
  return p;
}
}  // namespace

StreamScope::StreamScope(hipStream_t s) : prev(g_cur_stream), prev_epoch(g_cur_epoch) {
  g_cur_stream = s;
  g_cur_epoch = s != nullptr ? ++g_epoch_counter : 0ull;
}
StreamScope::~StreamScope() {
  g_cur_stream = prev;
  g_cur_epoch = prev_epoch;
}

int dev_alloc(void** p, size_t bytes) {
  *p = nullptr;
  if (bytes == 0) return SGA_OK;
  int device = 0;
  if (hipGetDevice(&device) != hipSuccess) return fail(SGA_ERR_HIP, "hipGetDevice failed");
  const size_t bucket = bucket_bytes(bytes);
  DevCache& c = dev_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  // same stream first (stream order makes the reuse safe), then blocks nobody uses, then blocks whose last users have finished
  if (g_cur_stream != nullptr && (*p = take_locked(c, {device, g_cur_stream, bucket})) != nullptr) c.n_stream_hit++;
  if (!*p && (*p = take_locked(c, {device, nullptr, bucket})) != nullptr) c.n_pool_hit++;
  if (!*p && (!c.pending.empty() || !c.unbatched.empty())) {
    collect_pending_locked(c);
    if ((*p = take_locked(c, {device, nullptr, bucket})) != nullptr) c.n_pending_hit++;
  }
  if (*p) {
    c.cached_bytes -= bucket;
  } else {
    c.n_malloc++;
    hipError_t e = hipMalloc(p, bucket);
    if (e != hipSuccess) {  // out of memory with blocks parked in the cache: give them back and retry once
      (void)hipGetLastError();
      release_cached_locked(c);
      e = hipMalloc(p, bucket);
    }
    if (e != hipSuccess) {
      *p = nullptr;
      return fail(SGA_ERR_HIP, "hipMalloc(%zu bytes) -> %s", bucket, hipGetErrorString(e));
    }
  }
  c.live[*p] = DevCache::Live{device, bucket, g_cur_epoch, g_cur_stream};
  return SGA_OK;
}

void dev_free(void* p) {
  if (!p) return;
  DevCache& c = dev_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  auto it = c.live.find(p);
  if (it == c.live.end()) {
    (void)hipFree(p);
    return;
  }
  const int device = it->second.device;
  const size_t bucket = it->second.bucket;
  const bool temporary = g_cur_stream != nullptr && it->second.epoch == g_cur_epoch && it->second.epoch != 0ull && it->second.stream == g_cur_stream;
  c.live.erase(it);
  if (c.contexts == 0 || c.cached_bytes + bucket > kCacheLimitBytes) {
    (void)hipFree(p);  // synchronises the device: safe whatever is in flight
    return;
  }
  c.cached_bytes += bucket;
  if (temporary) {  // allocated by this very invocation: nobody else has seen it
    c.free_blocks[{device, g_cur_stream, bucket}].push_back(p);
    return;
  }
  // Anything else — a buffer of a long-lived object (an index's attributes, a problem's mahalanobis cache, the rejector flags: kernels
  // another context has enqueued on its own stream may be reading it) or a block freed outside any entry point (destroy
  // functions) — may still be in use on any stream of the device: parked until the streams have passed this point (collect_pending_locked)
  c.unbatched.push_back(PendingBlock{p, device, bucket});
}

void dev_cache_context_created(int device, hipStream_t stream) {
  DevCache& c = dev_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  c.contexts++;
  c.streams.push_back({device, stream});
}
// the context's stream has been synchronised: its blocks join the shared pool
void dev_cache_context_destroyed(int device, hipStream_t stream) {
  DevCache& c = dev_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  for (size_t i = 0; i < c.streams.size(); i++)
    if (c.streams[i].first == device && c.streams[i].second == stream) {
      c.streams.erase(c.streams.begin() + i);
      break;
    }
  for (auto it = c.free_blocks.begin(); it != c.free_blocks.end();) {
    if (it->first.device == device && it->first.stream == stream && stream != nullptr) {
      auto& pool = c.free_blocks[{device, nullptr, it->first.bucket}];
      pool.insert(pool.end(), it->second.begin(), it->second.end());
      it = c.free_blocks.erase(it);
    } else {
      ++it;
    }
  }
  if (--c.contexts <= 0) {
    c.contexts = 0;
    release_cached_locked(c);
    for (hipEvent_t e : c.event_pool) (void)hipEventDestroy(e);
    c.event_pool.clear();
  }
}

}  // namespace sga

using namespace sga;

extern "C" {

void sga_allocator_stats(uint64_t out[5]) {
  DevCache& c = dev_cache();
  std::lock_guard<std::mutex> lock(c.mu);
  out[0] = c.n_malloc;
  out[1] = c.n_stream_hit;
  out[2] = c.n_pool_hit;
  out[3] = c.n_pending_hit;
  out[4] = c.n_deferred;
}

}  // extern "C"

// Host side of the C ABI (include/dietgpu_amd.h): argument checking, temp
// memory carving, one pinned-memory parameter upload per call, and the kernel
// launch sequences.  Everything is enqueued on the caller's stream; the only
// host synchronisation is checksum verification on decode (as upstream,
// GpuANSDecode.cuh:557-591) and the overflow-allocation fallback.
#include "../../include/dietgpu_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "format.h"
#include "kernel_variants.h"
#include "work_plan.h"

using namespace dgpu;

namespace {

thread_local std::string g_lastError;
// every batch member whose checksum did not match in this thread's last decode call (GpuANSDecode.cuh:581-590)
struct ChecksumMismatch {
  int32_t batch;
  uint32_t expected, got;
};
thread_local std::vector<ChecksumMismatch> g_mismatches;
thread_local const char* g_captureHint = nullptr;  // why a call cannot be captured into a HIP graph (set next to the error)

int fail(int code, const std::string& msg) {
  g_lastError = msg;
  return code;
}

#define DGPU_HIP(expr)                                                              \
  do {                                                                              \
    hipError_t e_ = (expr);                                                         \
    if (e_ != hipSuccess) {                                                         \
      return fail(DGPU_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    }                                                                               \
  } while (0)

#define DGPU_REQUIRE(cond, msg)                                      \
  do {                                                               \
    if (!(cond)) return fail(DGPU_ERR_INVALID_ARGUMENT, (msg));      \
  } while (0)

constexpr size_t kTempAlign = 256;  // kSDMAlignment, StackDeviceMemory.h:22

size_t alignUp(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------------------
// Optional per-kernel timing with HIP events on the launch stream (used by
// bench.py for the roofline figure; off by default, zero cost when off).
struct ProfSpan {
  const char* name;
  hipEvent_t start, stop;
};
struct ProfState {
  std::mutex mu;
  bool enabled = false;
  std::vector<ProfSpan> open;
  std::map<std::string, std::pair<uint64_t, double>> acc;  // name -> (launches, total ms)
};
ProfState& prof() {
  static ProfState* p = new ProfState();
  return *p;
}

class KernelTimer {
 public:
  KernelTimer(const char* name, hipStream_t stream) : stream_(stream) {
    ProfState& p = prof();
    if (!p.enabled) return;
    span_.name = name;
    // no system-scope fence at the events: it would write the L2 back around every kernel that is being timed
    if (hipEventCreateWithFlags(&span_.start, hipEventDisableSystemFence) != hipSuccess ||
        hipEventCreateWithFlags(&span_.stop, hipEventDisableSystemFence) != hipSuccess) return;
    (void)hipEventRecord(span_.start, stream_);
    active_ = true;
  }
  ~KernelTimer() {
    if (!active_) return;
    (void)hipEventRecord(span_.stop, stream_);
    ProfState& p = prof();
    std::lock_guard<std::mutex> g(p.mu);
    p.open.push_back(span_);
  }

 private:
  hipStream_t stream_;
  ProfSpan span_{};
  bool active_ = false;
};

#define DGPU_LAUNCH(name, stream, ...)   \
  do {                                   \
    KernelTimer kt_(name, stream);       \
    hipLaunchKernelGGL(__VA_ARGS__);     \
  } while (0)

// One launch of a kernel variant (kernel_variants.h) on `stream`.
template <typename... Args, typename... Given>
int launchVariant(const KernelVariant<Args...>& v, dim3 grid, hipStream_t stream, const Given&... args) {
  DGPU_LAUNCH(v.name, stream, v.fn, grid, dim3(v.threads), v.ldsBytes, stream, args...);
  DGPU_HIP(hipGetLastError());
  return DGPU_OK;
}

// ---------------------------------------------------------------------------
// Library-owned device state per (device, stream): everything a call needs that
// must outlive it or be zero when it starts.
//   * overflow slab: when the caller's temp memory is missing or too small the
//     reference falls back to cudaMalloc + cudaFree around every call
//     (synchronising, StackDeviceMemory.cpp:119-139).  Here the overflow comes
//     from a grow-only slab that is kept between calls: calls on one stream
//     execute in order, so every call can carve the slab from offset 0 without
//     synchronising.  A slab that has to grow in the middle of a call is RETIRED,
//     never freed under the call: allocations handed out earlier in the same call
//     live in it and their kernels have not even been launched yet.  Retired slabs
//     are freed by the NEXT call that needs overflow memory, after a stream
//     synchronise.
//   * arrival counters / accumulate-mode histogram counters of the histogram ->
//     normalisation hand-off, zero at rest.
// A call that touches this state holds `busy` from its first use until it has
// enqueued everything: two host threads enqueueing on the same stream would
// otherwise carve the same slab bytes for two calls whose kernels interleave.
// The registry is bounded: beyond kMaxStreams entries per process the idle ones
// are released after a device synchronise (streams come and go in long-running
// processes; their handles cannot be observed dying).
constexpr uint32_t kAccElements = 64;  // batches up to this size may use the accumulate-by-atomics histogram
struct StreamState {
  int device = 0;
  hipStream_t stream = nullptr;
  std::mutex busy;          // held by the call using this state
  uint64_t lastUse = 0;
  // overflow slab
  uint8_t* slab = nullptr;
  size_t slabCap = 0;
  std::vector<void*> retired;
  // slabs a CAPTURED call carved memory from: a HIP graph replays into them, so they outlive their retirement (until
  // dgpu_release_graph_state); slabInGraph: the current slab is such a slab
  bool slabInGraph = false;
  std::vector<void*> graphSlabs;
  // 65536 arrival counters + kAccElements x 256 histogram counters + 16384 spill-pool flags (zero at rest)
  uint32_t* counters = nullptr;
  // a call was CAPTURED into a HIP graph with pointers into this state (slab, counters): the graph replays without
  // passing through the library, so the state is never trimmed or released implicitly (dgpu_release_graph_state)
  bool graphPinned = false;

  void releaseDeviceMemory() {
    for (void* p : retired) (void)hipFree(p);
    retired.clear();
    for (void* p : graphSlabs) (void)hipFree(p);
    graphSlabs.clear();
    slabInGraph = false;
    if (slab) (void)hipFree(slab);
    if (counters) (void)hipFree(counters);
    slab = nullptr;
    slabCap = 0;
    counters = nullptr;
  }
};

class StreamRegistry {
 public:
  static constexpr size_t kMaxStreams = 32;
  // Returns the state of (current device, stream) with its `busy` mutex HELD, creating the state if necessary.
  // `busy` is taken (try_lock) while the registry mutex is held, so trimLocked() / release() -- which only drop
  // states whose `busy` they can take -- can never delete a state between its lookup and its use.  A state that is
  // busy (another host thread is enqueueing on the same stream) is waited for with the registry mutex released.
  // `create` false: nullptr (with *err == hipSuccess) when the stream has no state.
  StreamState* acquire(hipStream_t stream, hipError_t* err, bool create = true) {
    for (;;) {
      {
        std::lock_guard<std::mutex> g(mu_);
        int dev = 0;
        *err = hipGetDevice(&dev);
        if (*err != hipSuccess) return nullptr;
        auto key = std::make_pair(dev, stream);
        auto it = states_.find(key);
        if (it == states_.end()) {
          if (!create) return nullptr;
          if (states_.size() >= kMaxStreams) trimLocked();
          StreamState* s = new StreamState();
          s->device = dev;
          s->stream = stream;
          it = states_.emplace(key, s).first;
        }
        if (it->second->busy.try_lock()) {
          it->second->lastUse = ++clock_;
          return it->second;
        }
      }
      std::this_thread::yield();
    }
  }
  // Frees the device memory kept for `stream` on the current device (all streams
  // of all devices if `all`).  Synchronises first.  Returns the number of states released.
  // States captured into a HIP graph (graphPinned) are only released when `includeGraphPinned`.
  int release(hipStream_t stream, bool all, bool includeGraphPinned = false) {
    std::lock_guard<std::mutex> g(mu_);
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::vector<std::map<std::pair<int, hipStream_t>, StreamState*>::iterator> victims;
    for (auto it = states_.begin(); it != states_.end(); ++it) {
      StreamState* s = it->second;
      const bool match = all || (it->first.first == dev && it->first.second == stream);
      if (match && (includeGraphPinned || !s->graphPinned) && s->busy.try_lock()) victims.push_back(it);
    }
    return dropLocked(victims, dev);
  }
  size_t size() {
    std::lock_guard<std::mutex> g(mu_);
    return states_.size();
  }

 private:
  typedef std::map<std::pair<int, hipStream_t>, StreamState*>::iterator Iter;
  // `victims` hold their `busy`.  ONE device synchronise per device (nothing enqueued earlier can still be using
  // the memory afterwards); a device that cannot be synchronised keeps its memory (leaked, never freed under work).
  int dropLocked(const std::vector<Iter>& victims, int restoreDev) {
    std::map<int, bool> synced;
    for (Iter it : victims) {
      const int d = it->second->device;
      if (!synced.count(d)) synced[d] = hipSetDevice(d) == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
    int n = 0;
    for (Iter it : victims) {
      StreamState* s = it->second;
      if (synced[s->device] && hipSetDevice(s->device) == hipSuccess) {
        s->releaseDeviceMemory();
      } else {
        (void)hipGetLastError();
        s->slab = nullptr;  // cannot prove idleness: leak rather than free under running kernels
        s->counters = nullptr;
        s->retired.clear();
        s->graphSlabs.clear();
      }
      s->busy.unlock();
      delete s;
      states_.erase(it);
      ++n;
    }
    (void)hipSetDevice(restoreDev);
    return n;
  }
  // Drops the least recently used half of the idle states that no HIP graph refers to.
  void trimLocked() {
    std::vector<std::pair<uint64_t, Iter>> idle;
    for (auto it = states_.begin(); it != states_.end(); ++it) {
      if (!it->second->graphPinned) idle.push_back({it->second->lastUse, it});
    }
    std::sort(idle.begin(), idle.end(), [](const std::pair<uint64_t, Iter>& a, const std::pair<uint64_t, Iter>& b) { return a.first < b.first; });
    int cur = 0;
    (void)hipGetDevice(&cur);
    std::vector<Iter> victims;
    for (auto& e : idle) {
      if (victims.size() >= kMaxStreams / 2) break;
      if (e.second->second->busy.try_lock()) victims.push_back(e.second);
    }
    dropLocked(victims, cur);
  }
  std::mutex mu_;
  uint64_t clock_ = 0;
  std::map<std::pair<int, hipStream_t>, StreamState*> states_;
};

StreamRegistry& streamRegistry() {
  static StreamRegistry* r = new StreamRegistry();  // intentionally leaked: no teardown-order issues
  return *r;
}

// One call's hold on the stream state (taken lazily: calls whose temp memory
// suffices and that need no library-owned counters never touch it).
class StreamLease {
 public:
  explicit StreamLease(hipStream_t stream) : stream_(stream) {}
  StreamLease(const StreamLease&) = delete;
  StreamLease& operator=(const StreamLease&) = delete;
  ~StreamLease() {
    if (state_) state_->busy.unlock();
  }
  StreamState* state(hipError_t* err) {
    if (!state_) {
      StreamState* s = streamRegistry().acquire(stream_, err);  // returns with `busy` held
      if (!s) return nullptr;
      state_ = s;
      if (capturing()) s->graphPinned = true;
    }
    *err = hipSuccess;
    return state_;
  }
  hipStream_t stream() const { return stream_; }
  // Is the caller's stream being captured into a HIP graph?  Then nothing may synchronise or allocate, and every
  // library-owned address the kernels receive must stay valid for the life of the graph.
  bool capturing() {
    if (capturing_ < 0) {
      hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
      capturing_ = (hipStreamIsCapturing(stream_, &st) == hipSuccess && st == hipStreamCaptureStatusActive) ? 1 : 0;
      if (capturing_ == 0) (void)hipGetLastError();
    }
    return capturing_ == 1;
  }

 private:
  hipStream_t stream_;
  StreamState* state_ = nullptr;
  int capturing_ = -1;
};

// Temp memory: bump allocation out of the caller's region; what does not fit
// comes from the stream's overflow slab with a warning (StackDeviceMemory.cpp:119-139).
class TempArena {
 public:
  TempArena(void* base, size_t bytes, StreamLease& lease)
      : base_((uint8_t*)base), bytes_(base ? bytes : 0), lease_(lease) {
    // honour the 256-byte granularity even if the caller's pointer is odd
    size_t mis = ((uintptr_t)base_) % kTempAlign;
    if (base_ && mis) {
      size_t skip = kTempAlign - mis;
      if (skip >= bytes_) {
        base_ = nullptr;
        bytes_ = 0;
      } else {
        base_ += skip;
        bytes_ -= skip;
      }
    }
  }

  template <typename T>
  T* alloc(size_t count, hipError_t* err) {
    size_t need = std::max(alignUp(count * sizeof(T), kTempAlign), kTempAlign);
    requested_ += need;
    if (head_ + need <= bytes_) {
      T* p = (T*)(base_ + head_);
      head_ += need;
      return p;
    }
    // no warning when the caller chose to pass no temp memory at all
    if (!warned_ && bytes_ > 0) {
      fprintf(stderr,
              "dietgpu_amd: WARNING: temp memory too small (%zu bytes given, > %zu needed); "
              "using library-owned overflow memory\n",
              bytes_, requested_);
      warned_ = true;
    }
    return (T*)overflow(need, err);
  }

  size_t requested() const { return requested_; }

 private:
  void* overflow(size_t need, hipError_t* err) {
    StreamState* s = lease_.state(err);
    if (!s) return nullptr;
    if (!overflowUsed_) {
      overflowUsed_ = true;
      // first overflow allocation of this call: slabs retired by EARLIER calls can go
      // (their kernels precede everything this call enqueues on the stream) -- not while the stream is being
      // captured: a synchronise would invalidate the capture, they wait for the next plain call.  Slabs that a
      // captured call carved memory from are not in this list: a graph replays with their address (graphSlabs).
      if (!s->retired.empty() && !lease_.capturing()) {
        *err = hipStreamSynchronize(lease_.stream());
        if (*err != hipSuccess) return nullptr;
        for (void* p : s->retired) (void)hipFree(p);
        s->retired.clear();
      }
    }
    if (overflowHead_ + need > s->slabCap) {
      if (lease_.capturing()) {
        // growing the slab means hipMalloc in the middle of a stream capture
        *err = hipErrorStreamCaptureUnsupported;
        g_captureHint = "temp memory: the library-owned overflow slab would have to grow while the stream is being "
                        "captured into a HIP graph; pass enough temp memory, or run the same call once before capturing";
        return nullptr;
      }
      const size_t cap = std::max<size_t>(std::max(2 * s->slabCap, need + (need >> 2)), (size_t)8 << 20);
      void* p = nullptr;
      *err = hipMalloc(&p, cap);
      if (*err != hipSuccess) return nullptr;
      // the old slab may hold allocations of THIS call: retire it, never free it here; one that a HIP graph replays
      // into stays until dgpu_release_graph_state() ("neither evicted nor trimmed nor released", dietgpu_amd.h)
      if (s->slab) (s->slabInGraph ? s->graphSlabs : s->retired).push_back(s->slab);
      s->slabInGraph = false;
      s->slab = (uint8_t*)p;
      s->slabCap = cap;
      overflowHead_ = 0;
    }
    if (lease_.capturing()) s->slabInGraph = true;
    void* out = s->slab + overflowHead_;
    overflowHead_ += need;
    return out;
  }

  uint8_t* base_;
  size_t bytes_;
  StreamLease& lease_;
  size_t head_ = 0;
  size_t overflowHead_ = 0;
  size_t requested_ = 0;
  bool warned_ = false;
  bool overflowUsed_ = false;
};

#define DGPU_ALLOC(var, T, arena, count)                                     \
  T* var = nullptr;                                                          \
  do {                                                                       \
    hipError_t e_ = hipSuccess;                                              \
    var = (arena).alloc<T>((count), &e_);                                    \
    if (!var) return fail(DGPU_ERR_HIP, std::string("temp alloc: ") + (e_ == hipErrorStreamCaptureUnsupported && g_captureHint ? g_captureHint : hipGetErrorString(e_))); \
  } while (0)

// ---------------------------------------------------------------------------
// Host->device parameter upload (pointer / size arrays).
//
// The pointer-array entry points take HOST arrays (as the reference's do) that
// the kernels need in device memory.  A call's arrays are packed into one block
// and looked up in a small per-device cache of blocks already resident on the
// device: a training or collective loop compresses the same buffers step after
// step, and then nothing is uploaded at all.  A miss copies the block with one
// hipMemcpyAsync from pinned memory on the caller's stream (a ~3 us blit ahead of
// the first kernel; a side-stream copy + event wait measured slower).
//
// Lifetime rules:
//   * an entry is pinned (not evictable) while a call is being enqueued with it
//   * a miss records `released` on the caller's stream when the call has been
//     enqueued; eviction waits for it (it is 8 calls old by then)
//   * a hit records nothing; the entry remembers every stream that hit it, and
//     evicting it synchronises those streams first (rare: LRU)
//   * a hit from a stream other than the uploading one waits on `copied`
std::atomic<bool> g_paramCacheEnabled{true};  // dgpu_debug_set_param_cache

class ParamCache {
 public:
  struct Entry {
    void* host = nullptr;  // pinned; also the comparison copy
    void* dev = nullptr;
    size_t cap = 0;
    size_t bytes = 0;
    uint64_t hash = 0;
    uint64_t lastUse = 0;
    int pins = 0;
    hipEvent_t copied = nullptr;
    hipEvent_t released = nullptr;
    hipStream_t uploadStream = nullptr;
    std::vector<hipStream_t> hitStreams;  // every stream that hit this entry since its upload
    bool syncAllBeforeReuse = false;      // completion could not be tracked: device synchronise before reuse
    bool everUsed = false;
    bool graphPinned = false;             // a HIP graph holds entry->dev: never evicted (dgpu_release_graph_state)
  };

  // Returns a pinned entry holding `block`; *miss tells the caller to record `released`.
  // `capturing`: the stream is being captured into a HIP graph.  The graph will replay with entry->dev baked into
  // its kernel arguments without ever passing through acquire() again, so the entry is pinned for good; and nothing
  // here may synchronise, allocate or blit then, so only a block that is already resident (a hit) can be captured.
  hipError_t acquire(const uint8_t* block, size_t bytes, hipStream_t stream, Entry** out, bool* miss, bool capturing = false) {
    const uint64_t h = hashBlock(block, bytes);
    std::lock_guard<std::mutex> g(mu_);
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::vector<Entry*>& entries = perDevice_[dev];
    ++clock_;
    for (Entry* en : entries) {
      if (!g_paramCacheEnabled.load()) break;  // measurement hook: upload on every call
      if (en->everUsed && en->hash == h && en->bytes == bytes && memcmp(en->host, block, bytes) == 0) {
        if (stream != en->uploadStream && hipEventQuery(en->copied) != hipSuccess) {
          e = hipStreamWaitEvent(stream, en->copied, 0);
          if (e != hipSuccess) return e;
        }
        en->lastUse = clock_;
        en->pins++;
        if (capturing && !en->graphPinned) {
          en->graphPinned = true;
          en->pins++;  // never released: the entry stays where it is for the life of the graph
        }
        if (std::find(en->hitStreams.begin(), en->hitStreams.end(), stream) == en->hitStreams.end()) {
          en->hitStreams.push_back(stream);
        }
        *out = en;
        *miss = false;
        return hipSuccess;
      }
    }
    if (capturing) {
      g_captureHint = "the call's pointer / size arrays are not resident on the device yet and cannot be uploaded while the "
                      "stream is being captured into a HIP graph: run the same call once before capturing";
      return hipErrorStreamCaptureUnsupported;
    }
    // miss: least recently used unpinned entry, or a new one while the cache is small
    Entry* victim = nullptr;
    if (entries.size() >= kEntries) {
      for (Entry* en : entries) {
        if (en->pins == 0 && (!victim || en->lastUse < victim->lastUse)) victim = en;
      }
    }
    if (!victim) {
      victim = new Entry();
      entries.push_back(victim);
    }
    if (victim->everUsed) {
      // kernels of every call that used this block must be done with it: hits record
      // nothing, so synchronise each stream that hit it (rare: LRU eviction of a block
      // that was still in use a few calls ago)
      bool needDeviceSync = victim->syncAllBeforeReuse;
      for (hipStream_t hs : victim->hitStreams) {
        if (needDeviceSync) break;
        if (hipStreamSynchronize(hs) != hipSuccess) {
          (void)hipGetLastError();
          needDeviceSync = true;  // the stream may be gone
        }
      }
      if (needDeviceSync) {
        e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
      } else {
        e = hipEventSynchronize(victim->released);
        if (e != hipSuccess) return e;
      }
    }
    if (victim->cap < bytes) {
      if (victim->host) (void)hipHostFree(victim->host);
      if (victim->dev) (void)hipFree(victim->dev);
      victim->host = victim->dev = nullptr;
      victim->cap = 0;
      const size_t cap = std::max<size_t>(alignUp(bytes, 4096), 16384);
      e = hipHostMalloc(&victim->host, cap, hipHostMallocDefault);
      if (e != hipSuccess) return e;
      e = hipMalloc(&victim->dev, cap);
      if (e != hipSuccess) return e;
      victim->cap = cap;
    }
    if (!victim->copied) {
      // ordering only (a later stream's kernels after the blit; the host asking whether the call is done): no
      // system-scope fence, which costs a cache write-back per record and slows the kernels that follow
      e = hipEventCreateWithFlags(&victim->copied, hipEventDisableTiming | hipEventDisableSystemFence);
      if (e != hipSuccess) return e;
      e = hipEventCreateWithFlags(&victim->released, hipEventDisableTiming | hipEventDisableSystemFence);
      if (e != hipSuccess) return e;
    }
    memcpy(victim->host, block, bytes);
    victim->bytes = bytes;
    victim->hash = h;
    victim->everUsed = false;  // not matchable until the copy has been enqueued
    e = hipMemcpyAsync(victim->dev, victim->host, bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return e;
    e = hipEventRecord(victim->copied, stream);
    if (e != hipSuccess) return e;
    victim->everUsed = true;
    victim->uploadStream = stream;
    victim->hitStreams.clear();
    victim->syncAllBeforeReuse = false;
    victim->lastUse = clock_;
    victim->pins++;
    *out = victim;
    *miss = true;
    return hipSuccess;
  }

  // Makes the blocks HIP graphs were captured with evictable again (the caller has destroyed those graphs).
  int releaseGraphPins() {
    std::lock_guard<std::mutex> g(mu_);
    int n = 0;
    for (auto& kv : perDevice_) {
      for (Entry* en : kv.second) {
        if (en->graphPinned) {
          en->graphPinned = false;
          en->pins--;
          ++n;
        }
      }
    }
    return n;
  }

  void release(Entry* en, bool miss, hipStream_t stream) {
    std::lock_guard<std::mutex> g(mu_);
    if (miss) {
      if (hipEventRecord(en->released, stream) != hipSuccess) {
        // cannot track completion: never reuse this entry without a full sync
        en->syncAllBeforeReuse = true;
      }
    }
    en->pins--;
  }

 private:
  static constexpr size_t kEntries = 16;
  // (four independent lanes: a batch of tens of thousands of tensors has a parameter block of a megabyte, and one
  // multiply-xor chain over it was most of such a call's host time)
  static uint64_t hashBlock(const uint8_t* p, size_t n) {
    uint64_t h0 = 0x9e3779b97f4a7c15ull ^ n, h1 = 0xc2b2ae3d27d4eb4full, h2 = 0x165667b19e3779f9ull, h3 = 0x27d4eb2f165667c5ull;
    size_t i = 0;
    for (; i + 32 <= n; i += 32) {
      uint64_t w[4];
      memcpy(w, p + i, 32);
      h0 = (h0 ^ w[0]) * 0xff51afd7ed558ccdull;
      h1 = (h1 ^ w[1]) * 0xff51afd7ed558ccdull;
      h2 = (h2 ^ w[2]) * 0xff51afd7ed558ccdull;
      h3 = (h3 ^ w[3]) * 0xff51afd7ed558ccdull;
      h0 ^= h0 >> 32;
      h1 ^= h1 >> 32;
      h2 ^= h2 >> 32;
      h3 ^= h3 >> 32;
    }
    uint64_t h = h0 ^ (h1 * 3u) ^ (h2 * 5u) ^ (h3 * 7u);
    for (; i + 8 <= n; i += 8) {
      uint64_t w;
      memcpy(&w, p + i, 8);
      h = (h ^ w) * 0xff51afd7ed558ccdull;
      h ^= h >> 32;
    }
    for (; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
  }
  std::mutex mu_;
  uint64_t clock_ = 0;
  std::map<int, std::vector<Entry*>> perDevice_;
};

ParamCache& paramCache() {
  static ParamCache* c = new ParamCache();  // intentionally leaked: no teardown-order issues
  return *c;
}

// Unpins the parameter block of a call (and, after an upload, records when the
// call's kernels are done with it) once everything has been enqueued.
class ParamLease {
 public:
  ParamLease() = default;
  ParamLease(const ParamLease&) = delete;
  ParamLease& operator=(const ParamLease&) = delete;
  ~ParamLease() {
    if (entry_) paramCache().release(entry_, miss_, stream_);
  }
  void bind(ParamCache::Entry* e, bool miss, hipStream_t stream) {
    entry_ = e;
    miss_ = miss;
    stream_ = stream;
  }

 private:
  ParamCache::Entry* entry_ = nullptr;
  bool miss_ = false;
  hipStream_t stream_ = nullptr;
};

BatchView viewStride(const void* base, uint64_t stride, uint32_t uniformSize) {
  BatchView v;
  v.ptrs = nullptr;
  v.base = (uint64_t)(uintptr_t)base;
  v.stride = stride;
  v.sizes = nullptr;
  v.uniformSize = uniformSize;
  return v;
}

BatchView viewPointers(const uint64_t* ptrs_dev, const uint32_t* sizes_dev, uint32_t uniformSize) {
  BatchView v;
  v.ptrs = ptrs_dev;
  v.base = 0;
  v.stride = 0;
  v.sizes = sizes_dev;
  v.uniformSize = uniformSize;
  return v;
}

// Workgroups per element of the internal histogram pass.  The hand-off to the
// normalisation costs a few microseconds per workgroup (write-through + arrival
// atomic), so workgroups should be long; two per CU already saturate HBM.  With
// a large batch that is a few long workgroups per element, with a single large
// tensor up to 256 of them.
// Raw bytes carry twice the symbols (LDS atomics, address arithmetic) per byte of traffic: three workgroups per CU
// (256 x 1 MiB Zipf bytes: 53.9 -> 51.3 us; the exponent histogram loses 2 us with three).
constexpr uint32_t kHistTargetWgs = 512, kHistTargetWgsRaw = 768, kHistAccWgs = 512, kHistAccMaxBatch = 2;
// (The counters of an element in 16 sets instead of one -- so that 512 workgroups do not queue on 256 addresses -- measured
// SLOWER: 1 x 128 Mi bf16 histogram 49.3 us against 47.9, 1 x 16 Mi 18.4-19.5 against 16.6-16.9
// (profiles/r06_ab_hist_acc_sets_*.txt): summing the sets costs the normalising workgroup more than the queue does.)
uint32_t histPartsFor(uint32_t B, uint32_t maxBytes, bool raw) {
  const uint32_t bySize = divUp(std::max(maxBytes, 1u), 32u * 1024u);
  const uint32_t byBatch = divUp(raw ? kHistTargetWgsRaw : kHistTargetWgs, std::max(B, 1u));
  return std::max(1u, std::min(std::min(bySize, byBatch), 256u));
}
// One or two large elements: the counts of an element's workgroups meet in 256 library-owned
// atomic counters instead of per-workgroup partial histograms, so an element can be spread over
// ~512 workgroups without the normalising workgroup having to sum 512 partial histograms (a single
// 256 MiB tensor: 79 -> 52 us; more workgroups than that lose to contention on the counters).
bool histAccumulates(uint32_t B, uint32_t maxBytes, bool raw);
uint32_t histPartsAccFor(uint32_t B, uint32_t maxBytes) {
  const uint32_t bySize = divUp(std::max(maxBytes, 1u), 64u * 1024u);
  const uint32_t byBatch = divUp(kHistAccWgs, std::max(B, 1u));
  return std::max(1u, std::min(bySize, byBatch));
}

uint32_t gridX(uint32_t maxBytes, uint32_t bytesPerBlock, uint32_t cap) {
  uint32_t x = divUp(std::max(maxBytes, 1u), bytesPerBlock);
  return std::max(1u, std::min(x, cap));
}

bool validProbBits(int p) { return p == 9 || p == 10 || p == 11; }
bool validFloatType(uint32_t ft) { return ft == kFloat16 || ft == kBFloat16 || ft == kFloat32; }
const char* const kMsgFloatType = "floatType must be float16, bfloat16 or float32";

// getMaxCompressedSize, GpuANSEncode.cu:13-25 (block SIZE passed as block COUNT [sic]).  Upstream CHECKs the result
// against INT32_MAX (GpuANSEncode.cu:22: inputs beyond 419 321 blocks = 1 717 538 816 bytes abort); here such a size
// yields 0 and the encode entry points reject it.
constexpr uint32_t kMaxEncodableBytes = 419321u * kBlockSize;
uint32_t maxCompressedSizeHost(uint32_t bytes) {
  uint32_t blocks = divUp(bytes, kBlockSize);
  size_t raw = ansOverhead(kBlockSize);
  raw += (size_t)roundUp(kBlockSize + kBlockSize / 4, 16) * blocks;
  raw = alignUp(raw, 16);
  if (raw > (size_t)INT32_MAX) return 0u;
  return (uint32_t)raw;
}
bool encodableSize(uint32_t symbols) { return symbols <= kMaxEncodableBytes; }

// One call's batch as its entry point describes it: HOST arrays of device pointers and sizes (packed and uploaded as
// [in ptrs][out ptrs][sizes][inBytes][work][residual ptrs], the block the parameter cache hashes) or, when `strided`, two
// stride views.
struct Batch {
  uint32_t n = 0;  // elements
  bool strided = false;
  BatchView in, out;  // strided
  std::vector<uint64_t> inPtrs, outPtrs;
  std::vector<uint32_t> sizes;    // input sizes (encode) or output capacities (decode)
  std::vector<uint32_t> inBytes;  // decode, *_bounded entry points: bytes available per compressed input
  uint32_t uniformInBytes = 0;    // ... of a strided decode (0 = unknown)
  std::vector<uint32_t> work;     // work lists of a batch whose elements differ widely in size (work_plan.h)
  uint32_t maxSize = 0;           // the largest size / capacity
  // dgpu_float_feedback_compress: the residual that is added (empty: none yet) and the one that is stored, per element
  std::vector<uint64_t> resInPtrs, resOutPtrs;
};

// One side of a batch as an entry point receives it: a HOST array of device pointers, or (ptrs == nullptr) a base and
// a stride; every address must be a multiple of `align` (the stride from the second element on), `msg` says so.
struct Side {
  const void* const* ptrs;
  const void* base;
  uint64_t stride;
  uint32_t align;
  const char* msg;
};
const char* const kMsgCompIn = "compressed input must be 16-byte aligned";
const char* const kMsgCompOut = "compressed output must be 16-byte aligned";
const char* const kMsgAnsIn = "ANS input must be 4-byte aligned";
const char* const kMsgFloatIn = "float input must be float-word aligned";

Side ptrSide(const void* const* ptrs, uint32_t align = 1, const char* msg = "") { return Side{ptrs, nullptr, 0, align, msg}; }
Side strideSide(const void* base, uint64_t stride, uint32_t align = 1, const char* msg = "") { return Side{nullptr, base, stride, align, msg}; }

int sideAligned(const Side& s, uint32_t B) {
  DGPU_REQUIRE(s.ptrs || ((uintptr_t)s.base % s.align == 0 && (B <= 1 || s.stride % s.align == 0)), s.msg);
  return DGPU_OK;
}
int sideAddresses(const Side& s, uint32_t B, std::vector<uint64_t>* addr) {
  if (int rc = sideAligned(s, B)) return rc;
  addr->resize(B);
  for (uint32_t i = 0; i < B; ++i) {
    (*addr)[i] = s.ptrs ? (uint64_t)(uintptr_t)s.ptrs[i] : (uint64_t)(uintptr_t)s.base + i * s.stride;
    DGPU_REQUIRE(!s.ptrs || (*addr)[i] % s.align == 0, s.msg);
  }
  return DGPU_OK;
}

// The three shapes a batch arrives in.  sizesOnOut: `size` / `sizes` are output capacities (decode) rather than input
// sizes (encode).
int strideBatch(Batch* b, uint32_t B, const Side& in, const Side& out, uint32_t size, bool sizesOnOut, uint32_t inBytes = 0) {
  if (int rc = sideAligned(in, B)) return rc;
  if (int rc = sideAligned(out, B)) return rc;
  b->n = B;
  b->strided = true;
  b->in = viewStride(in.base, in.stride, sizesOnOut ? 0u : size);
  b->out = viewStride(out.base, out.stride, sizesOnOut ? size : 0u);
  b->uniformInBytes = inBytes;
  b->maxSize = size;
  return DGPU_OK;
}
int pointerBatch(Batch* b, uint32_t B, const Side& in, const Side& out, const uint32_t* sizes, const uint32_t* inBytes = nullptr) {
  int rc = sideAddresses(in, B, &b->inPtrs);
  if (!rc) rc = sideAddresses(out, B, &b->outPtrs);
  if (rc) return rc;
  b->n = B;
  b->sizes.assign(sizes, sizes + B);
  if (inBytes) b->inBytes.assign(inBytes, inBytes + B);
  for (uint32_t i = 0; i < B; ++i) b->maxSize = std::max(b->maxSize, sizes[i]);
  return DGPU_OK;
}
// `split`: one buffer cut into B elements of splitSizes[i] words of wordBytes, the input (encode) or the output
// (splitOnOut); interiorAlign != 0: every element but the last must be a multiple of it (alignment rules of
// GpuANSEncode.cu:132-140)
int splitBatch(Batch* b, uint32_t B, const Side& split, const uint32_t* splitSizes, uint32_t wordBytes, uint32_t interiorAlign,
               const Side& other, bool splitOnOut, const uint32_t* inBytes = nullptr) {
  if (int rc = sideAligned(split, 1)) return rc;
  for (uint32_t i = 0; i + 1 < B && interiorAlign; ++i) {
    DGPU_REQUIRE(splitSizes[i] % interiorAlign == 0, "interior split sizes must be multiples of 4 bytes");
  }
  int rc = sideAddresses(other, B, splitOnOut ? &b->inPtrs : &b->outPtrs);
  if (rc) return rc;
  std::vector<uint64_t>& ptrs = splitOnOut ? b->outPtrs : b->inPtrs;
  ptrs.resize(B);
  b->n = B;
  b->sizes.assign(splitSizes, splitSizes + B);
  if (inBytes) b->inBytes.assign(inBytes, inBytes + B);
  uint64_t prefix = 0;
  for (uint32_t i = 0; i < B; ++i) {
    ptrs[i] = (uint64_t)(uintptr_t)split.base + prefix * wordBytes;
    prefix += splitSizes[i];
    b->maxSize = std::max(b->maxSize, splitSizes[i]);
  }
  return DGPU_OK;
}

// A batch as the kernels see it: device views, the device copies of inBytes and work, and the hold on the parameter
// block they live in.
struct DeviceBatch {
  BatchView in, out;
  const uint32_t* inBytes = nullptr;
  const uint32_t* work = nullptr;
  BatchView resIn{}, resOut{};  // feedback calls (all zero: no such side)
  ParamLease lease;
};

int uploadParams(const Batch& b, bool sizesOnOut, StreamLease& stream, DeviceBatch* d) {
  const size_t outAt = b.inPtrs.size() * 8, sizesAt = outAt + b.outPtrs.size() * 8, inBytesAt = sizesAt + alignUp(b.sizes.size() * 4, 8),
               workAt = inBytesAt + alignUp(b.inBytes.size() * 4, 8), resInAt = workAt + alignUp(b.work.size() * 4, 8),
               resOutAt = resInAt + b.resInPtrs.size() * 8, bytes = resOutAt + b.resOutPtrs.size() * 8;
  if (bytes == 0) return DGPU_OK;
  static thread_local std::vector<uint8_t> block;
  block.assign(bytes, 0);
  uint8_t* h = block.data();
  if (outAt) memcpy(h, b.inPtrs.data(), outAt);
  if (sizesAt > outAt) memcpy(h + outAt, b.outPtrs.data(), sizesAt - outAt);
  if (!b.sizes.empty()) memcpy(h + sizesAt, b.sizes.data(), b.sizes.size() * 4);
  if (!b.inBytes.empty()) memcpy(h + inBytesAt, b.inBytes.data(), b.inBytes.size() * 4);
  if (!b.work.empty()) memcpy(h + workAt, b.work.data(), b.work.size() * 4);
  if (!b.resInPtrs.empty()) memcpy(h + resInAt, b.resInPtrs.data(), b.resInPtrs.size() * 8);
  if (!b.resOutPtrs.empty()) memcpy(h + resOutAt, b.resOutPtrs.data(), b.resOutPtrs.size() * 8);
  ParamCache::Entry* entry = nullptr;
  bool miss = false;
  const bool capturing = stream.capturing();
  const hipError_t ae = paramCache().acquire(h, bytes, stream.stream(), &entry, &miss, capturing);
  if (ae == hipErrorStreamCaptureUnsupported && capturing && g_captureHint) return fail(DGPU_ERR_HIP, std::string("HIP graph capture: ") + g_captureHint);
  DGPU_HIP(ae);
  d->lease.bind(entry, miss, stream.stream());
  const uint8_t* dev = (const uint8_t*)entry->dev;
  auto at = [dev](size_t offset, bool present) { return present ? dev + offset : nullptr; };
  const uint32_t* sizes = (const uint32_t*)at(sizesAt, !b.sizes.empty());
  d->in = viewPointers((const uint64_t*)at(0, outAt != 0), sizesOnOut ? nullptr : sizes, 0);
  d->out = viewPointers((const uint64_t*)at(outAt, sizesAt > outAt), sizesOnOut ? sizes : nullptr, 0);
  d->inBytes = (const uint32_t*)at(inBytesAt, !b.inBytes.empty());
  d->work = (const uint32_t*)at(workAt, !b.work.empty());
  if (!b.resInPtrs.empty()) d->resIn = viewPointers((const uint64_t*)at(resInAt, true), nullptr, 0);
  if (!b.resOutPtrs.empty()) d->resOut = viewPointers((const uint64_t*)at(resOutAt, true), nullptr, 0);
  return DGPU_OK;
}

// A pointer batch whose addresses form an arithmetic progression and whose sizes are all equal IS a stride batch
// (the rows of one tensor, the rows of the output matrix the tensor API allocates, any batch of one): it needs no
// parameter block on the device at all -- no cache lookup, and no blit + event records when the cache would miss
// (+9 us per call).  sizesOnOut: the sizes are output capacities (decode) rather than input sizes (encode).
bool progression(const std::vector<uint64_t>& p, uint64_t* stride) {
  *stride = p.size() > 1 ? p[1] - p[0] : 0;
  for (size_t i = 1; i < p.size(); ++i) {
    if (p[i] - p[i - 1] != *stride) return false;
  }
  return !p.empty();
}
// THE RULE: a batch with inBytes is never turned into stride views (a stride view carries one uniformInBytes at most);
// nor is one whose sides differ in length (the info calls: archive pointers only).
bool asStrideViews(const Batch& b, bool sizesOnOut, BatchView* in, BatchView* out) {
  if (!b.inBytes.empty() || b.inPtrs.size() != b.outPtrs.size()) return false;
  uint64_t inStride = 0, outStride = 0;
  if (!progression(b.inPtrs, &inStride) || !progression(b.outPtrs, &outStride)) return false;
  uint32_t u = b.sizes.empty() ? 0u : b.sizes[0];
  for (uint32_t sz : b.sizes) {
    if (sz != u) return false;
  }
  *in = viewStride((const void*)(uintptr_t)b.inPtrs[0], inStride, sizesOnOut ? 0u : u);
  *out = viewStride((const void*)(uintptr_t)b.outPtrs[0], outStride, sizesOnOut ? u : 0u);
  return true;
}
// ... and the residual sides of a feedback call, which must be progressions too
bool residualStrideViews(const Batch& b, BatchView* resIn, BatchView* resOut) {
  uint64_t inStride = 0, outStride = 0;
  if (!b.resInPtrs.empty() && !progression(b.resInPtrs, &inStride)) return false;
  if (!b.resOutPtrs.empty() && !progression(b.resOutPtrs, &outStride)) return false;
  if (!b.resInPtrs.empty()) *resIn = viewStride((const void*)(uintptr_t)b.resInPtrs[0], inStride, 0u);
  if (!b.resOutPtrs.empty()) *resOut = viewStride((const void*)(uintptr_t)b.resOutPtrs[0], outStride, 0u);
  return true;
}

// How a batch reaches the kernels: the caller's stride views, stride views of a pointer batch that is a progression, or
// the uploaded block -- then with the work lists `planWork` puts into b.work (only then: a progression has equal sizes).
// Whatever b.work holds is uploaded and hashed with the block: a planner that does not apply must leave it as it was
// (every planner here does: they return false before they touch it, or clear it).
template <typename PlanWork>
int resolveBatch(Batch& b, bool sizesOnOut, StreamLease& stream, DeviceBatch* d, PlanWork planWork) {
  if (b.strided) {
    d->in = b.in;
    d->out = b.out;
    return DGPU_OK;
  }
  if (asStrideViews(b, sizesOnOut, &d->in, &d->out) && residualStrideViews(b, &d->resIn, &d->resOut)) return DGPU_OK;
  d->resIn = d->resOut = BatchView{};
  planWork();
  return uploadParams(b, sizesOnOut, stream, d);
}
int resolveBatch(Batch& b, bool sizesOnOut, StreamLease& stream, DeviceBatch* d) {
  return resolveBatch(b, sizesOnOut, stream, d, [] {});
}

// What every codec entry point checks before anything else, the reset of its out-parameters and the end of an empty
// batch: *done says the call is over with the code returned.  ft: 0 = raw bytes; tooLarge (encoders): the refusal of
// more than the encodable `maxSize` symbols.
int checkCall(int P, uint32_t B, uint32_t ft, size_t* tempUsed, int32_t* errBatch, bool* done, const char* tooLarge = nullptr, uint32_t maxSize = 0) {
  *done = true;
  DGPU_REQUIRE(validProbBits(P), "probBits must be 9, 10 or 11");
  DGPU_REQUIRE(ft == 0 || validFloatType(ft), kMsgFloatType);
  DGPU_REQUIRE(B <= 65535u, "numInBatch must be <= 65535");
  DGPU_REQUIRE(!tooLarge || encodableSize(maxSize), tooLarge);
  if (tempUsed) *tempUsed = 0;
  if (errBatch) *errBatch = -1;
  *done = B == 0;
  return DGPU_OK;
}

// ---------------------------------------------------------------------------
// Launch sequences
// ---------------------------------------------------------------------------

uint32_t numComputeUnits() {
  static std::mutex mu;
  static std::map<int, uint32_t> cus;
  std::lock_guard<std::mutex> g(mu);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  hipDeviceProp_t prop;
  uint32_t n = 256;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) n = (uint32_t)prop.multiProcessorCount;
  cus[dev] = n;
  return n;
}

// The workgroups of `v` that are on the chip at once when `workgroups` of them are launched: the grid of a persistent
// launch, and the wavefronts that can hold spill slots at a time.
template <typename... Args>
uint32_t residentWorkgroups(const KernelVariant<Args...>& v, uint32_t workgroups) {
  return std::max(1u, std::min(workgroups, workgroupsPerCu(v) * numComputeUnits()));
}

// The wide stage (five workgroups per CU, no flushes on N(0,1) exponents) for persistent 8-block bf16 / fp32 tiles of
// batches whose elements have few tiles; elements of many tiles keep six workgroups per CU in flight behind their
// in-order commit (kernels_encode.h, kSpillStageWordsWide; profiles/r06_ab_encoder_five_per_cu_*.txt).
constexpr uint32_t kWideStageMaxTiles = 32;

uint32_t absentWorkgroupModulo();  // test hook, defined with the C ABI below

// start value of a test / A-B hook: the environment variable, or `otherwise`
int envInt(const char* name, int otherwise) {
  const char* e = getenv(name);
  return e && *e ? atoi(e) : otherwise;
}

// How the workgroups of the tiled encoder come to their tiles: persistent workgroups with a static ticket map, or one
// workgroup per tile, dispatched by the hardware in ticket order.  Measured on MI355X
// (profiles/r05_ab_encoder_hw_dispatch.txt, r05_ab_small_tiles_hw_dispatch.txt, r05_ab_pair_encoder_hw_dispatch.txt):
//   * raw bytes, 256 x 1 MiB: 152.7 -> 141.5 us under hardware dispatch (8192 tiles on 768 resident workgroups: the
//     compute-bound row loop of a slow CU no longer holds a fixed share of them);
//   * float tiles of 2 / 4 blocks (batches of elements of <= 16 Ki words): 118 -> 96 us / 98 -> 88 us;
//   * 8-block float tiles: nothing on 256 x 512 Ki, 1-3 % slower on few large tensors: they stay persistent;
//   * k_ans_encode_pair (single-block elements) always runs one workgroup per pair: 133.7 -> 96.8 us.
// -1 = this policy; dgpu_debug_set_encoder_dispatch / DGPU_ENC_DISPATCH force 0 (persistent) or 1 (hardware) where the
// kernel exists in both forms (tests, A/B runs).
std::atomic<int> g_encDispatch{envInt("DGPU_ENC_DISPATCH", -1)};
bool encoderHardwareDispatch(uint32_t numTickets, uint32_t resident) {
  const int m = g_encDispatch.load();
  if (m >= 0) return m != 0;
  return numTickets > resident;  // more tiles than slots: let the hardware balance them
}

// Work planning -- tile geometry, the work lists of ragged batches, size classes -- is host arithmetic in work_plan.h.
// Its two test hooks live here: dgpu_debug_set_work_lists / DGPU_WORK_LISTS and dgpu_debug_set_size_classes /
// DGPU_SIZE_CLASSES force lists / classes on (1: wherever the batch has a size array) or off (0); -1 = the policy.
std::atomic<int> g_workLists{envInt("DGPU_WORK_LISTS", -1)};
std::atomic<int> g_sizeClasses{envInt("DGPU_SIZE_CLASSES", -1)};
PlanPolicy planPolicy() { return {g_workLists.load(), g_sizeClasses.load()}; }

bool histAccumulates(uint32_t B, uint32_t maxBytes, bool raw) {
  return B <= kHistAccMaxBatch && histPartsAccFor(B, maxBytes) > histPartsFor(B, maxBytes, raw);
}

// Library-owned arrival counters for the histogram -> normalisation hand-off
// (HistFuse): 65536 u32 per (device, stream), zero at rest -- the kernel that uses
// them puts them back to zero.  Keyed by stream because calls on one stream are
// ordered while calls on different streams may overlap.
constexpr size_t kCounterWordsArrive = 65536;
constexpr size_t kCounterWordsAcc = (size_t)kAccElements * kNumSymbols;
constexpr size_t kCounterWordsSpill = 16384;  // flags of the hardware-dispatched encoders' spill-slot pool (kernels_encode.h: SpillPool)
int arrivalCounters(StreamLease& lease, uint32_t** out, uint32_t** acc, uint32_t** spillFlags = nullptr) {
  hipError_t e = hipSuccess;
  StreamState* s = lease.state(&e);
  if (!s) return fail(DGPU_ERR_HIP, std::string("stream state: ") + hipGetErrorString(e));
  if (!s->counters) {
    if (lease.capturing()) {
      return fail(DGPU_ERR_HIP, "HIP graph capture: the stream's hand-off counters do not exist yet and cannot be allocated while "
                                "the stream is being captured: run the same call once before capturing");
    }
    uint32_t* p = nullptr;
    const size_t words = kCounterWordsArrive + kCounterWordsAcc + kCounterWordsSpill;
    DGPU_HIP(hipMalloc((void**)&p, words * sizeof(uint32_t)));
    // once per (device, stream), ordered on the caller's stream ahead of the kernels that use the
    // counters (a plain hipMemset runs on the null stream, which non-blocking streams do not wait for)
    hipError_t me = hipMemsetAsync(p, 0, words * sizeof(uint32_t), lease.stream());
    if (me != hipSuccess) {
      (void)hipFree(p);
      return fail(DGPU_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(me));
    }
    s->counters = p;
  }
  *out = s->counters;
  *acc = s->counters + kCounterWordsArrive;
  if (spillFlags) *spillFlags = s->counters + kCounterWordsArrive + kCounterWordsAcc;
  return DGPU_OK;
}

// Cache policy of the histogram pass's input loads (format.h): non-temporal by default; ordinary (allocating) loads
// on request (dgpu_set_histogram_load_policy) for pipelines in which the codec's own dirty lines are what fills the
// memory-side cache when the pass starts.
std::atomic<int> g_histLoadPolicy{-1};  // -1: the compile-time default per input type, 0: non-temporal, 1: ordinary
bool histogramLoadsNonTemporal(uint32_t ft) {
  const int m = g_histLoadPolicy.load();
  (void)ft;
  return m < 0 ? kNtHistLoads : m == 0;
}

// Shared tail of every encode entry point: [checksum] -> histogram (+ fused
// normalisation) -> encode.  `in` holds raw bytes (floatType == 0: the ANS
// archive is the whole output) or float words (floatType != 0: the encoder
// splits them on the fly, the archive is a float archive).  `sourceType` is floatType, or floatType | kCastSource for
// a cast call: `in` then holds float32 words, which histogram and encoder round to floatType in registers.  Only the
// choice of the kernels depends on it -- grids, lists and temp memory are those of the plain call of floatType (no
// single-block kernels, though: such elements run on 2-block tiles).  No memset is needed
// on the common path: histogram workgroups store partial histograms, the last
// one of each element sums and normalises them and clears the tile descriptors +
// ticket for the encode kernel.
// (DGPU_TWO_LEVEL_LOOKBACK=0: the single level everywhere -- A/B runs and tests)
std::atomic<int> g_twoLevelLookback{envInt("DGPU_TWO_LEVEL_LOOKBACK", 1)};
// dgpu_float_rolling_compress: last call's counts instead of a histogram pass (smoothed, NormalizeArgs::smoothCounts;
// every element then has its own capacity, EncodeArgs::capAtMax) and / or this call's counts from the counting encoder.
struct RollingCounts {
  const uint32_t* countsIn = nullptr;
  uint32_t* countsOut = nullptr;
};
// dgpu_float_stochastic_compress: what the histogram and the encoder form a member's random bits from.  Kernel arguments,
// not part of the parameter block: calls that differ only in seed share the block and its cache entry.
struct StochasticSeed {
  uint64_t seed = 0;
  const uint64_t* seed_dev = nullptr;
  uint32_t firstMember = 0;
};
struct EncodeShared {
  uint32_t* checksumTemp = nullptr;  // [B] the batch's checksums (computed by the first class's call)
  uint4* table = nullptr;            // [B][256] encoder tables, indexed by the element's own index
  uint16_t* spill = nullptr;         // spill slots of the float encoders (every class's kernel is done with them when the next starts)
  size_t spillWords = 0;
};
int encodeCommon(
    TempArena& arena, StreamLease& lease, hipStream_t stream, int P, bool useChecksum, uint32_t B,
    const BatchView& in, const BatchView& archives, uint32_t sourceType,
    const LaunchGroup& group /* the whole batch, or one size class of it */, const uint32_t* work_dev /* the plan's lists on the device */,
    EncodeShared& shared /* what the groups of one call share */, const uint32_t* hist_dev /*may be null*/, uint32_t* outSize_dev,
    uint32_t outCapacity /* bytes at every archive pointer; block data beyond it is dropped */,
    uint32_t* histAcc_dev = nullptr /* the histogram in the stream's zero-at-rest counters instead of hist_dev (reduce-compress):
                                       the normalisation reads them and puts them back to zero */,
    const RollingCounts& rolling = RollingCounts{},
    const DeviceBatch* residual = nullptr /* feedback source: its resIn / resOut */,
    const StochasticSeed& sr = StochasticSeed{} /* stochastic source: handed to both launches */) {
  // (kCountingSource is the planner's: from here on the source is what the kernels are instantiated for)
  sourceType &= ~kCountingSource;
  // (rolling.countsIn arrives as hist_dev -- encodeBatch passes it as the call's histogram; here it only says that the
  // histogram is another call's: smoothed, and every element clipped at its own maximum)
  const bool counting = rolling.countsOut != nullptr, foreignTable = rolling.countsIn != nullptr;
  const uint32_t floatType = encArchiveType(sourceType);
  const uint32_t wordBytes = floatType ? floatWordBytes(floatType) : 1u;
  const uint32_t tileBlocks = group.tileBlocks, maxTiles = group.maxTiles, maxSize = group.maxSize;

  uint32_t* checksumTemp = shared.checksumTemp;
  if (useChecksum && !checksumTemp) {
    DGPU_ALLOC(ck, uint32_t, arena, B);
    checksumTemp = shared.checksumTemp = ck;
    DGPU_HIP(hipMemsetAsync(checksumTemp, 0, (size_t)B * 4, stream));
    // Float quirk kept from the reference (GpuFloatCompress.cuh:466-468): the
    // size in float WORDS is consumed as a BYTE count by the checksum.
    dim3 grid(gridX(maxSize, 64 * 1024, 64), B);
    DGPU_LAUNCH("k_checksum", stream, k_checksum, grid, dim3(256), 0, stream, in, (const uint32_t*)nullptr, (const uint8_t*)nullptr, checksumTemp);
    DGPU_HIP(hipGetLastError());
  }


  // Encoder tables [B][256] x 16 bytes, normalisation -> encoder.  Not for batches of single-block elements: there
  // the table would be as many bytes as the element's symbols, and k_ans_encode_pair derives it from the pdf table in
  // the archive header instead.
  uint4* table = shared.table;
  if (tileBlocks != kBlocksPerSingleTile && !table) {
    DGPU_ALLOC(tb, uint4, arena, (size_t)B * kNumSymbols);
    table = shared.table = tb;
  }
  // Work lists (descriptors and claim words for the tiles that exist only) of a listed group; an unlisted group's
  // fields are zero
  const bool lists = group.listed && tileBlocks != kBlocksPerSingleTile;
  const uint32_t numListedTiles = group.numTiles, numListedHistParts = group.numHistParts, listedHistPartBytes = group.histPartBytes;
  const uint32_t* tilesList = lists ? work_dev + group.tilesAt : nullptr;
  const uint32_t* histPartsList = lists ? work_dev + group.histAt : nullptr;
  const uint32_t* tileBaseList = lists ? work_dev + group.tileBaseAt : nullptr;
  // (the single-block class of a batch: the elements to pair up)
  const uint32_t* elemMap = (group.listed && !lists) ? work_dev + group.elemsAt : nullptr;
  const uint32_t numElems = elemMap ? group.numElems : B;
  DGPU_ALLOC(tileDesc, uint64_t, arena, lists ? std::max<size_t>(numListedTiles, 1u) : (size_t)B * std::max(maxTiles, 1u));
  DGPU_ALLOC(claims, uint32_t, arena, lists ? std::max<size_t>(numListedTiles, 1u) : (size_t)B * std::max(maxTiles, 1u));
  // second level of the look-back for elements of more than 64 tiles (kernels_encode.h, lookBackTwoLevel): rectangles only
  const uint32_t lookbackGroups = (floatType != 0 && !lists && tileBlocks != kBlocksPerSingleTile && maxTiles > kLookbackGroup && g_twoLevelLookback.load() != 0)
      ? divUp(maxTiles, kLookbackGroup) : 0u;
  uint64_t* groupWords = nullptr;
  if (lookbackGroups) {
    DGPU_ALLOC(gw, uint64_t, arena, (size_t)B * lookbackGroups * (kGroupArriveStride + 1u));
    groupWords = gw;
  }

  // The encoder's variant and grid.  8-block float tiles run as persistent workgroups, as many as fit on the chip at
  // once, that walk the tickets with a static map; raw bytes and float tiles of 2 / 4 blocks run one workgroup per tile
  // when there are more tiles than that, dispatched by the hardware in ticket order (encoderHardwareDispatch);
  // k_ans_encode_pair always runs one workgroup per pair.  `resident` = the workgroups of the kernel that fit on the
  // chip at once.  Spill slots (float inputs): [resident][slots per workgroup] -- a persistent workgroup's
  // own, or a pool handed out through spillFlags.
  const bool pairs = tileBlocks == kBlocksPerSingleTile;
  const uint32_t numTickets = lists ? numListedTiles : (elemMap ? numElems : B * maxTiles);
  const uint32_t numWorkgroups = pairs ? (numTickets + 1u) / 2u : numTickets;  // (one per pair of elements / per tile)
  const bool wideStage = maxTiles <= kWideStageMaxTiles;
  // (the counting form is persistent whatever dgpu_debug_set_encoder_dispatch says: it exists in that form only)
  const EncodeVariant persistent = counting ? encoderVariantCounting(P, sourceType, tileBlocks) : encoderVariant(P, sourceType, tileBlocks, false, wideStage);
  const EncodeVariant hardware = counting ? persistent : encoderVariant(P, sourceType, tileBlocks, true, wideStage);
  const bool bothForms = hardware.fn != persistent.fn;
  // The persistent grid is the persistent variant's own occupancy.  The spill pool must cover whichever form is
  // launched and the policy is decided before the form is: where both forms exist the larger occupancy counts there
  // (on gfx950 both allocate the same registers and LDS).
  const uint32_t residentPersistent = maxTiles > 0 ? residentWorkgroups(persistent, numWorkgroups) : 0u;
  const uint32_t resident =
      (bothForms && maxTiles > 0) ? std::max(residentPersistent, residentWorkgroups(hardware, numWorkgroups)) : residentPersistent;
  const bool hwDispatch = bothForms && encoderHardwareDispatch(numTickets, resident);
  const EncodeVariant& enc = hwDispatch ? hardware : persistent;
  uint16_t* spill = nullptr;
  uint32_t* spillFlags = nullptr;
  uint32_t spillPairs = 0;
  if (maxTiles > 0 && encodeSpills(floatType)) {
    // (single-block batches: two slots per workgroup, one per element of its pair)
    const uint32_t slotsPerWg = pairs ? 2u : tileBlocks;
    // (the size classes of one call run one after the other on the stream: they share the region of the first one
    // that is large enough)
    const size_t spillWords = (size_t)resident * slotsPerWg * encSpillSlotWords(P);
    if (shared.spill && shared.spillWords >= spillWords) {
      spill = shared.spill;
    } else {
      DGPU_ALLOC(sp, uint16_t, arena, spillWords);
      spill = shared.spill = sp;
      shared.spillWords = spillWords;
    }
    if (pairs || hwDispatch) {
      // one workgroup per pair / tile: the slots are a POOL with a pair for every wavefront that can be resident,
      // handed out through library-owned flags that are zero at rest
      uint32_t *arrive = nullptr, *acc = nullptr;
      int rc = arrivalCounters(lease, &arrive, &acc, &spillFlags);
      if (rc) return rc;
      spillPairs = resident * slotsPerWg / 2u;
      DGPU_REQUIRE(spillPairs <= kCounterWordsSpill, "more resident encoder wavefronts than spill-pool flags");
    }
  }

  NormalizeArgs n;
  n.sizes = in;
  n.hist = hist_dev;
  n.histAcc = nullptr;
  n.histParts = 1;
  n.probBits = P;
  n.encTable = table;
  n.refTable = nullptr;
  n.out = archives;
  n.writeHeader = 1;
  n.floatType = floatType;
  // ANS-level checksums are not used in float mode (GpuFloatCodec.h:50)
  n.useChecksum = (useChecksum && !floatType) ? 1 : 0;
  n.checksum = (useChecksum && !floatType) ? checksumTemp : nullptr;
  n.outSize = outSize_dev;
  n.floatUseChecksum = (useChecksum && floatType) ? 1 : 0;
  n.tileDesc = tileDesc;
  n.maxTiles = maxTiles;
  n.claims = claims;
  n.numInBatch = B;
  n.tileBase = tileBaseList;
  n.tileSymbols = tileBlocks * kBlockSize;
  n.groupWords = groupWords;
  n.groupWordsPerElement = lookbackGroups * (kGroupArriveStride + 1u);
  n.smoothCounts = foreignTable ? 1u : 0u;
  n.countsOut = rolling.countsOut;

  const bool haveHist = hist_dev || histAcc_dev;
  if (!haveHist && tileBlocks == kBlocksPerSingleTile && maxTiles > 0 && floatType != kFloat32) {
    // batches of single-block elements: one wavefront counts and normalises an element (kernels_pairs.h); no partial
    // histograms, no arrival counters.  (Measured on 32768 elements, profiles/r04_ab_single_block_elements.txt:
    // bf16 75.5 -> 65.5 us, fp16 80.5 -> 73.7; float32 -- 16 bytes of input per symbol and lane -- 69 -> 75.5, so
    // float32 keeps the workgroup per element.)
    int rc = launchVariant(statsSingleVariant(floatType, histogramLoadsNonTemporal(floatType)), dim3(divUp(numElems, kSingleStatWaves)), stream,
                           in, n, elemMap, numElems);
    if (rc) return rc;
  } else if (!haveHist) {
    const bool histList = lists && numListedHistParts != 0;
    const bool accumulate = !histList && histAccumulates(B, maxSize * wordBytes, floatType == 0);
    dim3 grid(accumulate ? histPartsAccFor(B, maxSize * wordBytes) : histPartsFor(B, maxSize * wordBytes, floatType == 0), B);
    if (histList) grid = dim3(numListedHistParts);  // one workgroup per listed (element, part)
    uint32_t* histTemp = nullptr;
    if (!accumulate) {
      DGPU_ALLOC(ht, uint32_t, arena, (size_t)(histList ? 1u : B) * grid.x * kNumSymbols);
      histTemp = ht;
    }
    HistFuse fuse;
    fuse.workMap = histList ? histPartsList : nullptr;
    fuse.partBytes = histList ? listedHistPartBytes : 0u;
    uint32_t* acc = nullptr;
    int rc = arrivalCounters(lease, &fuse.arrive, &acc);
    if (rc) return rc;
    fuse.acc = accumulate ? acc : nullptr;
    n.hist = histTemp;
    n.histAcc = fuse.acc;
    n.histParts = histList ? 1u : grid.x;
    fuse.norm = n;
    fuse.residual = residual ? residual->resIn : BatchView{};
    fuse.seed = sr.seed;
    fuse.seedPtr = sr.seed_dev;
    fuse.firstMember = sr.firstMember;
    // bins with 32 lane slots unless a workgroup sees too little data to pay for zeroing / folding them
    const bool smallBins = histList ? listedHistPartBytes <= 64u * 1024u : (uint64_t)maxSize * wordBytes / grid.x <= 64u * 1024u;
    rc = launchVariant(histogramVariant(sourceType, smallBins, histogramLoadsNonTemporal(floatType)), grid, stream, in, histTemp, 1u, fuse);
    if (rc) return rc;
  } else {
    // caller-supplied histogram (or the counts of reduce-compress): stand-alone normalisation
    n.histAcc = histAcc_dev;
    DGPU_LAUNCH("k_normalize", stream, k_normalize, dim3(B), dim3(256), 0, stream, n);
    DGPU_HIP(hipGetLastError());
  }
  if (maxTiles > 0) {
    const uint32_t grid = (pairs || hwDispatch) ? numWorkgroups : residentPersistent;
    EncodeArgs e;
    e.in = in;
    e.out = archives;
    e.encTable = table;
    e.maxTiles = maxTiles;
    e.numInBatch = B;
    e.numTickets = numTickets;
    e.workMap = lists ? tilesList : elemMap;
    e.tileDesc = tileDesc;
    e.claims = claims;
    e.groupWords = groupWords;
    e.groupsPerElement = lookbackGroups;
    e.absentModulo = absentWorkgroupModulo();
    {
      // tiles of ONE element that are in flight at once: the resident workgroups over the elements of this launch
      const uint32_t elems = lists ? std::max(1u, numTickets / std::max(maxTiles, 1u)) : std::max(numElems, 1u);
      e.pollLong = std::min(maxTiles, std::max(resident, 1u) / elems) > 12u ? 1u : 0u;
    }
    e.spill = spill;
    e.spillFlags = spillFlags;
    e.spillPairs = spillPairs;
    e.outSize = outSize_dev;
    e.outCapacity = outCapacity;
    e.useChecksum = (useChecksum && floatType) ? 1 : 0;
    e.checksum = (useChecksum && floatType) ? checksumTemp : nullptr;
    e.capAtMax = foreignTable ? 1u : 0u;
    e.countsOut = rolling.countsOut;
    e.resIn = residual ? residual->resIn : BatchView{};
    e.resOut = residual ? residual->resOut : BatchView{};
    e.seed = sr.seed;
    e.seedPtr = sr.seed_dev;
    e.firstMember = sr.firstMember;
    int rc = launchVariant(enc, dim3(grid), stream, e);
    if (rc) return rc;
  }
  return DGPU_OK;
}

// Shared tail of the encode entry points (ft: 0 for raw bytes): the batch as stride views or uploaded pointers, with
// the work lists of its plan (work_plan.h), then encodeCommon once per launch group.
int encodeBatch(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t ft, int P, int useChecksum, Batch& b,
    const uint32_t* histogram_dev /*may be null*/, uint32_t* outSize_dev, hipStream_t stream,
    uint32_t outCapacity = 0xffffffffu /* as encodeCommon's */, const RollingCounts& rolling = RollingCounts{},
    const StochasticSeed& sr = StochasticSeed{}) {
  // a counting call is planned without single-block kernels, one with last call's counts as one with a caller's histogram
  if (rolling.countsOut) ft |= kCountingSource;
  if (rolling.countsIn) histogram_dev = rolling.countsIn;
  StreamLease streamLease(stream);
  TempArena arena(temp_dev, tempBytes, streamLease);
  DeviceBatch d;
  // (a feedback call, and a stochastic one, is planned as the cast call it extends: same geometry, same lists, same
  // cached plan)
  const uint32_t planType = ft & ~(kFeedbackSource | kStochasticSource);
  std::vector<LaunchGroup> groups{encodeRectangle(b.maxSize, planType)};
  int rc = resolveBatch(b, false, streamLease, &d, [&] { planEncodeCall(planPolicy(), b.sizes, planType, b.maxSize, histogram_dev != nullptr, &groups, &b.work); });
  if (rc) return rc;
  // (float inputs: no exponent plane in temp memory, the encoder splits the float words itself)
  // every group on the kernels of its own geometry, one after the other
  EncodeShared shared;
  for (const LaunchGroup& g : groups) {
    rc = encodeCommon(arena, streamLease, stream, P, useChecksum != 0, b.n, d.in, d.out, ft, g, d.work, shared, histogram_dev, outSize_dev, outCapacity, nullptr, rolling,
                      encIsFeedback(ft) ? &d : nullptr, sr);
    if (rc) break;
  }
  if (tempUsed) *tempUsed = arena.requested();
  return rc;
}

int ansEncodeImpl(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int P, int useChecksum, Batch& b, const uint32_t* histogram_dev,
    uint32_t* outSize_dev, hipStream_t stream) {
  bool done;
  int rc = checkCall(P, b.n, 0u, tempUsed, /*errBatch*/ nullptr, &done,
                     "input larger than 1717538816 bytes: its maximum compressed size exceeds INT32_MAX (GpuANSEncode.cu:22)", b.maxSize);
  if (done) return rc;
  return encodeBatch(temp_dev, tempBytes, tempUsed, 0u, P, useChecksum, b, histogram_dev, outSize_dev, stream);
}

// (cast: the batch holds float32 words and ft is the archive's 16-bit type; feedback: a cast call whose batch carries
// residual pointers; stochastic: a cast call that rounds with the random bits of *stochastic)
int floatCompressImpl(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t ft, int P, int useChecksum, Batch& b, uint32_t* outSize_dev,
    hipStream_t stream, bool cast = false, const RollingCounts& rolling = RollingCounts{}, bool feedback = false,
    const StochasticSeed* stochastic = nullptr) {
  bool done;
  int rc = checkCall(P, b.n, ft, tempUsed, /*errBatch*/ nullptr, &done,
                     "tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX (GpuANSEncode.cu:22)",
                     b.maxSize);
  if (done) return rc;
  const uint32_t source = stochastic ? (ft | kCastSource | kStochasticSource)
                                     : (feedback ? (ft | kCastSource | kFeedbackSource) : (cast ? (ft | kCastSource) : ft));
  return encodeBatch(temp_dev, tempBytes, tempUsed, source, P, useChecksum, b, nullptr, outSize_dev, stream, 0xffffffffu, rolling,
                     stochastic ? *stochastic : StochasticSeed{});
}

// Order of k_ans_decode's workgroups (kernels_decode.h: decodeTileOf).  Measured on MI355X, cold round trip
// (profiles/r05_ab_decoder_order.txt): with the tiles of an element back to back, eight consecutive workgroups -- one per
// XCD -- read one archive and write one output row; letting every XCD walk its own elements spreads a moment's traffic
// over eight times as many rows: 256 x 512 Ki bf16 decode 107 -> 102 us (step -1.7 %), fp16 -3.5 %, 64 x 2 Mi -4 %,
// Zipf bytes -1 %.  It needs enough elements to keep the eight XCDs level (16 x 8 Mi: +17 % for the decoder alone, a
// batch of one: everything on one XCD), so small batches keep the element-major order.  -1 = this policy;
// dgpu_debug_set_decoder_order / DGPU_DEC_ORDER force an order (tests, A/B runs).
std::atomic<int> g_decOrder{envInt("DGPU_DEC_ORDER", -1)};
uint32_t decodeOrder(uint32_t B) {
  const int forced = g_decOrder.load();
  if (forced >= 0 && forced <= (int)kDecOrderXcd) return (uint32_t)forced;
  return B >= 64u ? kDecOrderXcd : kDecOrderElementMajor;
}

// What every launch of a decode call has in common.
DecodeArgs decodeArgs(const Batch& b, const DeviceBatch& d, uint32_t ft, uint8_t* outSuccess_dev, uint32_t* outSize_dev) {
  DecodeArgs a;
  a.in = d.in;
  a.out = d.out;
  a.floatType = ft;
  a.outSuccess = outSuccess_dev;
  a.outSize = outSize_dev;
  a.inBytes = d.inBytes;
  a.uniformInBytes = b.uniformInBytes;
  a.numInBatch = b.n;
  return a;
}

// One launch group of a decode call, in any form: the rectangle in the order of decodeOrder (padded to whole rounds of
// the eight XCDs where they walk their own elements), or the group's list; single-block elements (k_ans_decode_pair,
// every capacity <= 4096 symbols) run one workgroup per pair of elements.
int launchDecode(DecodeArgs d, const LaunchGroup& g, const uint32_t* work_dev, DecodeForm form, int P, hipStream_t stream) {
  const bool pairs = g.tileBlocks == kDecBlocksPerSingleTile;
  const uint32_t B = d.numInBatch;
  d.maxTiles = g.maxTiles;
  d.order = g.listed ? kDecOrderMap : decodeOrder(B);
  d.workMap = g.listed ? work_dev + (pairs ? g.elemsAt : g.tilesAt) : nullptr;
  d.numListed = g.numElems;
  const uint32_t tiles = g.listed ? std::max(g.numTiles, 1u) : (d.order == kDecOrderXcd ? roundUp(B, 8u) : B) * g.maxTiles;
  const uint32_t grid = pairs ? ((g.listed ? g.numElems : B) + 1u) / 2u : tiles;
  return launchVariant(decoderVariant(P, d.floatType, g.tileBlocks, form), dim3(grid), stream, d);
}

int decodeImpl(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t ft, int P, int useChecksum, Batch& b, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, hipStream_t stream, int32_t* errBatch) {
  g_mismatches.clear();
  bool done;
  int rc = checkCall(P, b.n, ft, tempUsed, errBatch, &done);
  if (done) return rc;
  const uint32_t B = b.n, maxCapacity = b.maxSize;
  StreamLease streamLease(stream);
  if (useChecksum && streamLease.capturing()) {
    // the comparison is host work behind a stream synchronise (as upstream, GpuANSDecode.cuh:557-591): it would
    // invalidate the capture, and a replay could never repeat it
    return fail(DGPU_ERR_HIP, "HIP graph capture: checksum verification on decode copies to the host and synchronises the "
                              "stream; it cannot be captured into a HIP graph (decode with useChecksum = 0 under capture)");
  }

  TempArena arena(temp_dev, tempBytes, streamLease);
  DeviceBatch dev;
  std::vector<LaunchGroup> groups{decodeRectangle(divUp(maxCapacity, kBlockSize), true)};
  rc = resolveBatch(b, true, streamLease, &dev, [&] { planDecodeCall(planPolicy(), b.sizes, maxCapacity, true, &groups, &b.work); });
  if (rc) return rc;

  uint32_t* sizesForChecksum = outSize_dev;
  uint8_t* successForChecksum = outSuccess_dev;
  if (useChecksum) {
    if (!sizesForChecksum) {
      DGPU_ALLOC(s, uint32_t, arena, B);
      sizesForChecksum = s;
    }
    if (!successForChecksum) {
      DGPU_ALLOC(s, uint8_t, arena, B);
      successForChecksum = s;
    }
  }

  const DecodeArgs d = decodeArgs(b, dev, ft, successForChecksum, sizesForChecksum);
  // every group on the decoder of its own geometry, one after the other
  for (const LaunchGroup& g : groups) {
    rc = launchDecode(d, g, dev.work, DecodeForm::kWhole, P, stream);
    if (rc) return rc;
  }

  int status = DGPU_OK;
  if (useChecksum) {
    // checksum the decoded data, fetch the archived checksum, compare on the
    // host (GpuANSDecode.cuh:557-591, GpuFloatDecompress.cuh:699-733).  The
    // decoded size (bytes, or -- float quirk -- float words used as a byte
    // count) bounds the checksummed range.
    DGPU_ALLOC(sums, uint32_t, arena, 2 * (size_t)B);
    DGPU_HIP(hipMemsetAsync(sums, 0, 2 * (size_t)B * 4, stream));
    dim3 grid(gridX(maxCapacity * (ft ? floatWordBytes(ft) : 1u), 64 * 1024, 64), B);
    hipLaunchKernelGGL(k_checksum, grid, dim3(256), 0, stream, dev.out, (const uint32_t*)sizesForChecksum,
                       (const uint8_t*)successForChecksum, sums);
    DGPU_HIP(hipGetLastError());
    if (ft) {
      hipLaunchKernelGGL(k_float_info, dim3(divUp(B, 128)), dim3(128), 0, stream, dev.in, B,
                         (uint32_t*)nullptr, (uint32_t*)nullptr, sums + B);
    } else {
      hipLaunchKernelGGL(k_ans_info, dim3(divUp(B, 128)), dim3(128), 0, stream, dev.in, B,
                         (uint32_t*)nullptr, sums + B);
    }
    DGPU_HIP(hipGetLastError());
    std::vector<uint32_t> h(2 * (size_t)B);
    std::vector<uint8_t> ok(B);
    DGPU_HIP(hipMemcpyAsync(h.data(), sums, h.size() * 4, hipMemcpyDeviceToHost, stream));
    DGPU_HIP(hipMemcpyAsync(ok.data(), successForChecksum, B, hipMemcpyDeviceToHost, stream));
    DGPU_HIP(hipStreamSynchronize(stream));
    // EVERY mismatching member is reported, as upstream pushes every one into errorInfo; the message is the
    // reference's, one line per member (its stringstream is never reset, so the text accumulates)
    std::string msg;
    for (uint32_t i = 0; i < B; ++i) {
      if (ok[i] && h[i] != h[B + i]) {
        char buf[160];
        snprintf(buf, sizeof(buf),
                 "Checksum mismatch in batch member %u: expected checksum %x got %x\n", i,
                 h[B + i], h[i]);
        msg += buf;
        g_mismatches.push_back({(int32_t)i, h[B + i], h[i]});
        if (status == DGPU_OK && errBatch) *errBatch = (int32_t)i;
        status = DGPU_ERR_CHECKSUM_MISMATCH;
      }
    }
    if (status != DGPU_OK) g_lastError = msg;
  }
  if (tempUsed) *tempUsed = arena.requested();
  return status;
}

// Ranged decode (k_ans_decode_range): blocks [firstBlock[i], firstBlock[i] + numBlocks[i]) of every element, into a
// buffer that holds the range.  The work list (planRangeCall) holds the tiles the request and the capacity allow; the
// element may turn out to end earlier -- those workgroups leave after the header, as the tiles beyond a short element do
// in a whole decode.  No temp memory, no host synchronisation.
int decodeRangeImpl(
    size_t* tempUsed, uint32_t ft, int P, uint32_t B, const void* const* in, const uint32_t* inBytes,
    const uint32_t* firstBlock, const uint32_t* numBlocks, void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  // (the arrays are read after the checks that do not need them: numInBatch itself may be what is wrong)
  bool done;
  int rc = checkCall(P, B, ft, tempUsed, /*errBatch*/ nullptr, &done);
  if (done) return rc;
  DGPU_REQUIRE(in && inBytes && firstBlock && numBlocks && out && outCapacity, "ranged decode: null array with numInBatch > 0");
  Batch b;
  rc = pointerBatch(&b, B, ptrSide(in, 16, kMsgCompIn), ptrSide(out), outCapacity, inBytes);
  if (rc) return rc;
  // (the tiles are planned in symbols, 32 bits: the blocks of a capacity must not round up to 2^32 of them)
  DGPU_REQUIRE(b.maxSize <= 0xfffff000u, "ranged decode: outCapacity must not exceed 0xfffff000");
  LaunchGroup group;
  if (!planRangeCall(B, firstBlock, numBlocks, outCapacity, &group, &b.work)) {
    return fail(DGPU_ERR_INVALID_ARGUMENT, "ranged decode: the ranges have too many tiles for one call");
  }

  StreamLease streamLease(stream);
  DeviceBatch dev;
  rc = resolveBatch(b, true, streamLease, &dev);
  if (rc) return rc;
  DecodeArgs d = decodeArgs(b, dev, ft, outSuccess_dev, outSize_dev);
  d.firstBlock = dev.work;
  d.numBlocks = dev.work + B;
  return launchDecode(d, group, dev.work, DecodeForm::kRanged, P, stream);
}

// The sources of a mixed call (dgpu_float_decode_reduce_mixed, dgpu_float_reduce_compress_mixed): kinds[k] == 0, an
// archive, 16-byte aligned like every compressed input; 1, a raw row of inBytes[k] / wordBytes words of the float type,
// word-aligned like a compress input.  A raw row's address enters the parameter block with kReduceRawTag set, which is
// how the kernel tells the two apart (kernels_decode.h) and why a call that differs from a warm one in its kinds alone
// hashes to another block.  *anyRaw: false = the batch, and its block, are those of the plain call.
int mixedSourceAddresses(const void* const* in, const uint32_t* inBytes, const uint8_t* kinds, uint32_t n, uint32_t wordBytes,
                         std::vector<uint64_t>* addr, bool* anyRaw) {
  addr->resize(n);
  for (uint32_t k = 0; k < n; ++k) {
    const uint64_t at = (uint64_t)(uintptr_t)in[k];
    DGPU_REQUIRE(kinds[k] <= 1u, "sourceKind must be 0 (archive) or 1 (raw row)");
    if (kinds[k] == 0u) {
      DGPU_REQUIRE(at % 16u == 0u, kMsgCompIn);
      (*addr)[k] = at;
    } else {
      DGPU_REQUIRE(at % wordBytes == 0u, "raw source must be float-word aligned");
      DGPU_REQUIRE(inBytes[k] % wordBytes == 0u, "inBytes of a raw source must be a multiple of the float word size");
      (*addr)[k] = at | kReduceRawTag;
      *anyRaw = true;
    }
  }
  return DGPU_OK;
}

// The batch of a float pointer-decode call with S sources per output: B * S inputs and inBytes (member-major) beside B
// outputs and capacities -- pointerBatch for S == 1.  kinds: null, every input is an archive; else mixedSourceAddresses.
// The parameter block holds every input, so its hash -- the parameter-cache key -- covers each source pointer and size,
// and S through the block's length and layout.  tooLarge: the refusal of a capacity whose blocks would round up to 2^32
// symbols (the tiles are planned in symbols, 32 bits); null: the caller has a tighter bound of its own.
int floatDecodeBatch(Batch* b, uint32_t ft, uint32_t B, uint32_t S, const void* const* in, const uint32_t* inBytes, const uint8_t* kinds,
                     const Side& out, const uint32_t* outCapacity, const char* tooLarge, bool* anyRaw = nullptr) {
  int rc = kinds ? mixedSourceAddresses(in, inBytes, kinds, B * S, floatWordBytes(ft), &b->inPtrs, anyRaw)
                 : sideAddresses(ptrSide(in, 16, kMsgCompIn), B * S, &b->inPtrs);
  if (!rc) rc = sideAddresses(out, B, &b->outPtrs);
  if (rc) return rc;
  b->n = B;
  b->sizes.assign(outCapacity, outCapacity + B);
  b->inBytes.assign(inBytes, inBytes + (size_t)B * S);
  for (uint32_t i = 0; i < B; ++i) b->maxSize = std::max(b->maxSize, outCapacity[i]);
  DGPU_REQUIRE(!tooLarge || b->maxSize <= 0xfffff000u, tooLarge);
  return DGPU_OK;
}

// The one launch group of such a call -- the rectangle of a whole decode on 16- or 4-block tiles, or the tile list when
// the capacities differ widely -- and the batch resolved with it.
int planFloatDecode(Batch& b, StreamLease& streamLease, DeviceBatch* dev, LaunchGroup* group) {
  std::vector<LaunchGroup> groups{decodeRectangle(divUp(b.maxSize, kBlockSize), false)};
  const int rc = resolveBatch(b, true, streamLease, dev, [&] { planDecodeCall(planPolicy(), b.sizes, b.maxSize, false, &groups, &b.work); });
  *group = groups[0];
  return rc;
}

// The factor of a scaled decode-accumulate: the host float, or device memory the kernel reads (dev, stride 0 / 1).
struct DecodeFactor {
  float scale;
  const float* dev;
  uint32_t stride;
};

// Decode-accumulate (k_ans_decode_accum): every archive widened to float32 and stored to (accumulate == 0) or added into
// (1) its float32 accumulator.  factor (k_ans_decode_accum_scaled): the widened word is multiplied by it first.  No temp
// memory, no host synchronisation.
int decodeAccumulateImpl(
    size_t* tempUsed, uint32_t ft, int P, int accumulate, uint32_t B, const void* const* in, const uint32_t* inBytes,
    void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream,
    const DecodeFactor* factor = nullptr) {
  DGPU_REQUIRE(validFloatType(ft), kMsgFloatType);
  DGPU_REQUIRE(accumulate == 0 || accumulate == 1, "decode-accumulate: accumulate must be 0 or 1");
  if (factor) {
    DGPU_REQUIRE(factor->stride <= 1u, "scaled decode-accumulate: scaleStride must be 0 (one factor) or 1 (one per member)");
    DGPU_REQUIRE(factor->dev != nullptr || (std::isfinite(factor->scale) && factor->scale != 0.0f),
                 "scaled decode-accumulate: a host scale must be finite and not zero");
    DGPU_REQUIRE((uintptr_t)factor->dev % 4u == 0u, "scaled decode-accumulate: scale_dev must be 4-byte aligned");
    // a host factor of exactly 1 is the plain call (a multiply by 1 would quiet a signalling NaN)
    if (!factor->dev && factor->scale == 1.0f) factor = nullptr;
  }
  bool done;
  int rc = checkCall(P, B, ft, tempUsed, /*errBatch*/ nullptr, &done);
  if (done) return rc;
  DGPU_REQUIRE(in && inBytes && out && outCapacity, "decode-accumulate: null array with numInBatch > 0");
  Batch b;
  rc = floatDecodeBatch(&b, ft, B, 1, in, inBytes, nullptr, ptrSide(out, 4, "decode-accumulate: accumulators must be 4-byte aligned"), outCapacity,
                        "decode-accumulate: outCapacity must not exceed 0xfffff000");
  if (rc) return rc;
  StreamLease streamLease(stream);
  DeviceBatch dev;
  LaunchGroup group;
  rc = planFloatDecode(b, streamLease, &dev, &group);
  if (rc) return rc;
  DecodeArgs d = decodeArgs(b, dev, ft, outSuccess_dev, outSize_dev);
  d.accumulate = (uint32_t)accumulate;
  if (!factor) return launchDecode(d, group, dev.work, DecodeForm::kAccum, P, stream);
  d.scale = factor->scale;
  d.scalePtr = factor->dev;
  d.scaleStride = factor->stride;
  return launchDecode(d, group, dev.work, DecodeForm::kAccumScaled, P, stream);
}

// Scaled decompress (k_ans_decode_scaled): the whole bounded float decode whose every word is multiplied by the member's
// float32 factor and rounded back to the archive's type before it is stored.  scale_dev: device memory, read by the
// kernel -- never here -- so the factor may be written by work enqueued before the call, and a captured call follows
// the value the memory holds at each replay; null: the host float.  No temp memory, no host synchronisation.
int decodeScaledImpl(
    size_t* tempUsed, uint32_t ft, int P, uint32_t B, const void* const* in, const uint32_t* inBytes, void* const* out,
    const uint32_t* outCapacity, float scale, const float* scale_dev, uint32_t scaleStride, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, hipStream_t stream) {
  DGPU_REQUIRE(validFloatType(ft), kMsgFloatType);
  DGPU_REQUIRE(scaleStride <= 1u, "scaled decompress: scaleStride must be 0 (one factor) or 1 (one per member)");
  DGPU_REQUIRE(scale_dev != nullptr || (std::isfinite(scale) && scale != 0.0f), "scaled decompress: a host scale must be finite and not zero");
  DGPU_REQUIRE((uintptr_t)scale_dev % 4u == 0u, "scaled decompress: scale_dev must be 4-byte aligned");
  bool done;
  int rc = checkCall(P, B, ft, tempUsed, /*errBatch*/ nullptr, &done);
  if (done) return rc;
  DGPU_REQUIRE(in && inBytes && out && outCapacity, "scaled decompress: null array with numInBatch > 0");
  Batch b;
  rc = floatDecodeBatch(&b, ft, B, 1, in, inBytes, nullptr, ptrSide(out), outCapacity, "scaled decompress: outCapacity must not exceed 0xfffff000");
  if (rc) return rc;
  StreamLease streamLease(stream);
  DeviceBatch dev;
  LaunchGroup group;
  rc = planFloatDecode(b, streamLease, &dev, &group);
  if (rc) return rc;
  DecodeArgs d = decodeArgs(b, dev, ft, outSuccess_dev, outSize_dev);
  d.scale = scale;
  d.scalePtr = scale_dev;
  d.scaleStride = scaleStride;
  return launchDecode(d, group, dev.work, DecodeForm::kWholeScaled, P, stream);
}

// Decode-update (k_ans_decode_update): every 16-bit archive multiplied by the member's float32 factor, added to
// (accumulate == 1) or stored over (0) its 16-bit tensor of the same type, and rounded stochastically.  scale_dev and
// seed_dev: device memory, read by the kernel -- never here -- so a captured call follows what they hold at each replay;
// null: the host values.  No temp memory, no host synchronisation.
int decodeUpdateImpl(
    uint32_t ft, int P, int accumulate, uint32_t B, const void* const* in, const uint32_t* inBytes, void* const* out,
    const uint32_t* outCapacity, float scale, const float* scale_dev, uint32_t scaleStride, uint64_t seed,
    const uint64_t* seed_dev, uint32_t firstMember, uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream) {
  DGPU_REQUIRE(ft == DGPU_FLOAT16 || ft == DGPU_BFLOAT16, "decode-update: floatType must be DGPU_FLOAT16 or DGPU_BFLOAT16");
  DGPU_REQUIRE(accumulate == 0 || accumulate == 1, "decode-update: accumulate must be 0 or 1");
  DGPU_REQUIRE(scaleStride <= 1u, "decode-update: scaleStride must be 0 (one factor) or 1 (one per member)");
  DGPU_REQUIRE(scale_dev != nullptr || (std::isfinite(scale) && scale != 0.0f), "decode-update: a host scale must be finite and not zero");
  DGPU_REQUIRE((uintptr_t)scale_dev % 4u == 0u, "decode-update: scale_dev must be 4-byte aligned");
  DGPU_REQUIRE((uintptr_t)seed_dev % 8u == 0u, "decode-update: seed_dev must be 8-byte aligned");
  bool done;
  int rc = checkCall(P, B, ft, /*tempUsed*/ nullptr, /*errBatch*/ nullptr, &done);
  if (done) return rc;
  DGPU_REQUIRE(in && inBytes && out && outCapacity, "decode-update: null array with numInBatch > 0");
  Batch b;
  rc = floatDecodeBatch(&b, ft, B, 1, in, inBytes, nullptr, ptrSide(out, 2, "decode-update: tensors must be 2-byte aligned"), outCapacity,
                        "decode-update: outCapacity must not exceed 0xfffff000");
  if (rc) return rc;
  StreamLease streamLease(stream);
  DeviceBatch dev;
  LaunchGroup group;
  rc = planFloatDecode(b, streamLease, &dev, &group);
  if (rc) return rc;
  DecodeArgs d = decodeArgs(b, dev, ft, outSuccess_dev, outSize_dev);
  d.accumulate = (uint32_t)accumulate;
  d.scale = scale;
  d.scalePtr = scale_dev;
  d.scaleStride = scaleStride;
  d.seed = seed;
  d.seedPtr = seed_dev;
  d.firstMember = firstMember;
  return launchDecode(d, group, dev.work, DecodeForm::kUpdate, P, stream);
}

// The norm outputs of a reduce call (either given: the call measures what it leaves) and the temp region their tile
// partials are carved from.
struct ReduceNorm {
  double* outSumSq = nullptr;      // [B] device, nullable
  uint32_t* outNonFinite = nullptr;  // [B] device, nullable
  void* temp = nullptr;
  size_t tempBytes = 0;
  bool wanted() const { return outSumSq != nullptr || outNonFinite != nullptr; }
};
// (before anything is enqueued; an output that is not given passes)
int reduceNormCheck(const ReduceNorm& norm) {
  DGPU_REQUIRE((uintptr_t)norm.outSumSq % 8u == 0u, "outSumSq_dev must be 8-byte aligned");
  DGPU_REQUIRE((uintptr_t)norm.outNonFinite % 4u == 0u, "outNonFinite_dev must be 4-byte aligned");
  return DGPU_OK;
}
// The (member, tile) partials of the launch group: carved from the arena, zero when the reduce kernel starts.
int reduceNormBegin(TempArena& arena, uint32_t B, const LaunchGroup& g, DecodeArgs* d, hipStream_t stream) {
  const size_t bytes = reduceNormPartialBytes(B, std::max(g.maxTiles, 1u));
  DGPU_ALLOC(partials, uint8_t, arena, bytes);
  DGPU_HIP(hipMemsetAsync(partials, 0, bytes, stream));
  d->normPartials = (double*)partials;
  return DGPU_OK;
}
int reduceNormFinish(const ReduceNorm& norm, uint32_t B, const LaunchGroup& g, const DecodeArgs& d, hipStream_t stream) {
  ReduceNormFinishArgs f;
  f.partials = d.normPartials;
  f.numInBatch = B;
  f.maxTiles = std::max(g.maxTiles, 1u);
  f.outSumSq = norm.outSumSq;
  f.outNonFinite = norm.outNonFinite;
  DGPU_LAUNCH("k_reduce_norm_finish", stream, k_reduce_norm_finish, dim3(divUp(B, kNormFinishThreads / 64u)), dim3(kNormFinishThreads), 0, stream, f);
  DGPU_HIP(hipGetLastError());
  return DGPU_OK;
}

// What each of the eight reduce entry points adds to the plain call.
struct ReduceOptions {
  bool mixed = false;              // `kinds` says which sources are raw rows (mixedSourceAddresses) and must be given
  const uint8_t* kinds = nullptr;  // [B * S] host; null: every source is an archive
  float scale = 1.0f;              // a kernel argument: the parameter block and its cache entry are the unscaled call's
  ReduceNorm norm;
};

// The reduce kernel of a call, stated once.  stats: reduce-compress, which counts the exponent bytes of the rounded
// sums.  A norm form serves every scale and every kind of source, a scaled form every kind of source, for S == 1 too;
// with no raw row among the sources the call is the plain one.
DecodeForm reduceForm(bool stats, bool anyRaw, bool scaled, bool norm) {
  if (norm) return stats ? DecodeForm::kReduceNormStats : DecodeForm::kReduceNorm;
  if (scaled) return stats ? DecodeForm::kReduceScaledStats : DecodeForm::kReduceScaled;
  if (anyRaw) return stats ? DecodeForm::kReduceMixedStats : DecodeForm::kReduceMixed;
  return stats ? DecodeForm::kReduceStats : DecodeForm::kReduce;
}

// Decode-reduce: S = numSources archives per float32 accumulator, summed left to right in one launch, all or nothing per
// member.  The launch plan is that of a decode-accumulate call with the same capacities, and a call of one archive per
// member with no factor and no norm IS that call.  No host synchronisation; with the norm outputs the launch is followed
// by k_reduce_norm_finish (reduceNormBegin / reduceNormFinish), and the tile partials are the call's only temp memory.
int decodeReduceImpl(
    size_t* tempUsed, uint32_t ft, int P, int accumulate, uint32_t B, uint32_t S, const void* const* in, const uint32_t* inBytes,
    void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, hipStream_t stream, const ReduceOptions& opt) {
  DGPU_REQUIRE(validFloatType(ft), kMsgFloatType);
  const bool withNorm = opt.norm.wanted();
  const bool plainKernel = opt.scale == 1.0f && !withNorm;  // (a factor or a norm never goes the ways of the plain call)
  if (int rcNorm = reduceNormCheck(opt.norm)) return rcNorm;
  DGPU_REQUIRE(accumulate == 0 || accumulate == 1, "decode-reduce: accumulate must be 0 or 1");
  DGPU_REQUIRE(S >= 1u && S <= kMaxReduceSources, "decode-reduce: numSources must be between 1 and 64");
  DGPU_REQUIRE((uint64_t)B * S <= 65535u, "decode-reduce: numInBatch * numSources must be <= 65535");
  auto asAccumulate = [&] { return decodeAccumulateImpl(tempUsed, ft, P, accumulate, B, in, inBytes, out, outCapacity, outSuccess_dev, outSize_dev, stream); };
  if (S == 1u && !opt.mixed && plainKernel) return asAccumulate();
  bool done;
  int rc = checkCall(P, B, ft, tempUsed, /*errBatch*/ nullptr, &done);
  if (done) return rc;
  DGPU_REQUIRE(in && inBytes && out && outCapacity, "decode-reduce: null array with numInBatch > 0");
  DGPU_REQUIRE(!opt.mixed || opt.kinds, "decode-reduce: sourceKind is null with numInBatch > 0");
  if (S == 1u && plainKernel && opt.kinds && std::all_of(opt.kinds, opt.kinds + B, [](uint8_t k) { return k == 0u; })) return asAccumulate();
  Batch b;
  bool anyRaw = false;
  rc = floatDecodeBatch(&b, ft, B, S, in, inBytes, opt.kinds, ptrSide(out, 4, "decode-reduce: accumulators must be 4-byte aligned"), outCapacity,
                        "decode-reduce: outCapacity must not exceed 0xfffff000", &anyRaw);
  if (rc) return rc;
  StreamLease streamLease(stream);
  DeviceBatch dev;
  LaunchGroup group;
  rc = planFloatDecode(b, streamLease, &dev, &group);
  if (rc) return rc;
  DecodeArgs d = decodeArgs(b, dev, ft, outSuccess_dev, outSize_dev);
  d.accumulate = (uint32_t)accumulate;
  d.numSources = S;
  d.scale = opt.scale;
  const DecodeForm form = reduceForm(false, anyRaw, !plainKernel, withNorm);
  if (!withNorm) return launchDecode(d, group, dev.work, form, P, stream);
  TempArena arena(opt.norm.temp, opt.norm.tempBytes, streamLease);
  rc = reduceNormBegin(arena, B, group, &d, stream);
  if (!rc) rc = launchDecode(d, group, dev.work, form, P, stream);
  if (!rc) rc = reduceNormFinish(opt.norm, B, group, d, stream);
  if (tempUsed) *tempUsed = arena.requested();
  return rc;
}

// Reduce-compress: decode-reduce into the accumulators, then cast-compress of the accumulators, without the cast
// histogram pass -- the reduce kernel (k_ans_decode_reduce_stats) counts the exponent bytes of the rounded sums as it
// stores them, and the cast encoder runs on the table normalised from those counts (encodeCommon with a histogram).
// The counts [B][256] are zero when the reduce kernel starts: for B <= kAccElements they are the stream's zero-at-rest
// histogram counters (held under the stream lease; k_normalize reads them and puts them back to zero), otherwise a
// region of temp memory cleared by one memset on the stream.  A member that fails the reduce has no counts: its table is
// the flat one, which codes any data.  Everything is validated before the first enqueue; nothing synchronises.
// The reduce kernels are the counting forms of decodeReduceImpl's (reduceForm): with a scale they store, round and count
// the scaled sums -- the encoder does not know -- and with the norm outputs they measure the sums ROUNDED to the archive
// type; the partials come out of the call's temp memory like the counts.
int reduceCompressImpl(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t ft, int P, int accumulate, uint32_t B, uint32_t S,
    const void* const* in, const uint32_t* inBytes, void* const* acc, const uint32_t* outCapacity, void* const* outArchive,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, hipStream_t stream, const ReduceOptions& opt) {
  DGPU_REQUIRE(ft == kFloat16 || ft == kBFloat16, "reduce-compress: floatType must be float16 or bfloat16 (float32: decode-reduce, then dgpu_float_compress)");
  const bool withNorm = opt.norm.wanted();
  if (int rcNorm = reduceNormCheck(opt.norm)) return rcNorm;
  DGPU_REQUIRE(accumulate == 0 || accumulate == 1, "reduce-compress: accumulate must be 0 or 1");
  DGPU_REQUIRE(S >= 1u && S <= kMaxReduceSources, "reduce-compress: numSources must be between 1 and 64");
  DGPU_REQUIRE((uint64_t)B * S <= 65535u, "reduce-compress: numInBatch * numSources must be <= 65535");
  bool done;
  int rc = checkCall(P, B, ft, tempUsed, /*errBatch*/ nullptr, &done);
  if (done) return rc;
  DGPU_REQUIRE(in && inBytes && acc && outCapacity && outArchive, "reduce-compress: null array with numInBatch > 0");
  DGPU_REQUIRE(!opt.mixed || opt.kinds, "reduce-compress: sourceKind is null with numInBatch > 0");
  // the reduce side: B * S archives into B accumulators (decodeReduceImpl); the compress side: the accumulators into B archives
  Batch bd, be;
  bool anyRaw = false;
  const Side accSide = ptrSide(acc, 4, "reduce-compress: accumulators must be 4-byte aligned");
  rc = floatDecodeBatch(&bd, ft, B, S, in, inBytes, opt.kinds, accSide, outCapacity, /*tooLarge: encodableSize*/ nullptr, &anyRaw);
  if (!rc) rc = pointerBatch(&be, B, accSide, ptrSide(outArchive, 16, kMsgCompOut), outCapacity);
  if (rc) return rc;
  DGPU_REQUIRE(encodableSize(be.maxSize),
               "reduce-compress: outCapacity larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX (GpuANSEncode.cu:22)");

  StreamLease streamLease(stream);
  TempArena arena(temp_dev, tempBytes, streamLease);
  DeviceBatch devD, devE;
  LaunchGroup groupD;
  rc = planFloatDecode(bd, streamLease, &devD, &groupD);
  if (rc) return rc;
  const uint32_t castType = ft | kCastSource;
  std::vector<LaunchGroup> groupsE{encodeRectangle(be.maxSize, castType)};
  rc = resolveBatch(be, false, streamLease, &devE, [&] { planEncodeCall(planPolicy(), be.sizes, castType, be.maxSize, true, &groupsE, &be.work); });
  if (rc) return rc;

  uint32_t *counts = nullptr, *countsAtRest = nullptr;
  if (B <= kAccElements) {
    uint32_t* arrive = nullptr;
    rc = arrivalCounters(streamLease, &arrive, &countsAtRest);
    if (rc) return rc;
    counts = countsAtRest;
  } else {
    DGPU_ALLOC(c, uint32_t, arena, (size_t)B * kNumSymbols);
    counts = c;
    DGPU_HIP(hipMemsetAsync(counts, 0, (size_t)B * kNumSymbols * 4, stream));
  }

  DecodeArgs d = decodeArgs(bd, devD, ft, outSuccess_dev, outSize_dev);
  d.accumulate = (uint32_t)accumulate;
  d.numSources = S;
  d.stats = counts;
  d.scale = opt.scale;
  if (withNorm) {
    rc = reduceNormBegin(arena, B, groupD, &d, stream);
    if (rc) {  // (nothing is launched: the counters are still zero)
      if (tempUsed) *tempUsed = arena.requested();
      return rc;
    }
  }
  rc = launchDecode(d, groupD, devD.work, reduceForm(true, anyRaw, opt.scale != 1.0f, withNorm), P, stream);
  if (!rc) {
    EncodeShared shared;
    rc = encodeCommon(arena, streamLease, stream, P, false, B, devE.in, devE.out, castType, groupsE[0], devE.work, shared,
                      countsAtRest ? nullptr : counts, outArchiveSize_dev, 0xffffffffu, countsAtRest);
    // (the normalisation may not have been enqueued: the counters are zero at rest whatever happened)
    if (rc && countsAtRest) (void)hipMemsetAsync(countsAtRest, 0, (size_t)B * kNumSymbols * 4, stream);
  }
  // (after the encoder: its failure handling above stays what it was; the partials are a region of their own, d.normPartials)
  if (!rc && withNorm) rc = reduceNormFinish(opt.norm, B, groupD, d, stream);
  if (tempUsed) *tempUsed = arena.requested();
  return rc;
}

}  // namespace

// ===========================================================================
// extern "C" surface
// ===========================================================================
extern "C" {

const char* dgpu_version(void) { return "dietgpu_amd 0.1 (gfx950)"; }
uint32_t dgpu_abi_version(void) { return DGPU_ABI_VERSION; }
const char* dgpu_last_error(void) { return g_lastError.c_str(); }

uint32_t dgpu_last_checksum_mismatches(int32_t* batchIdx, uint32_t* expected, uint32_t* got, uint32_t cap) {
  const uint32_t n = (uint32_t)g_mismatches.size();
  for (uint32_t i = 0; i < n && i < cap; ++i) {
    if (batchIdx) batchIdx[i] = g_mismatches[i].batch;
    if (expected) expected[i] = g_mismatches[i].expected;
    if (got) got[i] = g_mismatches[i].got;
  }
  return n;
}

static std::atomic<uint32_t> g_absentModulo{0};
}  // extern "C"
namespace {
uint32_t absentWorkgroupModulo() { return g_absentModulo.load(); }
}  // namespace
extern "C" {
void dgpu_debug_set_absent_workgroups(uint32_t modulo) { g_absentModulo.store(modulo); }
void dgpu_debug_set_encoder_dispatch(int mode) { g_encDispatch.store(mode < 0 ? -1 : (mode != 0)); }
void dgpu_debug_set_decoder_order(int order) { g_decOrder.store(order); }
void dgpu_debug_set_param_cache(int on) { g_paramCacheEnabled.store(on != 0); }
void dgpu_debug_set_work_lists(int mode) { g_workLists.store(mode < 0 ? -1 : (mode ? 1 : 0)); }
void dgpu_debug_set_size_classes(int mode) { g_sizeClasses.store(mode < 0 ? -1 : (mode ? 1 : 0)); }
void dgpu_set_histogram_load_policy(int mode) { g_histLoadPolicy.store(mode < 0 ? -1 : (mode != 0)); }
int dgpu_release_graph_state(void) {
  const int n = paramCache().releaseGraphPins();
  return n + streamRegistry().release(nullptr, true, true);
}

int dgpu_release_stream_state(void* stream) { return streamRegistry().release((hipStream_t)stream, false); }
int dgpu_release_all_stream_state(void) { return streamRegistry().release(nullptr, true); }
uint32_t dgpu_debug_stream_state_count(void) { return (uint32_t)streamRegistry().size(); }
int64_t dgpu_debug_counters_nonzero(void* stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess || st != hipStreamCaptureStatusNone) {
    (void)hipGetLastError();
    return -1;  // (a synchronise would invalidate a capture)
  }
  hipError_t e = hipSuccess;
  StreamState* s = streamRegistry().acquire((hipStream_t)stream, &e, false);  // `busy` held: no call frees the counters underneath
  if (!s) return -1;
  int64_t n = -1;
  std::vector<uint32_t> host(kCounterWordsArrive + kCounterWordsAcc + kCounterWordsSpill);
  if (s->counters && hipStreamSynchronize((hipStream_t)stream) == hipSuccess &&
      hipMemcpy(host.data(), s->counters, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess) {
    n = (int64_t)std::count_if(host.begin(), host.end(), [](uint32_t w) { return w != 0u; });
  }
  s->busy.unlock();
  return n;
}

void dgpu_prof_enable(int on) {
  ProfState& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  p.enabled = on != 0;
}

void dgpu_prof_reset(void) {
  ProfState& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  for (auto& s : p.open) {
    (void)hipEventDestroy(s.start);
    (void)hipEventDestroy(s.stop);
  }
  p.open.clear();
  p.acc.clear();
}

int dgpu_prof_summary(char* buf, size_t cap) {
  ProfState& p = prof();
  std::lock_guard<std::mutex> g(p.mu);
  for (auto& s : p.open) {
    float ms = 0.f;
    if (hipEventSynchronize(s.stop) == hipSuccess && hipEventElapsedTime(&ms, s.start, s.stop) == hipSuccess) {
      auto& a = p.acc[s.name];
      a.first += 1;
      a.second += ms;
    }
    (void)hipEventDestroy(s.start);
    (void)hipEventDestroy(s.stop);
  }
  p.open.clear();
  std::string out = "{";
  bool first = true;
  for (auto& kv : p.acc) {
    char line[256];
    snprintf(line, sizeof(line), "%s\"%s\": {\"launches\": %llu, \"total_ms\": %.6f}", first ? "" : ", ",
             kv.first.c_str(), (unsigned long long)kv.second.first, kv.second.second);
    out += line;
    first = false;
  }
  out += "}";
  if (out.size() + 1 > cap) return -1;
  memcpy(buf, out.c_str(), out.size() + 1);
  return (int)out.size();
}

uint32_t dgpu_ans_max_compressed_size(uint32_t bytes) { return maxCompressedSizeHost(bytes); }

uint32_t dgpu_float_max_compressed_size(uint32_t ft, uint32_t n) {
  const uint32_t ans = maxCompressedSizeHost(n);
  if (ans == 0u) return 0u;  // beyond the reference's INT32_MAX guard
  const uint64_t total = 16ull + ans + (ft == kFloat32 ? 2ull * roundUp(n, 8u) + roundUp(n, 16u) : (uint64_t)roundUp(n, 16u));
  return total > 0xffffffffull ? 0u : (uint32_t)total;
}

static size_t encodeTempBytes(uint32_t B, uint32_t maxBytes, uint32_t wordBytes, bool spills) {
  size_t tiles = std::max(tilesFor(maxBytes), 1u);
  size_t parts = histPartsFor(B, maxBytes * wordBytes, true);
  size_t t = 0;
  t += alignUp((size_t)B * 4, kTempAlign);                                        // checksums
  // partial histograms: the rectangle, or the list of a batch whose elements differ widely in size (planHistList)
  t += alignUp(std::max((size_t)B * parts, (size_t)B + kHistTargetWgsForListsRaw + 16u) * kNumSymbols * 4, kTempAlign);
  t += alignUp((size_t)B * kNumSymbols * 16, kTempAlign);                         // encoder table
  t += alignUp((size_t)B * tiles * 8, kTempAlign);                                // tile descriptors
  t += alignUp((size_t)B * tiles * 4, kTempAlign);                                // tile claim words
  if (tiles > kLookbackGroup) t += alignUp((size_t)B * divUp((uint32_t)tiles, kLookbackGroup) * (kGroupArriveStride + 1u) * 8, kTempAlign);  // look-back groups
  if (spills) {
    // spill slots of the persistent encoder workgroups (bounded by what fits on the chip)
    size_t perCu = (160u * 1024u) / encLdsBytes(9, true, kBFloat16, kBlocksPerTile);
    size_t grid = std::min((size_t)B * tiles, perCu * numComputeUnits());
    t += alignUp(grid * kBlocksPerTile * encSpillSlotWords(11) * 2, kTempAlign);
  }
  return t + kTempAlign;
}

size_t dgpu_ans_encode_temp_bytes(uint32_t B, uint32_t maxBytes) {
  return encodeTempBytes(B, maxBytes, 1, encodeSpills(0));
}

size_t dgpu_ans_decode_temp_bytes(uint32_t B, uint32_t maxBytes, int probBits) {
  (void)maxBytes;
  (void)probBits;  // the decode LUT is built in LDS by each workgroup
  size_t t = 0;
  t += 3 * alignUp((size_t)B * 8, kTempAlign);  // checksum verification scratch
  return t + kTempAlign;
}

size_t dgpu_float_compress_temp_bytes(uint32_t ft, uint32_t B, uint32_t maxFloats) {
  // no exponent plane: the split is fused into the encoder
  return encodeTempBytes(B, maxFloats, validFloatType(ft) ? floatWordBytes(ft) : 4u, true);
}

size_t dgpu_float_reduce_compress_temp_bytes(uint32_t ft, uint32_t B, uint32_t maxWords) {
  // the compress side's, and the counts of a batch that is too large for the stream's counters
  return dgpu_float_compress_temp_bytes(ft, B, maxWords) + (B > kAccElements ? alignUp((size_t)B * kNumSymbols * 4, kTempAlign) : 0u);
}

size_t dgpu_float_decompress_temp_bytes(uint32_t ft, uint32_t B, uint32_t maxFloats, int probBits) {
  (void)ft;
  return dgpu_ans_decode_temp_bytes(B, maxFloats, probBits);
}

// ---- encode ----------------------------------------------------------------
int dgpu_ans_encode_batch_stride(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, uint32_t inPerBatchSize, uint32_t inPerBatchStride,
    const uint32_t* histogram_dev, void* out_dev, uint32_t outPerBatchStride,
    uint32_t* outSize_dev, void* stream) {
  Batch b;
  int rc = strideBatch(&b, numInBatch, strideSide(in_dev, inPerBatchStride, DGPU_ANS_REQUIRED_ALIGNMENT, kMsgAnsIn),
                       strideSide(out_dev, outPerBatchStride, 16, kMsgCompOut), inPerBatchSize, false);
  if (rc) return rc;
  return ansEncodeImpl(temp_dev, tempBytes, tempUsed, probBits, useChecksum, b, histogram_dev, outSize_dev, (hipStream_t)stream);
}

int dgpu_ans_encode_batch_pointer(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inSize,
    const uint32_t* histogram_dev, void* const* out, uint32_t* outSize_dev, void* stream) {
  Batch b;
  int rc = pointerBatch(&b, numInBatch, ptrSide(in, DGPU_ANS_REQUIRED_ALIGNMENT, kMsgAnsIn), ptrSide(out, 16, kMsgCompOut), inSize);
  if (rc) return rc;
  return ansEncodeImpl(temp_dev, tempBytes, tempUsed, probBits, useChecksum, b, histogram_dev, outSize_dev, (hipStream_t)stream);
}

int dgpu_ans_encode_batch_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, const uint32_t* inSplitSizes,
    const uint32_t* histogram_dev, void* out_dev, uint32_t outStride, uint32_t* outSize_dev,
    void* stream) {
  Batch b;
  int rc = splitBatch(&b, numInBatch, strideSide(in_dev, 0, DGPU_ANS_REQUIRED_ALIGNMENT, kMsgAnsIn), inSplitSizes, 1u,
                      DGPU_ANS_REQUIRED_ALIGNMENT, strideSide(out_dev, outStride, 16, kMsgCompOut), false);
  if (rc) return rc;
  return ansEncodeImpl(temp_dev, tempBytes, tempUsed, probBits, useChecksum, b, histogram_dev, outSize_dev, (hipStream_t)stream);
}

// ---- decode ----------------------------------------------------------------
int dgpu_ans_decode_batch_stride(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, uint32_t inPerBatchStride, void* out_dev,
    uint32_t outPerBatchStride, uint32_t outPerBatchCapacity, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  Batch b;
  int rc = strideBatch(&b, numInBatch, strideSide(in_dev, inPerBatchStride, 16, kMsgCompIn), strideSide(out_dev, outPerBatchStride),
                       outPerBatchCapacity, true);
  if (rc) return rc;
  return decodeImpl(temp_dev, tempBytes, tempUsed, 0, probBits, useChecksum, b, outSuccess_dev, outSize_dev, (hipStream_t)stream, errBatch);
}

// (ft: 0 for raw bytes; inBytes: the *_bounded entry points)
static int decodePointerCommon(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t ft, int probBits,
    int useChecksum, uint32_t numInBatch, const void* const* in, void* const* out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream,
    int32_t* errBatch, const uint32_t* inBytes = nullptr) {
  Batch b;
  int rc = pointerBatch(&b, numInBatch, ptrSide(in, 16, kMsgCompIn), ptrSide(out), outCapacity, inBytes);
  if (rc) return rc;
  return decodeImpl(temp_dev, tempBytes, tempUsed, ft, probBits, useChecksum, b, outSuccess_dev, outSize_dev, (hipStream_t)stream, errBatch);
}

int dgpu_ans_decode_batch_pointer(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  return decodePointerCommon(temp_dev, tempBytes, tempUsed, 0, probBits, useChecksum, numInBatch,
                             in, out, outCapacity, outSuccess_dev, outSize_dev, stream, errBatch);
}

// (raw bytes: the output and every interior split 4-byte aligned)
static int decodeSplitCommon(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t ft, int probBits,
    int useChecksum, uint32_t numInBatch, const void* const* in, void* out_dev,
    const uint32_t* outSplitSizes, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream,
    int32_t* errBatch, const uint32_t* inBytes = nullptr) {
  const Side outSide = ft ? strideSide(out_dev, 0) : strideSide(out_dev, 0, DGPU_ANS_REQUIRED_ALIGNMENT, "output must be 4-byte aligned");
  Batch b;
  int rc = splitBatch(&b, numInBatch, outSide, outSplitSizes, ft ? floatWordBytes(ft) : 1u, ft ? 0u : DGPU_ANS_REQUIRED_ALIGNMENT,
                      ptrSide(in, 16, kMsgCompIn), true, inBytes);
  if (rc) return rc;
  return decodeImpl(temp_dev, tempBytes, tempUsed, ft, probBits, useChecksum, b, outSuccess_dev, outSize_dev, (hipStream_t)stream, errBatch);
}

int dgpu_ans_decode_batch_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, void* out_dev, const uint32_t* outSplitSizes,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  return decodeSplitCommon(temp_dev, tempBytes, tempUsed, 0, probBits, useChecksum, numInBatch, in,
                           out_dev, outSplitSizes, outSuccess_dev, outSize_dev, stream, errBatch);
}

// ---- decode with known input sizes ("bounded") ---------------------------------
// Same as the four pointer / split-size decode entry points, plus `inBytes` (HOST array): the bytes available at
// in[i].  The reference API carries no compressed sizes, so a truncated archive is followed past its buffer
// there; the tensor API knows every tensor's size and uses these.
int dgpu_ans_decode_batch_pointer_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes, void* const* out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  return decodePointerCommon(temp_dev, tempBytes, tempUsed, 0, probBits, useChecksum, numInBatch, in, out, outCapacity,
                             outSuccess_dev, outSize_dev, stream, errBatch, inBytes);
}
int dgpu_ans_decode_batch_split_size_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes, void* out_dev,
    const uint32_t* outSplitSizes, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  return decodeSplitCommon(temp_dev, tempBytes, tempUsed, 0, probBits, useChecksum, numInBatch, in, out_dev,
                           outSplitSizes, outSuccess_dev, outSize_dev, stream, errBatch, inBytes);
}
int dgpu_float_decompress_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes, void* const* out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  return decodePointerCommon(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum, numInBatch, in, out,
                             outCapacity, outSuccess_dev, outSize_dev, stream, errBatch, inBytes);
}
int dgpu_float_decompress_split_size_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes, void* out_dev,
    const uint32_t* outSplitSizes, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream, int32_t* errBatch) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  return decodeSplitCommon(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum, numInBatch, in, out_dev,
                           outSplitSizes, outSuccess_dev, outSize_dev, stream, errBatch, inBytes);
}

// ---- ranged decode (no upstream equivalent) -------------------------------------
int dgpu_ans_decode_batch_pointer_range(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, int probBits, uint32_t numInBatch,
    const void* const* in, const uint32_t* inBytes, const uint32_t* firstBlock, const uint32_t* numBlocks,
    void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  return decodeRangeImpl(tempUsed, 0, probBits, numInBatch, in, inBytes, firstBlock, numBlocks, out, outCapacity,
                         outSuccess_dev, outSize_dev, (hipStream_t)stream);
}
int dgpu_float_decompress_range(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, uint32_t numInBatch,
    const void* const* in, const uint32_t* inBytes, const uint32_t* firstBlock, const uint32_t* numBlocks,
    void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  return decodeRangeImpl(tempUsed, floatType, probBits, numInBatch, in, inBytes, firstBlock, numBlocks, out, outCapacity,
                         outSuccess_dev, outSize_dev, (hipStream_t)stream);
}

// ---- decode-accumulate (no upstream equivalent) ----------------------------------
int dgpu_float_decode_accumulate(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes, void* const* out, const uint32_t* outCapacity,
    uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  return decodeAccumulateImpl(tempUsed, floatType, probBits, accumulate, numInBatch, in, inBytes, out, outCapacity,
                              outSuccess_dev, outSize_dev, (hipStream_t)stream);
}

// ---- scaled decode-accumulate (no upstream equivalent) ----------------------------
int dgpu_float_decode_accumulate_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, const void* const* in, const uint32_t* inBytes, void* const* out, const uint32_t* outCapacity,
    float scale, const float* scale_dev, uint32_t scaleStride, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  const DecodeFactor factor{scale, scale_dev, scaleStride};
  return decodeAccumulateImpl(tempUsed, floatType, probBits, accumulate, numInBatch, in, inBytes, out, outCapacity,
                              outSuccess_dev, outSize_dev, (hipStream_t)stream, &factor);
}

// ---- scaled decompress (no upstream equivalent) -----------------------------------
int dgpu_float_decode_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, uint32_t numInBatch,
    const void* const* in, const uint32_t* inBytes, void* const* out, const uint32_t* outCapacity, float scale,
    const float* scale_dev, uint32_t scaleStride, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  return decodeScaledImpl(tempUsed, floatType, probBits, numInBatch, in, inBytes, out, outCapacity, scale, scale_dev, scaleStride,
                          outSuccess_dev, outSize_dev, (hipStream_t)stream);
}

// ---- decode-update (no upstream equivalent) ----------------------------------------
int dgpu_float_decode_update(
    uint32_t floatType, int probBits, int accumulate, uint32_t numInBatch, const void* const* in, const uint32_t* inBytes,
    void* const* out, const uint32_t* outCapacity, float scale, const float* scale_dev, uint32_t scaleStride, uint64_t seed,
    const uint64_t* seed_dev, uint32_t firstMember, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  return decodeUpdateImpl(floatType, probBits, accumulate, numInBatch, in, inBytes, out, outCapacity, scale, scale_dev, scaleStride,
                          seed, seed_dev, firstMember, outSuccess_dev, outSize_dev, (hipStream_t)stream);
}

// ---- the reduce family (no upstream equivalent) -------------------------------------
// Eight entry points over decodeReduceImpl / reduceCompressImpl: each states which ReduceOptions {mixed, kinds, scale,
// norm} it passes.  Decode-reduce takes temp memory for the norm partials only.
static bool scaleOk(float scale) { return std::isfinite(scale) && scale != 0.0f; }

int dgpu_float_decode_reduce(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, void* const* out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  return decodeReduceImpl(tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, out, outCapacity,
                          outSuccess_dev, outSize_dev, (hipStream_t)stream, ReduceOptions());
}

int dgpu_float_reduce_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, void* const* acc,
    const uint32_t* outCapacity, void* const* outArchive, uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    uint32_t* outArchiveSize_dev, void* stream) {
  return reduceCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, acc,
                            outCapacity, outArchive, outSuccess_dev, outSize_dev, outArchiveSize_dev, (hipStream_t)stream, ReduceOptions());
}

// mixed sources: archives and raw rows of floatType words; sourceKind must be given
int dgpu_float_decode_reduce_mixed(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, const uint8_t* sourceKind,
    void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  return decodeReduceImpl(tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, out, outCapacity,
                          outSuccess_dev, outSize_dev, (hipStream_t)stream, ReduceOptions{true, sourceKind});
}

int dgpu_float_reduce_compress_mixed(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, const uint8_t* sourceKind,
    void* const* acc, const uint32_t* outCapacity, void* const* outArchive, uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    uint32_t* outArchiveSize_dev, void* stream) {
  return reduceCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, acc,
                            outCapacity, outArchive, outSuccess_dev, outSize_dev, outArchiveSize_dev, (hipStream_t)stream,
                            ReduceOptions{true, sourceKind});
}

// scaled: acc = fl32(sum * scale) in the reduce kernel
// (sourceKind NULL: every source is an archive.  The scale is checked first: nothing is enqueued for a bad one.)
int dgpu_float_decode_reduce_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, const uint8_t* sourceKind,
    float scale, void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream) {
  (void)temp_dev;
  (void)tempBytes;
  DGPU_REQUIRE(scaleOk(scale), "decode-reduce: scale must be finite and not zero");
  return decodeReduceImpl(tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, out, outCapacity,
                          outSuccess_dev, outSize_dev, (hipStream_t)stream, ReduceOptions{sourceKind != nullptr, sourceKind, scale});
}

int dgpu_float_reduce_compress_scaled(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, const uint8_t* sourceKind,
    float scale, void* const* acc, const uint32_t* outCapacity, void* const* outArchive, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, void* stream) {
  DGPU_REQUIRE(scaleOk(scale), "reduce-compress: scale must be finite and not zero");
  return reduceCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, acc,
                            outCapacity, outArchive, outSuccess_dev, outSize_dev, outArchiveSize_dev, (hipStream_t)stream,
                            ReduceOptions{sourceKind != nullptr, sourceKind, scale});
}

// norm: the reduce call also reports the squared norm and the non-finite count of what it leaves
// (both outputs NULL: the scaled call.  Scale and alignment are checked first: nothing is enqueued for a bad one.)
size_t dgpu_float_reduce_norm_temp_bytes(uint32_t floatType, uint32_t numInBatch, uint32_t maxWords, int compress) {
  // (the tiles of the launch, bounded so that the figure never falls as maxWords grows: 8 blocks are two 4-block tiles,
  // 9 blocks one 16-block tile)
  const uint32_t blocks = divUp(maxWords, kBlockSize);
  const uint32_t tiles = std::max({divUp(blocks, kDecBlocksPerTile), std::min(divUp(blocks, kDecBlocksPerSmallTile), 2u), 1u});
  return alignUp(reduceNormPartialBytes(numInBatch, tiles), kTempAlign) + kTempAlign +
      (compress ? dgpu_float_reduce_compress_temp_bytes(floatType, numInBatch, maxWords) : 0u);
}

int dgpu_float_decode_reduce_norm(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, const uint8_t* sourceKind,
    float scale, void* const* out, const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev,
    double* outSumSq_dev, uint32_t* outNonFinite_dev, void* stream) {
  DGPU_REQUIRE(scaleOk(scale), "decode-reduce: scale must be finite and not zero");
  return decodeReduceImpl(tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, out, outCapacity,
                          outSuccess_dev, outSize_dev, (hipStream_t)stream,
                          ReduceOptions{sourceKind != nullptr, sourceKind, scale, {outSumSq_dev, outNonFinite_dev, temp_dev, tempBytes}});
}

int dgpu_float_reduce_compress_norm(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int accumulate,
    uint32_t numInBatch, uint32_t numSources, const void* const* in, const uint32_t* inBytes, const uint8_t* sourceKind,
    float scale, void* const* acc, const uint32_t* outCapacity, void* const* outArchive, uint8_t* outSuccess_dev,
    uint32_t* outSize_dev, uint32_t* outArchiveSize_dev, double* outSumSq_dev, uint32_t* outNonFinite_dev, void* stream) {
  DGPU_REQUIRE(scaleOk(scale), "reduce-compress: scale must be finite and not zero");
  // (the partials come out of the arena of the call: the norm has no region of its own)
  return reduceCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, accumulate, numInBatch, numSources, in, inBytes, acc,
                            outCapacity, outArchive, outSuccess_dev, outSize_dev, outArchiveSize_dev, (hipStream_t)stream,
                            ReduceOptions{sourceKind != nullptr, sourceKind, scale, {outSumSq_dev, outNonFinite_dev}});
}

// ---- float stride batches with capacities on both sides (the compressed collectives) --------------------
int dgpu_float_compress_stride_capped(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, uint32_t inWords, uint32_t inStrideBytes, void* out_dev,
    uint32_t outStrideBytes, uint32_t outCapacityBytes, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  bool done;
  int rc = checkCall(probBits, numInBatch, floatType, tempUsed, /*errBatch*/ nullptr, &done, "tensor larger than 1717538816 words (GpuANSEncode.cu:22)", inWords);
  if (rc) return rc;
  const char* const outMsg = "compressed output rows, their stride and their capacity must be 16-byte aligned";
  Batch b;
  rc = strideBatch(&b, numInBatch, strideSide(in_dev, inStrideBytes, floatWordBytes(floatType), kMsgFloatIn),
                   strideSide(out_dev, outStrideBytes, 16, outMsg), inWords, false);
  if (rc) return rc;
  DGPU_REQUIRE(outCapacityBytes % 16 == 0, outMsg);
  DGPU_REQUIRE(numInBatch <= 1 || outCapacityBytes <= outStrideBytes, "outCapacityBytes must not exceed outStrideBytes");
  DGPU_REQUIRE(inWords > kBlockSize, "capped compression needs rows of more than one 4096-word block");
  // everything except the block data is stored unconditionally: it must fit
  const uint32_t nb = divUp(inWords, kBlockSize);
  const uint64_t fixed = (uint64_t)ansOffsetInArchive(floatType, inWords) + ansOverhead(nb);
  DGPU_REQUIRE(fixed <= outCapacityBytes, "outCapacityBytes is smaller than the archive's header, tables and non-compressed planes");
  if (done) return DGPU_OK;  // (an empty batch, after the checks of its arguments)
  return encodeBatch(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum, b, nullptr, outSize_dev, (hipStream_t)stream, outCapacityBytes);
}

int dgpu_float_decompress_stride_bounded(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits, int useChecksum,
    uint32_t numInBatch, const void* in_dev, uint32_t inStrideBytes, uint32_t inBytes, void* out_dev,
    uint32_t outStrideBytes, uint32_t outCapacityWords, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream,
    int32_t* errBatch) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  Batch b;
  int rc = strideBatch(&b, numInBatch, strideSide(in_dev, inStrideBytes, 16, kMsgCompIn),
                       strideSide(out_dev, outStrideBytes, floatWordBytes(floatType), "float output must be float-word aligned"),
                       outCapacityWords, true, inBytes);
  if (rc) return rc;
  DGPU_REQUIRE(inBytes != 0, "inBytes must be the bytes available per compressed row");
  return decodeImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum, b, outSuccess_dev, outSize_dev, (hipStream_t)stream, errBatch);
}

// ---- info ------------------------------------------------------------------
int dgpu_ans_get_compressed_info_device(
    const void* const* in_dev, uint32_t numInBatch, uint32_t* outSizes_dev,
    uint32_t* outChecksum_dev, void* stream) {
  if (numInBatch == 0 || (!outSizes_dev && !outChecksum_dev)) return DGPU_OK;
  BatchView in = viewPointers((const uint64_t*)in_dev, nullptr, 0);
  hipLaunchKernelGGL(k_ans_info, dim3(divUp(numInBatch, 128)), dim3(128), 0, (hipStream_t)stream,
                     in, numInBatch, outSizes_dev, outChecksum_dev);
  DGPU_HIP(hipGetLastError());
  return DGPU_OK;
}

// (the *_get_compressed_info entry points: HOST array of archive pointers -> the array on the device)
static int uploadArchivePointers(const void* const* in, uint32_t numInBatch, hipStream_t stream, DeviceBatch* d) {
  Batch b;
  b.inPtrs.resize(numInBatch);
  for (uint32_t i = 0; i < numInBatch; ++i) b.inPtrs[i] = (uint64_t)(uintptr_t)in[i];
  StreamLease streamLease(stream);
  return resolveBatch(b, false, streamLease, d);  // (no out side: never stride views, see asStrideViews)
}

int dgpu_ans_get_compressed_info(
    void* temp_dev, size_t tempBytes, const void* const* in, uint32_t numInBatch,
    uint32_t* outSizes_dev, uint32_t* outChecksum_dev, void* stream) {
  if (numInBatch == 0 || (!outSizes_dev && !outChecksum_dev)) return DGPU_OK;
  (void)temp_dev;
  (void)tempBytes;
  DeviceBatch d;
  int rc = uploadArchivePointers(in, numInBatch, (hipStream_t)stream, &d);
  if (rc) return rc;
  return dgpu_ans_get_compressed_info_device((const void* const*)d.in.ptrs, numInBatch, outSizes_dev, outChecksum_dev, stream);
}

int dgpu_float_get_compressed_info_device(
    const void* const* in_dev, uint32_t numInBatch, uint32_t* outSizes_dev,
    uint32_t* outTypes_dev, uint32_t* outChecksum_dev, void* stream) {
  if (numInBatch == 0 || (!outSizes_dev && !outTypes_dev && !outChecksum_dev)) return DGPU_OK;
  BatchView in = viewPointers((const uint64_t*)in_dev, nullptr, 0);
  hipLaunchKernelGGL(k_float_info, dim3(divUp(numInBatch, 128)), dim3(128), 0, (hipStream_t)stream,
                     in, numInBatch, outSizes_dev, outTypes_dev, outChecksum_dev);
  DGPU_HIP(hipGetLastError());
  return DGPU_OK;
}

int dgpu_float_get_compressed_info(
    void* temp_dev, size_t tempBytes, const void* const* in, uint32_t numInBatch,
    uint32_t* outSizes_dev, uint32_t* outTypes_dev, uint32_t* outChecksum_dev, void* stream) {
  if (numInBatch == 0 || (!outSizes_dev && !outTypes_dev && !outChecksum_dev)) return DGPU_OK;
  (void)temp_dev;
  (void)tempBytes;
  DeviceBatch d;
  int rc = uploadArchivePointers(in, numInBatch, (hipStream_t)stream, &d);
  if (rc) return rc;
  return dgpu_float_get_compressed_info_device((const void* const*)d.in.ptrs, numInBatch, outSizes_dev, outTypes_dev, outChecksum_dev, stream);
}

// ---- float codec -------------------------------------------------------------
int dgpu_float_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    int useChecksum, uint32_t numInBatch, const void* const* in, const uint32_t* inSize,
    void* const* out, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  Batch b;
  int rc = pointerBatch(&b, numInBatch, ptrSide(in, floatWordBytes(floatType), kMsgFloatIn), ptrSide(out, 16, kMsgCompOut), inSize);
  if (rc) return rc;
  return floatCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum, b, outSize_dev, (hipStream_t)stream);
}

// ---- cast-compress (no upstream equivalent) ------------------------------------------
// float32 words in, ordinary float16 / bfloat16 archives out: the rounding is fused into the histogram and the encoder
// (kernels_encode.h, ChunkSourceCast).  No checksum: it covers the 16-bit words, which never reach memory.
int dgpu_float_cast_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    uint32_t numInBatch, const void* const* in, const uint32_t* inSize,
    void* const* out, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(floatType == kFloat16 || floatType == kBFloat16, "floatType of a cast archive must be float16 or bfloat16");
  Batch b;
  int rc = pointerBatch(&b, numInBatch, ptrSide(in, 4, "float32 input must be 4-byte aligned"), ptrSide(out, 16, kMsgCompOut), inSize);
  if (rc) return rc;
  return floatCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, 0, b, outSize_dev, (hipStream_t)stream, true);
}

// ---- feedback cast-compress (no upstream equivalent) -----------------------------------
// Cast-compress of x + e with the rounding error stored back as the next call's e (kernels_encode.h,
// ChunkSourceFeedback): the cast call with a source flag and two more pointer arrays in its batch.
int dgpu_float_feedback_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    uint32_t numInBatch, const void* const* in, const uint32_t* inSize, const void* const* residualIn,
    void* const* residualOut, void* const* out, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(floatType == kFloat16 || floatType == kBFloat16, "floatType of a feedback archive must be float16 or bfloat16");
  DGPU_REQUIRE(validProbBits(probBits), "probBits must be 9, 10 or 11");
  DGPU_REQUIRE(numInBatch <= 65535u, "numInBatch must be <= 65535");
  DGPU_REQUIRE(numInBatch == 0 || residualOut, "feedback compress: residualOut must not be null");
  DGPU_REQUIRE(numInBatch == 0 || (in && inSize && out), "feedback compress: in, inSize and out must not be null");
  // every range the call reads or writes, for the overlap rule: an element's residualOut may BE its residualIn
  std::vector<std::pair<uint64_t, uint64_t>> ranges;
  ranges.reserve((size_t)numInBatch * 4u);
  for (uint32_t i = 0; i < numInBatch; ++i) {
    DGPU_REQUIRE(in[i] && residualOut[i] && out[i] && (!residualIn || residualIn[i]), "feedback compress: null entry in a pointer array");
    DGPU_REQUIRE(encodableSize(inSize[i]),
                 "tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX (GpuANSEncode.cu:22)");
    const uint64_t x = (uint64_t)(uintptr_t)in[i], ro = (uint64_t)(uintptr_t)residualOut[i], bytes = (uint64_t)inSize[i] * 4u;
    const uint64_t ri = residualIn ? (uint64_t)(uintptr_t)residualIn[i] : ro;
    DGPU_REQUIRE(x % 4 == 0 && ro % 4 == 0 && ri % 4 == 0, "feedback compress: float32 input and residuals must be 4-byte aligned");
    DGPU_REQUIRE(x % 16 == ro % 16 && x % 16 == ri % 16, "feedback compress: in[i], residualIn[i] and residualOut[i] must be congruent modulo 16");
    if (bytes == 0) continue;
    ranges.emplace_back(x, x + bytes);
    ranges.emplace_back(ro, ro + bytes);
    if (ri != ro) ranges.emplace_back(ri, ri + bytes);
    const uint64_t o = (uint64_t)(uintptr_t)out[i];
    ranges.emplace_back(o, o + dgpu_float_max_compressed_size(floatType, inSize[i]));
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t k = 1; k < ranges.size(); ++k) {
    DGPU_REQUIRE(ranges[k - 1].second <= ranges[k].first,
                 "feedback compress: in, residualIn, residualOut and out must not overlap (residualOut[i] == residualIn[i] excepted)");
  }
  Batch b;
  int rc = pointerBatch(&b, numInBatch, ptrSide(in, 4, "float32 input must be 4-byte aligned"), ptrSide(out, 16, kMsgCompOut), inSize);
  if (rc) return rc;
  b.resOutPtrs.resize(numInBatch);
  for (uint32_t i = 0; i < numInBatch; ++i) b.resOutPtrs[i] = (uint64_t)(uintptr_t)residualOut[i];
  if (residualIn) {
    b.resInPtrs.resize(numInBatch);
    for (uint32_t i = 0; i < numInBatch; ++i) b.resInPtrs[i] = (uint64_t)(uintptr_t)residualIn[i];
  }
  return floatCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, 0, b, outSize_dev, (hipStream_t)stream, true, RollingCounts{}, true);
}

// ---- stochastic cast-compress (no upstream equivalent) ---------------------------------
// Cast-compress whose every rounding is stochastic (kernels_encode.h, ChunkSourceStochastic): the cast call with a source
// flag and three values handed to its two launches.  Temporaries come from the stream's slab.
int dgpu_float_stochastic_compress(
    uint32_t floatType, int probBits, uint32_t numInBatch, const void* const* in, const uint32_t* inSize, uint64_t seed,
    const uint64_t* seed_dev, uint32_t firstMember, void* const* out, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(floatType == kFloat16 || floatType == kBFloat16, "stochastic compress: floatType of the archive must be float16 or bfloat16");
  DGPU_REQUIRE(validProbBits(probBits), "probBits must be 9, 10 or 11");
  DGPU_REQUIRE(numInBatch <= 65535u, "numInBatch must be <= 65535");
  DGPU_REQUIRE((uintptr_t)seed_dev % 8u == 0u, "stochastic compress: seed_dev must be 8-byte aligned");
  DGPU_REQUIRE(numInBatch == 0 || (in && inSize && out), "stochastic compress: null array with numInBatch > 0");
  for (uint32_t i = 0; i < numInBatch; ++i) {
    DGPU_REQUIRE(encodableSize(inSize[i]),
                 "tensor larger than 1717538816 words: the maximum compressed size of its exponent plane exceeds INT32_MAX (GpuANSEncode.cu:22)");
  }
  Batch b;
  int rc = pointerBatch(&b, numInBatch, ptrSide(in, 4, "float32 input must be 4-byte aligned"), ptrSide(out, 16, kMsgCompOut), inSize);
  if (rc) return rc;
  const StochasticSeed sr{seed, seed_dev, firstMember};
  return floatCompressImpl(nullptr, 0, nullptr, floatType, probBits, 0, b, outSize_dev, (hipStream_t)stream, true, RollingCounts{}, false, &sr);
}

// ---- rolling-table compress (no upstream equivalent) ------------------------------------
// The table of this call from the counts of the last one (countsIn_dev: no histogram pass), the counts of this call for
// the next one (countsOut_dev: the counting encoder).  float16 / bfloat16 archives only: the float32 encoder has no
// counting form.
int dgpu_float_rolling_compress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, uint32_t sourceFloat32, int probBits,
    uint32_t numInBatch, const void* const* in, const uint32_t* inSize, const uint32_t* countsIn_dev,
    uint32_t* countsOut_dev, void* const* out, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(floatType == kFloat16 || floatType == kBFloat16,
               "rolling compress: floatType of the archive must be float16 or bfloat16 (float32 archives: dgpu_float_compress)");
  DGPU_REQUIRE(sourceFloat32 <= 1u, "rolling compress: sourceFloat32 must be 0 or 1");
  DGPU_REQUIRE((uintptr_t)countsIn_dev % 4 == 0 && (uintptr_t)countsOut_dev % 4 == 0, "rolling compress: counts must be 4-byte aligned");
  if (!countsIn_dev && !countsOut_dev) {
    return sourceFloat32 ? dgpu_float_cast_compress(temp_dev, tempBytes, tempUsed, floatType, probBits, numInBatch, in, inSize, out, outSize_dev, stream)
                         : dgpu_float_compress(temp_dev, tempBytes, tempUsed, floatType, probBits, 0, numInBatch, in, inSize, out, outSize_dev, stream);
  }
  if (countsIn_dev && countsOut_dev && countsIn_dev != countsOut_dev) {
    const uintptr_t a = (uintptr_t)countsIn_dev, c = (uintptr_t)countsOut_dev, bytes = (uintptr_t)numInBatch * kNumSymbols * 4u;
    DGPU_REQUIRE(a + bytes <= c || c + bytes <= a, "rolling compress: countsIn_dev and countsOut_dev must be the same buffer or not overlap");
  }
  Batch b;
  int rc = pointerBatch(&b, numInBatch, sourceFloat32 ? ptrSide(in, 4, "float32 input must be 4-byte aligned") : ptrSide(in, 2, kMsgFloatIn),
                        ptrSide(out, 16, kMsgCompOut), inSize);
  if (rc) return rc;
  RollingCounts rolling;
  rolling.countsIn = countsIn_dev;
  rolling.countsOut = countsOut_dev;
  return floatCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, 0, b, outSize_dev, (hipStream_t)stream, sourceFloat32 != 0u, rolling);
}

int dgpu_float_compress_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    int useChecksum, uint32_t numInBatch, const void* in_dev, const uint32_t* inSplitSizes,
    void* out_dev, uint32_t outStride, uint32_t* outSize_dev, void* stream) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  Batch b;
  int rc = splitBatch(&b, numInBatch, strideSide(in_dev, 0), inSplitSizes, floatWordBytes(floatType), 0u,
                      strideSide(out_dev, outStride, 16, kMsgCompOut), false);
  if (rc) return rc;
  return floatCompressImpl(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum, b, outSize_dev, (hipStream_t)stream);
}

int dgpu_float_decompress(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    int useChecksum, uint32_t numInBatch, const void* const* in, void* const* out,
    const uint32_t* outCapacity, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream,
    int32_t* errBatch) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  return decodePointerCommon(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum,
                             numInBatch, in, out, outCapacity, outSuccess_dev, outSize_dev, stream,
                             errBatch);
}

int dgpu_float_decompress_split_size(
    void* temp_dev, size_t tempBytes, size_t* tempUsed, uint32_t floatType, int probBits,
    int useChecksum, uint32_t numInBatch, const void* const* in, void* out_dev,
    const uint32_t* outSplitSizes, uint8_t* outSuccess_dev, uint32_t* outSize_dev, void* stream,
    int32_t* errBatch) {
  DGPU_REQUIRE(validFloatType(floatType), kMsgFloatType);
  return decodeSplitCommon(temp_dev, tempBytes, tempUsed, floatType, probBits, useChecksum,
                           numInBatch, in, out_dev, outSplitSizes, outSuccess_dev, outSize_dev,
                           stream, errBatch);
}

// ---- building blocks for parity tests ----------------------------------------
int dgpu_ans_histogram_batch_stride(
    uint32_t numInBatch, const void* in_dev, uint32_t inPerBatchSize, uint32_t inPerBatchStride,
    uint32_t* histogram_dev, void* stream) {
  DGPU_REQUIRE(numInBatch <= 65535u, "numInBatch must be <= 65535");
  if (numInBatch == 0) return DGPU_OK;
  DGPU_HIP(hipMemsetAsync(histogram_dev, 0, (size_t)numInBatch * kNumSymbols * 4, (hipStream_t)stream));
  BatchView in = viewStride(in_dev, inPerBatchStride, inPerBatchSize);
  dim3 grid(gridX(inPerBatchSize, 32 * 1024, 64), numInBatch);
  HistFuse noFuse;
  noFuse.workMap = nullptr;
  noFuse.partBytes = 0;
  noFuse.arrive = nullptr;
  noFuse.acc = nullptr;
  noFuse.norm = NormalizeArgs{};
  noFuse.residual = BatchView{};
  noFuse.seed = 0;
  noFuse.seedPtr = nullptr;
  noFuse.firstMember = 0;
  const HistogramVariant hist = histogramVariant(0u, false, true);
  hipLaunchKernelGGL(hist.fn, grid, dim3(hist.threads), hist.ldsBytes, (hipStream_t)stream, in, histogram_dev, 0u, noFuse);
  DGPU_HIP(hipGetLastError());
  return DGPU_OK;
}

int dgpu_ans_calc_weights(
    uint32_t numInBatch, int probBits, const uint32_t* sizes_dev, uint32_t uniformSize,
    const uint32_t* histogram_dev, uint32_t* table_dev, void* stream) {
  DGPU_REQUIRE(validProbBits(probBits), "probBits must be 9, 10 or 11");
  if (numInBatch == 0) return DGPU_OK;
  NormalizeArgs n;
  n.sizes = viewPointers(nullptr, sizes_dev, uniformSize);
  n.hist = histogram_dev;
  n.smoothCounts = 0;
  n.countsOut = nullptr;
  n.histAcc = nullptr;
  n.histParts = 1;
  n.probBits = probBits;
  n.encTable = nullptr;
  n.refTable = (uint4*)table_dev;
  n.out = viewStride(nullptr, 0, 0);
  n.writeHeader = 0;
  n.floatType = 0;
  n.useChecksum = 0;
  n.checksum = nullptr;
  n.outSize = nullptr;
  n.floatUseChecksum = 0;
  n.tileDesc = nullptr;
  n.maxTiles = 0;
  n.claims = nullptr;
  n.numInBatch = numInBatch;
  n.tileBase = nullptr;
  n.tileSymbols = 0;
  n.groupWords = nullptr;
  n.groupWordsPerElement = 0;
  hipLaunchKernelGGL(k_normalize, dim3(numInBatch), dim3(256), 0, (hipStream_t)stream, n);
  DGPU_HIP(hipGetLastError());
  return DGPU_OK;
}

}  // extern "C"

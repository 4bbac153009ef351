// mcba_host.h -- the host runtime of libmcba.so, once for every translation unit with a host driver: error convention of the C ABI,
// resource cache, the buffers that go through it (DevBuf, PinnedBuf, OutBuf: an output the caller may leave out), the transfers
// of a call counted in elements, and the scaffold of a handle-less call (DeviceCall: stream, buffers through the cache, timing by
// host clock or by HIP events into the family's four or five slots).  g_error, g_fill_stream,
// g_park_on_release and the ResourceCache exist ONCE per library: declared here (hidden: not part of the ABI), defined in mcba_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

namespace mcba {
namespace host {

struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

#define HIP_OK(expr)                                                                                                  \
  do {                                                                                                                \
    hipError_t e_ = (expr);                                                                                           \
    if (e_ != hipSuccess) throw ::mcba::host::Error(std::string(#expr) + " failed: " + hipGetErrorString(e_));         \
  } while (0)

#define REQUIRE(cond, msg)                              \
  do {                                                  \
    if (!(cond)) throw ::mcba::host::Error(msg);        \
  } while (0)

// MCBA_PRIVATE: shared by the library's units, not part of its ABI.  RULE for a thread-local object declared with it: one WITHOUT a
// dynamic initialiser must be __thread, not thread_local -- an extern thread_local refers to its TLS init function, which nobody
// defines then, and as a hidden undefined weak symbol that reference does not resolve to null in a shared object (a crash on first use).
#define MCBA_PRIVATE __attribute__((visibility("hidden")))
MCBA_PRIVATE extern thread_local std::string g_error;         // text behind mcba_last_error()
MCBA_PRIVATE extern __thread hipStream_t g_fill_stream;       // stream of the running API call (see DevBuf::alloc)
MCBA_PRIVATE extern __thread bool g_park_on_release;          // set while the buffers of a handle or of a regular call end go away

// (g_fill_stream is valid for the duration of ONE API call: the entry points that allocate set it, every exit clears it)
#define API_BEGIN try {
#define API_END                                         \
  ::mcba::host::g_fill_stream = nullptr;                \
  return 0;                                             \
  }                                                     \
  catch (const std::exception& e) {                     \
    ::mcba::host::g_fill_stream = nullptr;              \
    ::mcba::host::g_error = e.what();                   \
    return 1;                                           \
  }                                                     \
  catch (...) {                                         \
    ::mcba::host::g_fill_stream = nullptr;              \
    ::mcba::host::g_error = "unknown error";            \
    return 1;                                           \
  }

MCBA_PRIVATE const char* dbg_switch(const char* name);   // experiment / path-forcing switches (mcba_api.hip, mcba_debug_set_switch)

// A launch that the runtime rejects (too much dynamic LDS, a bad grid) does not throw: it leaves an error behind and the stream lacks
// that kernel.  Every synchronisation point of the API collects the launch status; launches sized at run time check right away.
inline void check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw Error(std::string("kernel launch failed (") + what + "): " + hipGetErrorString(e));
}

// grid.x of a kernel that walks its workgroups' worth of work in a grid-stride loop: max(1, min(workgroups, builtin_cap, override)).
// The override is process-wide (mcba_debug_set_grid_cap; 0 = none: the launch has the grid the built-in cap gives it) and lets a test
// run the second and later rounds of such a loop on a small input.  The value returned is kept per thread for
// mcba_debug_last_capped_grid.  Defined in mcba_api.hip.
MCBA_PRIVATE int capped_grid(long long workgroups, long long builtin_cap);

inline double now_seconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Process-wide cache of the resources a handle or a handle-less call owns (~50 hipMalloc / hipFree pairs, four pinned buffers and a
// stream per handle cost more than the three bundle adjustments they serve: 4 ms of a 15 ms calibrate at the north-star rig).  An
// idle owner parks them here and the next one of the same shape takes them back, exact size match only.  Bounded (MCBA_CACHE_MB of
// device memory, default 512; 0 = off), emptied before an out-of-memory is reported; mcba_release_cached_memory() returns everything.
struct ResourceCache {
  static size_t cache_bytes_max() {
    static const size_t cap = [] {
      const char* e = getenv("MCBA_CACHE_MB");
      const long mb = e ? atol(e) : 512;
      return (size_t)(mb > 0 ? mb : 0) << 20;
    }();
    return cap;
  }
  static constexpr size_t HOST_BYTES_MAX = 64ull << 20;
  std::mutex m;
  std::multimap<std::pair<int, size_t>, void*> dev, host;   // (device, bytes) -> pointer
  std::vector<std::pair<int, hipStream_t>> streams, side_streams;
  size_t dev_bytes = 0, host_bytes = 0;
  static int device() {
    int d = 0;
    (void)hipGetDevice(&d);
    return d;
  }
  void* take(std::multimap<std::pair<int, size_t>, void*>& pool, size_t& total, size_t bytes) {
    std::lock_guard<std::mutex> lock(m);
    auto it = pool.find({device(), bytes});
    if (it == pool.end()) return nullptr;
    void* p = it->second;
    pool.erase(it);
    total -= bytes;
    return p;
  }
  // (resources are parked under the device of the handle that owned them, which need not be the caller's current device)
  static int& park_device() {
    static thread_local int d = -1;
    return d;
  }
  bool park(std::multimap<std::pair<int, size_t>, void*>& pool, size_t& total, size_t cap, void* p, size_t bytes) {
    std::lock_guard<std::mutex> lock(m);
    if (total + bytes > cap) return false;
    pool.insert({{park_device() >= 0 ? park_device() : device(), bytes}, p});
    total += bytes;
    return true;
  }
  void* take_dev(size_t bytes) { return take(dev, dev_bytes, bytes); }
  void* take_host(size_t bytes) { return take(host, host_bytes, bytes); }
  bool park_dev(void* p, size_t bytes) { return park(dev, dev_bytes, cache_bytes_max(), p, bytes); }
  bool park_host(void* p, size_t bytes) { return cache_bytes_max() > 0 && park(host, host_bytes, HOST_BYTES_MAX, p, bytes); }
  // (side = the non-blocking second stream of a handle, which carries the trial cost beside the speculative linearisation:
  //  its own pool -- the main stream must stay a blocking stream, the synchronous copies of the API rely on that.  Creating
  //  it anew cost every mcba_create 2-3 ms.)
  hipStream_t take_stream(bool side = false) {
    std::lock_guard<std::mutex> lock(m);
    auto& pool = side ? side_streams : streams;
    const int d = device();
    for (size_t i = 0; i < pool.size(); ++i)
      if (pool[i].first == d) {
        hipStream_t s = pool[i].second;
        pool.erase(pool.begin() + i);
        return s;
      }
    return nullptr;
  }
  bool park_stream(hipStream_t s, bool side = false) {
    std::lock_guard<std::mutex> lock(m);
    auto& pool = side ? side_streams : streams;
    if (pool.size() >= 4 || cache_bytes_max() == 0) return false;
    pool.push_back({park_device() >= 0 ? park_device() : device(), s});
    return true;
  }
  void clear() {
    std::lock_guard<std::mutex> lock(m);
    for (auto& e : dev) (void)hipFree(e.second);
    for (auto& e : host) (void)hipHostFree(e.second);
    for (auto& e : streams) (void)hipStreamDestroy(e.second);
    for (auto& e : side_streams) (void)hipStreamDestroy(e.second);
    dev.clear(); host.clear(); streams.clear(); side_streams.clear();
    dev_bytes = host_bytes = 0;
  }
};
MCBA_PRIVATE ResourceCache& resource_cache();   // the one cache of the library (mcba_api.hip)

// pinned host memory through the cache (hipHostMalloc is ~0.2 ms a call)
inline void* pinned_alloc(size_t bytes) {
  bytes = std::max<size_t>(bytes, 8);
  if (void* p = resource_cache().take_host(bytes)) return p;
  void* p = nullptr;
  hipError_t e = hipHostMalloc(&p, bytes);
  if (e == hipErrorOutOfMemory) {   // parked buffers are the first thing to give back
    (void)hipGetLastError();
    resource_cache().clear();
    e = hipHostMalloc(&p, bytes);
  }
  if (e != hipSuccess) throw std::runtime_error(std::string("hipHostMalloc failed: ") + hipGetErrorString(e));
  return p;
}
inline void pinned_free(void* p, size_t bytes) {
  bytes = std::max<size_t>(bytes, 8);
  if (p == nullptr) return;
  if (!(g_park_on_release && resource_cache().park_host(p, bytes))) (void)hipHostFree(p);
}
// a pinned staging buffer that lives as long as its scope
struct PinnedBuf {
  void* p;
  size_t bytes;
  explicit PinnedBuf(size_t n) : p(pinned_alloc(n)), bytes(n) {}
  PinnedBuf(const PinnedBuf&) = delete;
  ~PinnedBuf() { pinned_free(p, bytes); }
};

template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  explicit DevBuf(size_t count) { alloc(count, false); }   // n elements, not zero-filled
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  static size_t bytes_of(size_t count) { return (std::max<size_t>(count, 1) * sizeof(T) + 511) / 512 * 512; }
  void release() {
    if (p && !(g_park_on_release && resource_cache().park_dev(p, bytes_of(n)))) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count, bool zero = true) {
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (p == nullptr || n < count) {   // (a buffer that is large enough is reused: hipFree / hipMalloc cost ~100 us each)
      release();
      n = count;
      p = (T*)resource_cache().take_dev(bytes_of(count));
      if (p == nullptr) {
        hipError_t e = hipMalloc((void**)&p, bytes_of(count));
        if (e == hipErrorOutOfMemory) {   // memory parked by destroyed handles must never cause an out-of-memory failure
          (void)hipGetLastError();
          resource_cache().clear();
          e = hipMalloc((void**)&p, bytes_of(count));
        }
        if (e != hipSuccess) {
          p = nullptr;
          n = 0;
          throw Error(std::string("hipMalloc of ") + std::to_string(bytes_of(count)) + " bytes failed: " + hipGetErrorString(e));
        }
      }
    }
    if (zero) {
      // zero-fill ON THE HANDLE'S STREAM (g_fill_stream is set by every API entry that allocates): ordered against the
      // kernels that use the buffer, no host synchronisation per buffer (mcba_create makes ~40 of them).  Without a
      // stream: hipMemset on the NULL stream is asynchronous w.r.t. the host and not ordered against a non-blocking
      // stream (torch.cuda.Stream) -> wait.
      if (g_fill_stream != nullptr) {
        HIP_OK(hipMemsetAsync(p, 0, bytes, g_fill_stream));
      } else {
        HIP_OK(hipMemset(p, 0, bytes));
        HIP_OK(hipStreamSynchronize(nullptr));
      }
    }
  }
  template <typename V>
  void upload(const V& h) {   // std::vector<T> or SlotVec<T>
    alloc(h.size(), h.empty());
    if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  }
};

// The transfers of a call, on its stream, counted in ELEMENTS (no synchronisation).  upload_to / download_async take plain
// pointers: a run inside a packed buffer (d_out = pose | sse) is an offset pointer.
template <class T>
void upload_to(T* dev, const T* h, size_t n, hipStream_t st) {
  HIP_OK(hipMemcpyAsync(dev, h, n * sizeof(T), hipMemcpyHostToDevice, st));
}
template <class T>
void download_async(T* h, const T* dev, size_t n, hipStream_t st) {
  HIP_OK(hipMemcpyAsync(h, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
}
// a buffer of at least n elements filled from the host (not zero-filled; one that is large enough already is not touched)
template <class T>
void upload_async(DevBuf<T>& d, const T* h, size_t n, hipStream_t st) {
  d.alloc(n, false);
  upload_to(d.p, h, n, st);
}
template <class T>
void upload_vector(DevBuf<T>& d, const std::vector<T>& h, hipStream_t st) {
  if (h.empty()) return d.alloc(0, false);
  upload_async(d, h.data(), h.size(), st);
}

// An output the caller may leave out: allocated only if the host pointer is there, dev() null for the kernel if not, fetch()
// downloads it if it is (to `to`, where the result goes through a staging array first).  Declared AFTER the call object.
template <class T>
struct OutBuf {
  T* host;
  size_t n;
  DevBuf<T> d;
  OutBuf(T* host_or_null, size_t count) : host(host_or_null), n(count) {
    if (host) d.alloc(n, false);
  }
  T* dev() const { return host ? d.p : nullptr; }
  void fetch(hipStream_t st, T* to = nullptr) const {
    if (host) download_async(to ? to : host, d.p, n, st);
  }
};

// The timing slots of a handle-less family and the count that goes with them (mcba_debug_*_ms): what the slots mean is the
// family's business, how many it reports (4, or 5: two event-timed kernels) is stated where its getter is.  One thread_local
// instance per family (MCBA_TIMING_GETTER).
struct CallTiming {
  static constexpr int MAX_SLOTS = 5;
  double ms[MAX_SLOTS] = {0.0, 0.0, 0.0, 0.0, 0.0};
  int64_t count = 0;
  int n_slots;
  constexpr explicit CallTiming(int slots = 4) : n_slots(slots) {}
  void reset(int64_t n = 0) {
    for (double& v : ms) v = 0.0;
    count = n;
  }
  void report(double* ms_out, int64_t* count_out) const {   // (exactly n_slots doubles: callers of a four-slot family pass double[4])
    REQUIRE(ms_out, "null argument");
    for (int i = 0; i < n_slots; ++i) ms_out[i] = ms[i];
    if (count_out) *count_out = count;
  }
};

// One handle-less call on a stream of its own, its buffers going through the resource cache, timed into its family's slots.
// ORDER: declare it BEFORE every DevBuf / OutBuf / PinnedBuf of the call (or hold them as members of a type derived from it): its
// destructor then runs AFTER theirs -- they are parked while g_park_on_release still says how the call ended, then the stream goes
// back and the flag is cleared.
//   open()    lazy: a stream from the cache or a new one; a call with nothing to do returns before it, the device untouched
//   finish()  the regular end (the stream is synchronised): buffers are parked.  An exception leaves the flag false: they are freed.
// Two ways to time a call:
//   by host clock (pose table, intrinsics, hand-eye: plan | uploads | kernel | downloads)
//     stamp()   the next time stamp (the first is the construction); record(): the last one, and the intervals -> tm.ms[0..]
//   by HIP events around its n - 1 kernels (undistortion, triangulation: n = 2; localisation: n = 3), n + 2 slots:
//     open(n)          creates the events; the uploads start here
//     mark(i)          i == 0: the uploads are complete (synchronises) -> slot 0; records event i
//     end_kernels()    launch status, synchronises; event i - 1 .. event i -> slot i; the downloads start here
//     finish(count)    synchronises; downloads -> slot n, the whole call since construction -> slot n + 1, the count; then finish()
//     finish_prepared(count)   instead of it, n = 2: host preparation | uploads | kernel | downloads (stereo pairs)
struct DeviceCall {
  static constexpr int MAX_EVENTS = CallTiming::MAX_SLOTS - 2;
  CallTiming& tm;
  double t[5] = {now_seconds(), 0.0, 0.0, 0.0, 0.0};
  int n_stamps = 1;
  hipStream_t st = nullptr;
  hipEvent_t ev[MAX_EVENTS] = {};
  int n_events = 0;
  double t_up = 0.0, t_down = 0.0;
  explicit DeviceCall(CallTiming& timing) : tm(timing) {}
  DeviceCall(const DeviceCall&) = delete;
  void open(int events = 0) {
    REQUIRE(events == 0 || (events >= 2 && events + 2 <= tm.n_slots), "DeviceCall::open: the family's timing has no slots for these events");
    st = resource_cache().take_stream();
    if (st == nullptr) HIP_OK(hipStreamCreate(&st));
    g_fill_stream = st;
    for (; n_events < events; ++n_events) HIP_OK(hipEventCreate(&ev[n_events]));
    t_up = now_seconds();
  }
  void stamp() { t[n_stamps++] = now_seconds(); }
  void record() {
    stamp();
    for (int i = 0; i + 1 < n_stamps; ++i) tm.ms[i] = (t[i + 1] - t[i]) * 1e3;
  }
  void mark(int i) {
    if (i == 0) {
      HIP_OK(hipStreamSynchronize(st));
      tm.ms[0] = (now_seconds() - t_up) * 1e3;
    }
    HIP_OK(hipEventRecord(ev[i], st));
  }
  void end_kernels(const char* what) {
    check_launch(what);
    HIP_OK(hipStreamSynchronize(st));
    for (int i = 1; i < n_events; ++i) {
      float ms = 0.0f;
      HIP_OK(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
      tm.ms[i] = (double)ms;
    }
    t_down = now_seconds();
  }
  void finish() { g_park_on_release = true; }
  void finish(int64_t count) {
    HIP_OK(hipStreamSynchronize(st));
    const double now = now_seconds();
    tm.ms[n_events] = (now - t_down) * 1e3;
    tm.ms[n_events + 1] = (now - t[0]) * 1e3;
    tm.count = count;
    finish();
  }
  // the four-slot layout of a call with ONE event-timed kernel whose host preparation is worth a slot of its own (the views of every
  // stereo pair are counted on the host): after open(2), mark(0), mark(1), end_kernels() and the downloads,
  //   host preparation (construction .. open) | uploads | kernel (events) | downloads, and the count; then finish()
  void finish_prepared(int64_t count) {
    HIP_OK(hipStreamSynchronize(st));
    const double uploads = tm.ms[0], kernel = tm.ms[1];
    tm.ms[0] = (t_up - t[0]) * 1e3;
    tm.ms[1] = uploads;
    tm.ms[2] = kernel;
    tm.ms[3] = (now_seconds() - t_down) * 1e3;
    tm.count = count;
    finish();
  }
  ~DeviceCall() {
    for (int i = 0; i < n_events; ++i) (void)hipEventDestroy(ev[i]);
    if (st && !resource_cache().park_stream(st)) (void)hipStreamDestroy(st);
    g_park_on_release = false;
  }
};

// a family's timing (thread_local, this unit's own) and its mcba_debug_*_ms entry, which writes `slots` doubles and the count
#define MCBA_TIMING_GETTER(name, timing, slots)                             \
  namespace {                                                               \
  thread_local ::mcba::host::CallTiming timing(slots);                      \
  }                                                                         \
  extern "C" int32_t name(double* ms, int64_t* count) {                     \
    API_BEGIN                                                               \
    timing.report(ms, count);                                               \
    API_END                                                                 \
  }

}  // namespace host
}  // namespace mcba

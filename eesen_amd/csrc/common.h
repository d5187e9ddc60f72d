// common.h -- error plumbing, device buffers and launch helpers shared by the HIP sources.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <string>
#include <utility>

#include "../../include/eesen_hip.h"

namespace eesen {

// Internal failures travel as exceptions up to the C-ABI wrappers (capi.cpp), which turn them into a
// status code + thread-local message; nothing throws across the `extern "C"` boundary.
struct Error : public std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define EESEN_HIP_CHECK(expr)                                                                       \
  do {                                                                                              \
    hipError_t e_ = (expr);                                                                         \
    if (e_ != hipSuccess)                                                                           \
      throw ::eesen::Error(EESEN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + \
                                              __FILE__ + ":" + std::to_string(__LINE__) + ")");     \
  } while (0)

#define EESEN_REQUIRE(cond, code, msg)                                       \
  do {                                                                       \
    if (!(cond)) throw ::eesen::Error((code), std::string(msg) + " [" #cond "]"); \
  } while (0)

inline void check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw Error(EESEN_ERR_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
}

// Owning device allocation (fp32 / int32 elements), grow-only resize so steady-state steps allocate nothing.
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // returns true when a new allocation was made (contents undefined then; `cap` elements, possibly more than n).
  // The FIRST allocation is exact (a fixed-shape workload pays for what it uses); a buffer that has to GROW takes half as much again:
  // the recipes sort their lists by length (train_ctc_parallel.sh:84-89), so T grows from minibatch to minibatch through a whole
  // epoch, and exact growth meant a hipFree -- which drains the device -- and a hipMalloc of every activation buffer on EVERY
  // minibatch (round 5, measured through the trainer binaries: 331 k padded frames/s end to end where the same loop on warm buffers
  // does 1.1 M).
  bool reserve(size_t n) {
    if (n <= cap) return false;
    // The margin is bounded (round 6): at most 1 GiB per buffer, and none when the device could not hold the margin twice
    // over -- a near-capacity shape that fits with exact sizing must not fail because EARLIER buffers kept slack.  Peak footprint on a
    // length-sorted list: the exact footprint of the longest minibatch + at most min(50 %, 1 GiB) per buffer.
    size_t want = cap ? std::max(n, cap + cap / 2) : n;
    if (want > n) {
      want = std::min(want, n + ((size_t)1 << 30) / sizeof(T));
      size_t fr = 0, tot = 0;
      if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); want = n; }
      else if (fr + cap * sizeof(T) < n * sizeof(T) + 2 * (want - n) * sizeof(T)) want = n;
    }
    release();
    if (hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T)) == hipSuccess) { cap = want; return true; }
    p = nullptr;
    (void)hipGetLastError();
    EESEN_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)));   // (no room for the margin: exactly what is needed)
    cap = n;
    return true;
  }
};

// Owning HIP event, created on first use (without timing unless asked for).  Converts to hipEvent_t for hipStreamWaitEvent /
// hipEventElapsedTime.
struct DevEvent {
  hipEvent_t e = nullptr;
  bool timing = false;
  DevEvent() = default;
  explicit DevEvent(bool timing_) : timing(timing_) {}
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  DevEvent(DevEvent&& o) noexcept : e(o.e), timing(o.timing) { o.e = nullptr; }
  DevEvent& operator=(DevEvent&& o) noexcept {
    if (this != &o) { release(); e = o.e; timing = o.timing; o.e = nullptr; }
    return *this;
  }
  ~DevEvent() { release(); }
  void release() {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  hipEvent_t get() {
    if (!e) EESEN_HIP_CHECK(hipEventCreateWithFlags(&e, timing ? hipEventDefault : hipEventDisableTiming));
    return e;
  }
  operator hipEvent_t() { return get(); }
  void record(hipStream_t st) { EESEN_HIP_CHECK(hipEventRecord(get(), st)); }
  void wait() { if (e) EESEN_HIP_CHECK(hipEventSynchronize(e)); }             // host wait; never recorded: nothing to wait for
  bool query() const { return !e || hipEventQuery(e) == hipSuccess; }         // true once everything recorded so far has run
};

// Owning HIP stream.  Whoever holds one drains it in its own destructor body: members are released after that body.
struct DevStream {
  hipStream_t s = nullptr;
  DevStream() = default;
  DevStream(const DevStream&) = delete;
  DevStream& operator=(const DevStream&) = delete;
  ~DevStream() { if (s) (void)hipStreamDestroy(s); }
  operator hipStream_t() const { return s; }
};

// Owning pinned host allocation + the event of the device's last use of it.  The one wait rule of every staging slot:
//   p = reserve(bytes, grow_to)   waits for the outstanding use, grows when bytes > cap (to max(bytes, grow_to): each site keeps its
//                                 own margin), returns the host pointer;
//   ... fill / enqueue the copy on `st` ...
//   used(st)                      records the event behind the copy.
// A buffer whose reuse is ordered by something else (the feeder's slot events, a synchronous copy) never calls used(): reserve()
// then only owns and grows.
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  DevEvent ev;     // the device's last use
  bool busy = false;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap), ev(std::move(o.ev)), busy(o.busy) { o.p = nullptr; o.cap = 0; o.busy = false; }
  PinBuf& operator=(PinBuf&& o) noexcept {
    if (this != &o) { release(); p = o.p; cap = o.cap; ev = std::move(o.ev); busy = o.busy; o.p = nullptr; o.cap = 0; o.busy = false; }
    return *this;
  }
  ~PinBuf() { release(); }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  void wait() {
    if (busy) { ev.wait(); busy = false; }
  }
  void* reserve(size_t bytes, size_t grow_to = 0) {
    wait();
    if (bytes > cap) {
      if (p) EESEN_HIP_CHECK(hipHostFree(p));
      p = nullptr;
      cap = 0;
      const size_t want = std::max(bytes, grow_to);
      EESEN_HIP_CHECK(hipHostMalloc(&p, want, hipHostMallocDefault));
      cap = want;
    }
    return p;
  }
  template <class T> T* as() const { return static_cast<T*>(p); }
  void used(hipStream_t st) { ev.record(st); busy = true; }
};

// The device a handle is created on: there is one, and the index names it.
inline void require_device(int dev) {
  int n = 0;
  const hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    throw Error(EESEN_ERR_HIP, "no HIP device available: this library has no CPU fallback (hipGetDeviceCount: " +
                                   std::string(e == hipSuccess ? "0 devices" : hipGetErrorString(e)) + ")");
  EESEN_REQUIRE(dev >= 0 && dev < n, EESEN_ERR_INVALID, "device index out of range");
  EESEN_HIP_CHECK(hipSetDevice(dev));
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline long cdivl(long a, long b) { return (a + b - 1) / b; }

}  // namespace eesen

// stage.hpp — what every host-driven entry point of every handle family shares (host code only): the error check, the handle guard, the zeroing
// allocator, a device scratch buffer grown on demand, and one staged call — the caller's arrays through that buffer around one launch.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "stage_layout.hpp"

namespace crl {

void set_error(const std::string& msg);

#define CRL_HIP_CHECK(expr)                                                                                   \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess) {                                                                                   \
      crl::set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e) + " (" + __FILE__ + ":" +      \
                     std::to_string(__LINE__) + ")");                                                         \
      return 1;                                                                                               \
    }                                                                                                         \
  } while (0)

// first statement of an entry point that takes a handle; noun = "crl_ppo", "crl_dqn", "crl_ddpg" or "crl_a2c"
#define CRL_HANDLE_GUARD(h, noun)                                       \
  if (!(h)) { crl::set_error("null " noun " handle"); return 1; }      \
  CRL_HIP_CHECK(hipSetDevice((h)->device));

template <typename T>
inline int dalloc(T** p, size_t n, bool zero = true) {
  CRL_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(p), n * sizeof(T)));
  if (zero) CRL_HIP_CHECK(hipMemset(*p, 0, n * sizeof(T)));
  return 0;
}

// A device scratch buffer of a handle, grown on demand and never shrunk.
struct Scratch { void* p = nullptr; size_t bytes = 0; };
inline int scratch_reserve(Scratch& s, hipStream_t st, size_t want) {
  if (s.bytes >= want) return 0;
  // Work enqueued earlier on the handle's stream may still read the old buffer, so the stream is drained before it is freed. hipFree happens to
  // wait for the device today; nothing in its contract says it will keep doing so.
  CRL_HIP_CHECK(hipStreamSynchronize(st));
  if (s.p) CRL_HIP_CHECK(hipFree(s.p));
  s.p = nullptr; s.bytes = 0;
  CRL_HIP_CHECK(hipMalloc(&s.p, want));
  s.bytes = want;
  return 0;
}
inline void scratch_release(Scratch& s) {
  if (s.p) (void)hipFree(s.p);
  s = Scratch{};
}

// One staged call. Declare the sections in order, reserve the scratch once, then: put (host → section), the launch on at(), get (section → host,
// skipped for a null host pointer), finish (the one synchronise: host buffers are only borrowed for the call).
template <typename T> struct Section { int i; };
struct Staged {
  hipStream_t st;
  StageLayout lay;
  char* base = nullptr;
  explicit Staged(hipStream_t stream) : st(stream) {}
  template <typename T> Section<T> add(size_t count) { return {lay.add(sizeof(T), count)}; }
  int reserve(Scratch& s, size_t floor = 0) {
    if (lay.bad) { set_error("staged call: the sections do not fit the address space"); return 1; }
    if (scratch_reserve(s, st, lay.total < floor ? floor : lay.total)) return 1;
    base = static_cast<char*>(s.p);
    return 0;
  }
  template <typename T> T* at(Section<T> s) const { return reinterpret_cast<T*>(base + lay.off[s.i]); }
  template <typename T> int put(Section<T> s, const T* host) {
    CRL_HIP_CHECK(hipMemcpyAsync(base + lay.off[s.i], host, lay.bytes[s.i], hipMemcpyHostToDevice, st));
    return 0;
  }
  template <typename T> int get(Section<T> s, T* host) {
    if (host) CRL_HIP_CHECK(hipMemcpyAsync(host, base + lay.off[s.i], lay.bytes[s.i], hipMemcpyDeviceToHost, st));
    return 0;
  }
  int finish() {
    CRL_HIP_CHECK(hipStreamSynchronize(st));
    return 0;
  }
};

}  // namespace crl

// stateless.hpp -- how a call that takes `int device` instead of a context gets onto its device (host code only).  Such an entry
// writes, in this order: its argument rules (st_fail: they hold on a machine without a device too), st_clear(), st_open(), then its
// DevPool / StreamGuard, st_stage() for every array `mem` describes, and its work under ST_CK.
//   st_fail    records "<family>: <what>" in the calling thread's slot -- the text behind cilhip_last_error(NULL) -- and hands the status back
//   ST_CK      a HIP call that must succeed: "<family>: <call>: <hipGetErrorString>", CILHIP_ERR_HIP
//   st_open    device count, range test, hipSetDevice
//   st_stage   the device image of a caller's array: the caller's own pointer (CILHIP_MEM_DEVICE) or an uploaded copy the pool owns
//   st_now_ms  the host's steady clock in milliseconds: what the *_last_stats phase times are differences of
#pragma once

#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <type_traits>

#include "../../include/cilantro_hip/c_api.h"
#include "device_mem.hpp"

namespace cilhip {

// what the calling thread's last stateless call refused or failed on; empty: nothing
inline std::string& st_slot() { thread_local std::string slot; return slot; }
inline const char* stateless_last_error() { return st_slot().empty() ? "null context" : st_slot().c_str(); }
inline void st_clear() { st_slot().clear(); }

inline int st_fail(int status, const char* family, const char* what, const char* detail = nullptr) noexcept {
  try {
    std::string& s = st_slot();
    s = family; s += ": "; s += what;
    if (detail) { s += ": "; s += detail; }
  } catch (...) {}      // (out of host memory: the status still says what happened)
  return status;
}

// the text of an argument refusal that names no single rule (the rules are c_api.h's, by the entry)
constexpr const char* kBadArguments = "an argument breaks the entry's rules (a null array, a size beyond its limit, an unknown mode)";

#define ST_CK(family, call) do { const hipError_t st_e_ = (call); if (st_e_ != hipSuccess) return cilhip::st_fail(CILHIP_ERR_HIP, family, #call, hipGetErrorString(st_e_)); } while (0)

// CILHIP_OK with `device` current; CILHIP_ERR_NO_DEVICE: no usable device at all; `out_of_range`: there are devices, `device` is none
// of them (the status is the caller's: the k-means family answers CILHIP_ERR_INVALID); CILHIP_ERR_HIP: hipSetDevice itself failed
inline int st_open(const char* family, int device, int out_of_range = CILHIP_ERR_NO_DEVICE) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return st_fail(CILHIP_ERR_NO_DEVICE, family, "no such HIP device (the call runs on the device: there is no CPU path)");
  if (device < 0 || device >= ndev) return st_fail(out_of_range, family, "no such HIP device", "the device index is out of range");
  ST_CK(family, hipSetDevice(device));
  return CILHIP_OK;
}

// *out = n elements of T on the device holding src[0 .. n): src itself for CILHIP_MEM_DEVICE, otherwise a block of `pool` filled by
// an asynchronous copy on s (src must stay valid until s has run it).  T: float, F3, const F3 ...; n == 0 is the caller's business.
template <class T> hipError_t st_stage(DevPool& pool, hipStream_t s, int mem, const float* src, size_t n, T** out) {
  using U = typename std::remove_const<T>::type;
  if (mem == CILHIP_MEM_DEVICE) { *out = reinterpret_cast<T*>(const_cast<float*>(src)); return hipSuccess; }
  U* d = nullptr;
  const hipError_t e = pool.get(&d, n);
  *out = d;
  return e != hipSuccess ? e : hipMemcpyAsync(d, src, n * sizeof(U), hipMemcpyHostToDevice, s);
}

inline double st_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace cilhip

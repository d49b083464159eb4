// ransac_sampling.hpp -- the random samples of a RANSAC run (model_estimation/ransac_base.hpp:83-91), drawn on the host: both
// estimators (ransac.hip, ransac_transform.hip) draw from here.  Plain C++, no HIP: tests/cpp/test_ransac_sampling.cpp pins every
// index against a literal copy of the loop the two files used to carry.
// Under hipcc the same functions are callable from a kernel (robust_normals.hip draws its elemental starts per lane with them):
// integer arithmetic only, so host and device give the same indices; tests/cpp/test_mcd_sampling.cpp pins the host side against the
// numpy restatement the GPU tests compare the kernel's decisions with.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CILHIP_SAMPLING_HD __host__ __device__
#else
#define CILHIP_SAMPLING_HD
#endif

namespace cilhip {

CILHIP_SAMPLING_HD inline uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

CILHIP_SAMPLING_HD inline uint64_t bounded(uint64_t& s, uint64_t bound) {   // uniform in [0, bound) (128-bit multiply, bias < 2^-32)
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(splitmix64(s), bound);      // the high word of the same 64 x 64 product
#else
  return (uint64_t)(((unsigned __int128)splitmix64(s) * bound) >> 64);
#endif
}

// out[3 * it .. 3 * it + 3): the sample of iteration it -- sample_size (<= 3, <= n) distinct indices below n, the rest 0
CILHIP_SAMPLING_HD inline void draw_samples(uint64_t seed, size_t n, uint32_t sample_size, size_t max_iter, uint32_t* out) {
  uint64_t st = seed;
  for (size_t it = 0; it < max_iter; ++it) {
    uint32_t pick[3] = {0, 0, 0};
    for (uint32_t i = 0; i < sample_size; ++i) {
      uint32_t v = (uint32_t)bounded(st, n - i);   // i-th draw among the n-i indices not picked yet
      uint32_t srt[3];
      for (uint32_t a = 0; a < i; ++a) srt[a] = pick[a];
      for (uint32_t a = 0; a + 1 < i; ++a)
        if (srt[a] > srt[a + 1]) { const uint32_t t = srt[a]; srt[a] = srt[a + 1]; srt[a + 1] = t; }
      for (uint32_t a = 0; a < i; ++a) v += v >= srt[a] ? 1u : 0u;
      pick[i] = v;
    }
    for (int i = 0; i < 3; ++i) out[3 * it + i] = pick[i];
  }
}

// a caller's samples: every index an iteration uses (its first sample_size entries) is below n
inline bool samples_in_range(const uint32_t* samples, size_t n, uint32_t sample_size, size_t max_iter) {
  for (size_t i = 0; i < 3 * max_iter; ++i)
    if ((i % 3) < sample_size && samples[i] >= n) return false;
  return true;
}

}  // namespace cilhip

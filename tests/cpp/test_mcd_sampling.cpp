// tests/cpp/test_mcd_sampling.cpp -- the elemental starts of the robust normal estimation (csrc/robust_normals.hip draws them per lane with
// csrc/ransac_sampling.hpp's draw_samples), printed for tests/test_robust_normal_refs_cpu.py, which compares every
// line with the Python-integer sampler of tests/_robust_normal_refs.py:
//   <seed> <row> <trial> <m> <p0> <p1> <p2>
// over a few seeds, every list length 4..32, rows from 0 up to 2^32 - 17 and trials 0..63.  Host only.
#include <cstdint>
#include <cstdio>

#include "../../cilantro_amd/csrc/ransac_sampling.hpp"

int main() {
  const uint64_t seeds[] = {0ull, 1ull, 0x9E3779B97F4A7C15ull, 0xFFFFFFFFFFFFFFFFull, 20240607ull};
  const uint64_t rows[] = {0ull, 1ull, 255ull, 256ull, 65537ull, (1ull << 31) - 1, 1ull << 31, (1ull << 32) - 17};
  const int trials[] = {0, 1, 5, 63};
  for (const uint64_t seed : seeds)
    for (const uint64_t row : rows)
      for (const int trial : trials)
        for (size_t m = 4; m <= 32; ++m) {
          uint32_t pick[3];
          cilhip::draw_samples(seed ^ ((uint64_t)row << 8 | (uint64_t)trial), m, 3, 1, pick);
          std::printf("%llu %llu %d %zu %u %u %u\n", (unsigned long long)seed, (unsigned long long)row, trial, m, pick[0], pick[1], pick[2]);
        }
  return 0;
}

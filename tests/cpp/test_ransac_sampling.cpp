// Host-only check of cilantro_amd/csrc/ransac_sampling.hpp: the samples both RANSAC estimators draw when the caller passes none,
// and the range check of the samples a caller does pass.  The checker below (ref_*) is a literal copy of the loop the two
// estimator files carried before the header existed -- a fixture: it must never be edited to follow the header.  Nothing here is
// a tolerance: every index must agree, bit for bit.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../cilantro_amd/csrc/ransac_sampling.hpp"

static int g_fail = 0;
static std::string g_what;
#define CHECK(cond) do { if (!(cond)) { if (g_fail < 40) std::printf("FAIL line %d [%s]: %s\n", __LINE__, g_what.c_str(), #cond); ++g_fail; } } while (0)

// ---- the fixture ---------------------------------------------------------------------------------------------------
static inline uint64_t ref_splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static inline uint64_t ref_bounded(uint64_t& s, uint64_t bound) { return (uint64_t)(((unsigned __int128)ref_splitmix64(s) * bound) >> 64); }

static std::vector<uint32_t> ref_draw(uint64_t seed, size_t n, size_t max_iter) {
  const uint32_t sample_size = n < 3 ? (uint32_t)n : 3u;
  std::vector<uint32_t> hsamp;
  hsamp.resize(3 * max_iter);
  uint64_t st = seed;
  for (size_t it = 0; it < max_iter; ++it) {
    uint32_t pick[3] = {0, 0, 0};
    for (uint32_t i = 0; i < sample_size; ++i) {
      uint32_t v = (uint32_t)ref_bounded(st, n - i);   // i-th draw among the n-i indices not picked yet
      uint32_t srt[3];
      for (uint32_t a = 0; a < i; ++a) srt[a] = pick[a];
      for (uint32_t a = 0; a + 1 < i; ++a)
        if (srt[a] > srt[a + 1]) { const uint32_t t = srt[a]; srt[a] = srt[a + 1]; srt[a + 1] = t; }
      for (uint32_t a = 0; a < i; ++a) v += v >= srt[a] ? 1u : 0u;
      pick[i] = v;
    }
    for (int i = 0; i < 3; ++i) hsamp[3 * it + i] = pick[i];
  }
  return hsamp;
}
static bool ref_refuses(const uint32_t* samples, size_t n, size_t max_iter) {
  const uint32_t sample_size = n < 3 ? (uint32_t)n : 3u;
  for (size_t i = 0; i < 3 * max_iter; ++i)
    if ((i % 3) < sample_size && samples[i] >= n) return true;
  return false;
}

int main() {
  const size_t sizes[] = {1, 2, 3, 4, 5, 1000, 0xFFFFFFF0ull};
  const size_t iters[] = {1, 7, 128};
  std::vector<uint64_t> seeds;
  for (uint64_t s = 0; s < 256; ++s) seeds.push_back(s);
  for (int b = 8; b < 64; ++b) seeds.push_back((1ull << b) - (uint64_t)(b & 1));      // the upper bits of the state too
  seeds.push_back(~0ull);
  size_t drawn = 0, refused = 0, accepted = 0;
  for (size_t n : sizes)
    for (size_t max_iter : iters) {
      const uint32_t sample_size = n < 3 ? (uint32_t)n : 3u;
      for (uint64_t seed : seeds) {
        g_what = "n " + std::to_string(n) + " max_iter " + std::to_string(max_iter) + " seed " + std::to_string(seed);
        std::vector<uint32_t> got(3 * max_iter, 0xDEADBEEFu);
        cilhip::draw_samples(seed, n, sample_size, max_iter, got.data());
        CHECK(got == ref_draw(seed, n, max_iter));
        bool shape = true;
        for (size_t it = 0; it < max_iter; ++it) {
          const uint32_t* p = &got[3 * it];
          for (uint32_t i = 0; i < 3; ++i) {
            if (i >= sample_size) { shape = shape && p[i] == 0; continue; }
            shape = shape && p[i] < n;
            for (uint32_t j = 0; j < i; ++j) shape = shape && p[i] != p[j];
          }
        }
        CHECK(shape);
        drawn += 3 * max_iter;
        // the range check: what was drawn is accepted; one entry pushed to n or beyond is refused exactly when an iteration uses it
        CHECK(cilhip::samples_in_range(got.data(), n, sample_size, max_iter));
        uint64_t st = seed ^ 0xA5A5A5A5ull;
        for (int trial = 0; trial < 6; ++trial) {
          std::vector<uint32_t> bad = got;
          const size_t pos = (size_t)(ref_splitmix64(st) % (3 * max_iter));
          const uint64_t room = 0x100000000ull - (uint64_t)n;      // values n .. 2^32 - 1
          bad[pos] = (uint32_t)((uint64_t)n + (trial == 0 ? 0 : ref_splitmix64(st) % room));
          const bool in_use = (pos % 3) < sample_size;
          const bool ok = cilhip::samples_in_range(bad.data(), n, sample_size, max_iter);
          CHECK(ok == !in_use);
          CHECK(ok == !ref_refuses(bad.data(), n, max_iter));
          (ok ? accepted : refused) += 1;
        }
        // the largest index below n is fine wherever it stands
        std::vector<uint32_t> top = got;
        top[3 * (max_iter - 1)] = (uint32_t)(n - 1);
        CHECK(cilhip::samples_in_range(top.data(), n, sample_size, max_iter));
      }
    }
  // the generator itself, one step at a time
  uint64_t a = 12345, b = 12345;
  for (int i = 0; i < 1000; ++i) CHECK(cilhip::splitmix64(a) == ref_splitmix64(b) && a == b);
  for (int i = 0; i < 1000; ++i) { const uint64_t bound = (ref_splitmix64(b) >> (i % 64)) | 1ull; a = b; uint64_t c = b; CHECK(cilhip::bounded(a, bound) == ref_bounded(c, bound) && a == c); b = c; }
  CHECK(refused > 0 && accepted > 0);      // (n < 3 leaves unused slots: both outcomes were seen)
  std::printf("%zu indices compared, %zu arrays refused, %zu with a large value in an unused slot accepted\n", drawn, refused, accepted);
  if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

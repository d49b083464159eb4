// Host build of the rigid fit in cilantro_amd/csrc/solve.hpp (compiled with hipcc, runs without a GPU), for tests/test_rigid_refs_cpu.py:
// reads pair sets from a file -- uint32 count, then per set uint32 n, n x 3 f32 dst, n x 3 f32 src --, adds the 16 raw f64 moments pair
// by pair as one lane of k_tmodels does, calls kabsch_from_sums, rounds the twelve outputs to f32 and packs them col-major as
// ransac_transform.hip does; writes per set 16 f32 and one int32: 1 when kabsch_rotation_polar took the set's sigma, 0 when the fit
// fell to the SVD.
#include "../../cilantro_amd/csrc/solve.hpp"

#include <cstdint>
#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
  using namespace cilhip;
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t count = 0;
  if (std::fread(&count, 4, 1, f) != 1) return 2;
  for (uint32_t k = 0; k < count; ++k) {
    uint32_t n = 0;
    if (std::fread(&n, 4, 1, f) != 1) return 2;
    std::vector<float> d(3 * (size_t)n + 1), s(3 * (size_t)n + 1);
    if (n && (std::fread(d.data(), 4, 3 * (size_t)n, f) != 3 * (size_t)n || std::fread(s.data(), 4, 3 * (size_t)n, f) != 3 * (size_t)n)) return 2;
    double sums[16];
    for (int i = 0; i < 16; ++i) sums[i] = 0.0;
    for (uint32_t i = 0; i < n; ++i) {
      const double p[3] = {(double)d[3 * i], (double)d[3 * i + 1], (double)d[3 * i + 2]};
      const double q[3] = {(double)s[3 * i], (double)s[3 * i + 1], (double)s[3 * i + 2]};
      sums[0] += 1.0;
      for (int c = 0; c < 3; ++c) { sums[1 + c] += p[c]; sums[4 + c] += q[c]; }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sums[7 + r * 3 + c] += p[r] * q[c];
    }
    double L[9], t[3];
    kabsch_from_sums(sums, L, t);
    float T[16];
    for (int i = 0; i < 16; ++i) T[i] = 0.0f;
    T[15] = 1.0f;
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T[c * 4 + r] = (float)L[r * 3 + c]; T[12 + r] = (float)t[r]; }
    int32_t polar = 0;
    if (n > 0) {      // the sigma kabsch_from_sums forms
      double mud[3], mus[3], sig[9], R[9];
      for (int c = 0; c < 3; ++c) { mud[c] = sums[1 + c] / sums[0]; mus[c] = sums[4 + c] / sums[0]; }
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) sig[r * 3 + c] = sums[7 + r * 3 + c] / sums[0] - mud[r] * mus[c];
      polar = kabsch_rotation_polar(sig, R) ? 1 : 0;
    }
    std::fwrite(T, 4, 16, stdout);
    std::fwrite(&polar, 4, 1, stdout);
  }
  std::fclose(f);
  return 0;
}

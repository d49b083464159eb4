// test_mean_shift_nd_host.cpp -- csrc/mean_shift_nd_host.hpp on its own: no HIP, no library call.  Every refusal of cilhip_mean_shift_nd in
// the order the entry applies them, the call without a seed, and the slice plan of rule M3: the slices cover
// [0, n) exactly once and in order, the plan is a function of (n, n_active) alone, and the partial sums stay within their bound.
// tests/test_meanshift_nd_refs_cpu.py builds it twice (plainly, and under ASan / UBSan) and runs both; prints "host OK".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cilantro_amd/csrc/mean_shift_nd_host.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool says(const cilhip::NdVerdict& v, int status, const char* needle) { return v.status == status && v.what && std::strstr(v.what, needle); }

int main() {
  using namespace cilhip;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> pts(5 * 16, 1.0f), shifted(5 * 16, 7.0f);
  std::vector<uint32_t> labels(5, 7u);
  size_t nc = 77, it = 77;
  cilhip_ms_params prm{};
  prm.kernel_radius = 1.0f; prm.max_iter = 5; prm.cluster_tol = 0.1f; prm.convergence_tol = 1e-4f; prm.kernel_kind = 0; prm.kernel_sigma = 1.0f; prm.form = 0;
  const MsnCall good{pts.data(), 5, 16, nullptr, 0, 0, &prm, shifted.data(), labels.data(), &nc, &it};
  const size_t big = (size_t)ND_MAX_COUNT;

  // the rules
  CHECK(msn_check(good).status == 0);
  { MsnCall c = good; c.dim = 1; c.mem = 1; c.seeds = pts.data(); c.n_seeds = 3; CHECK(msn_check(c).status == 0); }
  { MsnCall c = good; c.points = nullptr; c.n = 0; c.seeds = pts.data(); c.n_seeds = 2; CHECK(msn_check(c).status == 0); }      // no points, with seeds: legal
  { MsnCall c = good; c.points = nullptr; c.n = 0; c.shifted_out = nullptr; c.labels_out = nullptr; CHECK(msn_check(c).status == 0); }      // no seed at all: no outputs needed
  { MsnCall c = good; c.n = big - 1; CHECK(msn_check(c).status == 0); }
  { MsnCall c = good; c.params = nullptr; CHECK(says(msn_check(c), -1, "params is null")); }
  { MsnCall c = good; c.n_clusters_out = nullptr; CHECK(says(msn_check(c), -1, "n_clusters_out is null")); }
  { MsnCall c = good; c.iterations_out = nullptr; CHECK(says(msn_check(c), -1, "iterations_out is null")); }
  { MsnCall c = good; c.dim = 0; CHECK(says(msn_check(c), -1, "dim is 0")); }
  { MsnCall c = good; c.n = big; CHECK(says(msn_check(c), -1, "n must be below 2^32 - 16")); }
  { MsnCall c = good; c.seeds = pts.data(); c.n_seeds = big; CHECK(says(msn_check(c), -1, "n_seeds must be below 2^32 - 16")); }
  { MsnCall c = good; c.mem = 2; CHECK(says(msn_check(c), -1, "mem")); }
  { MsnCall c = good; c.mem = -1; CHECK(says(msn_check(c), -1, "mem")); }
  { MsnCall c = good; c.points = nullptr; CHECK(says(msn_check(c), -1, "points is null")); }
  { MsnCall c = good; c.n_seeds = 3; CHECK(says(msn_check(c), -1, "seed array")); }
  { MsnCall c = good; c.shifted_out = nullptr; CHECK(says(msn_check(c), -1, "shifted_seeds_out is null")); }
  { MsnCall c = good; c.labels_out = nullptr; CHECK(says(msn_check(c), -1, "labels_out is null")); }
  { MsnCall c = good; c.dim = 17; CHECK(says(msn_check(c), -3, "dim > 16")); }
  { MsnCall c = good; c.dim = 17; c.points = nullptr; CHECK(says(msn_check(c), -1, "points is null")); }      // an invalid argument is named before the unsupported one
  struct Field { float cilhip_ms_params::*f; const char* word; };
  for (const Field& fd : {Field{&cilhip_ms_params::kernel_radius, "kernel_radius"}, Field{&cilhip_ms_params::cluster_tol, "cluster_tol"},
                          Field{&cilhip_ms_params::convergence_tol, "convergence_tol"}})
    for (const float bad : {nan, inf, -1.0f, -inf}) {
      cilhip_ms_params p = prm;
      p.*(fd.f) = bad;
      MsnCall c = good; c.params = &p;
      CHECK(says(msn_check(c), -1, fd.word));
      p.*(fd.f) = 0.0f;
      CHECK(msn_check(c).status == 0);      // zero is a value
    }
  for (const float bad : {nan, inf, 0.0f, -1.0f}) {
    cilhip_ms_params p = prm;
    p.kernel_sigma = bad;
    MsnCall c = good; c.params = &p;
    CHECK(msn_check(c).status == 0);      // a sigma is only looked at with the RBF kernel
    p.kernel_kind = 2;
    CHECK(says(msn_check(c), -1, "kernel_sigma"));
  }
  for (const int bad : {-1, 3}) { cilhip_ms_params p = prm; p.kernel_kind = bad; MsnCall c = good; c.params = &p; CHECK(says(msn_check(c), -1, "kernel_kind")); }
  for (const int bad : {-1, 1, 2, 3}) { cilhip_ms_params p = prm; p.form = bad; MsnCall c = good; c.params = &p; CHECK(says(msn_check(c), -1, "form must be 0")); }
  CHECK(shifted[0] == 7.0f && labels[0] == 7u && nc == 77 && it == 77);      // a check writes nothing

  {      // no seed at all
    uint32_t off[2] = {7u, 7u};
    msn_answer_empty(CILHIP_MEM_HOST, off, &nc, &it);
    CHECK(nc == 0 && it == 0 && off[0] == 0 && off[1] == 7u);
    nc = it = 77; off[0] = 7u;
    msn_answer_empty(CILHIP_MEM_DEVICE, off, &nc, &it);      // a device array is not the host's to write
    CHECK(nc == 0 && it == 0 && off[0] == 7u);
    msn_answer_empty(CILHIP_MEM_HOST, nullptr, &nc, &it);
  }

  // the slice plan
  const size_t ns_list[] = {0u, 1u, 3u, 4u, 5u, 511u, 512u, 513u, 4097u, 1000000u, 4294967279u};
  const size_t act_list[] = {1u, 255u, 256u, 257u, 100000u};
  for (const size_t n : ns_list)
    for (const size_t act : act_list) {
      const size_t s = msn_slices(n, act), len = msn_slice_length(n, s);
      CHECK(s >= 1 && s <= MSN_MAX_SLICES && len % MSN_TILE == 0 && len <= 0xFFFFFFFFull);
      CHECK(s == 1 || (n / s >= MSN_MIN_SLICE && s * act * MSN_PART_ROW_BYTES <= MSN_PART_BYTES));      // no short slice, the partial sums within their bound
      // slice y is [min(y len, n), min((y + 1) len, n)): one after the other from 0 to n
      size_t at = 0;
      for (size_t y = 0; y < s; ++y) {
        const unsigned long long first = (unsigned long long)y * len, lo = first < n ? first : n, hi = first + len < n ? first + len : n;
        CHECK(lo == at && hi >= lo);
        at = (size_t)hi;
      }
      CHECK(at == n);
      CHECK(msn_slices(n, act) == s && msn_slice_length(n, s) == len);      // a function of its arguments alone
      for (const size_t dim : {1u, 3u, 16u}) {
        CHECK(msn_part_doubles(n, act, dim) >= s * act * (dim + 1));      // the room of a whole run holds its first pass ...
        CHECK(msn_part_doubles(n, act, dim) >= msn_slices(n, 1) * (dim + 1) && msn_part_doubles(n, act, dim) >= msn_slices(n, (act + 1) / 2) * ((act + 1) / 2) * (dim + 1));      // ... and later ones
        CHECK(msn_part_doubles(n, act, dim) * sizeof(double) <= (MSN_PART_BYTES > act * MSN_PART_ROW_BYTES ? MSN_PART_BYTES : act * MSN_PART_ROW_BYTES));
      }
    }
  CHECK(msn_slices(4097, 41) == 8 && msn_slices(1u << 20, 1) == 256 && msn_slices(1u << 20, 10000) == 26 && msn_slices(100000, 100000) == 3);
  CHECK(msn_slices(1023, 41) == 1 && msn_slices(1024, 41) == 2 && msn_slices(1025, 256) == 2 && msn_slices(1025, 257) == 2);
  CHECK(msn_slices(1u << 20, 100000) == 3 && msn_slices(1u << 30, 400000) == 1 && msn_slices(1u << 30, 200000) == 2);      // 64 MiB / 136 bytes = 493447 rows
  CHECK(msn_slices(5, 0) == 1 && msn_slices(0, 0) == 1);

  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("host OK\n");
  return 0;
}

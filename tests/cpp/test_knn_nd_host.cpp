// test_knn_nd_host.cpp -- csrc/knn_nd_host.hpp on its own: no HIP, no library call.  The argument rules N4 of DESIGN.md section 21 in the
// order the entries apply them, the rows and offsets of a call that needs no device, and the capacity protocol's decision.
// tests/test_knn_nd_refs_cpu.py builds it twice (plainly, and under ASan / UBSan) and runs both; prints "host OK".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cilantro_amd/csrc/knn_nd_host.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool says(const cilhip::NdVerdict& v, int status, const char* needle) { return v.status == status && v.what && std::strstr(v.what, needle); }

int main() {
  using namespace cilhip;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> ref(5 * 16, 1.0f);
  std::vector<uint32_t> idx(64, 7u);
  std::vector<uint64_t> off(8, 7u);
  const size_t big = (size_t)ND_MAX_COUNT;

  // k-NN rules
  CHECK(nd_check_knn(ref.data(), 5, 3, 16, 0, 32, inf, idx.data()).status == 0);
  CHECK(nd_check_knn(ref.data(), 5, 3, 1, 1, 1, 0.5f, idx.data()).status == 0);
  CHECK(nd_check_knn(nullptr, 0, 3, 4, 0, 3, inf, idx.data()).status == 0);      // no points: a NULL ref is fine
  CHECK(nd_check_knn(ref.data(), 5, 3, 4, 0, 40, -1.0f, idx.data()).status == -3);      // (a negative bound is a trivial call, not a refusal)
  CHECK(says(nd_check_knn(nullptr, 5, 3, 4, 0, 3, inf, idx.data()), -1, "ref is NULL"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 4, 0, 3, inf, nullptr), -1, "idx_out is NULL"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 0, 0, 3, inf, idx.data()), -1, "dim is 0"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 4, 0, 0, inf, idx.data()), -1, "k is 0"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 4, 0, 3, nan, idx.data()), -1, "max_sq_dist is NaN"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 4, 2, 3, inf, idx.data()), -1, "mem"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 4, -1, 3, inf, idx.data()), -1, "mem"));
  CHECK(says(nd_check_knn(ref.data(), big, 3, 4, 0, 3, inf, idx.data()), -1, "2^32 - 16"));
  CHECK(says(nd_check_knn(ref.data(), 5, big, 4, 0, 3, inf, idx.data()), -1, "2^32 - 16"));
  CHECK(nd_check_knn(ref.data(), big - 1, big - 1, 4, 0, 3, inf, idx.data()).status == 0);
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 17, 0, 3, inf, idx.data()), -3, "dim > 16"));
  CHECK(says(nd_check_knn(ref.data(), 5, 3, 16, 0, 33, inf, idx.data()), -3, "k > 32"));

  // radius rules
  CHECK(nd_check_radius(ref.data(), 5, 3, 16, 0, 1.0f, off.data()).status == 0);
  CHECK(nd_check_radius(ref.data(), 5, 3, 16, 0, -1.0f, off.data()).status == 0);
  CHECK(says(nd_check_radius(ref.data(), 5, 3, 4, 0, 1.0f, nullptr), -1, "offsets_out is NULL"));
  CHECK(says(nd_check_radius(ref.data(), 5, 3, 4, 0, inf, off.data()), -1, "not finite"));
  CHECK(says(nd_check_radius(ref.data(), 5, 3, 4, 0, nan, off.data()), -1, "not finite"));
  CHECK(says(nd_check_radius(nullptr, 5, 3, 4, 0, 1.0f, off.data()), -1, "ref is NULL"));
  CHECK(says(nd_check_radius(ref.data(), 5, 3, 0, 0, 1.0f, off.data()), -1, "dim is 0"));
  CHECK(says(nd_check_radius(ref.data(), 5, 3, 4, 7, 1.0f, off.data()), -1, "mem"));
  CHECK(says(nd_check_radius(ref.data(), 5, 3, 17, 0, 1.0f, off.data()), -3, "dim > 16"));

  // calls that need no device
  CHECK(nd_knn_trivial(0, 3, inf) && nd_knn_trivial(5, 0, inf) && nd_knn_trivial(5, 3, 0.0f) && nd_knn_trivial(5, 3, -0.0f) && nd_knn_trivial(5, 3, -inf));
  CHECK(!nd_knn_trivial(5, 3, inf) && !nd_knn_trivial(5, 3, std::numeric_limits<float>::denorm_min()));
  CHECK(nd_radius_trivial(0, 3, 1.0f) && nd_radius_trivial(5, 0, 1.0f) && nd_radius_trivial(5, 3, 0.0f) && nd_radius_trivial(5, 3, -2.0f) && !nd_radius_trivial(5, 3, 1e-30f));

  {      // rows: exactly n_query * k entries, every optional array optional
    std::vector<uint32_t> rows(3 * 4 + 1, 7u), cnt(3 + 1, 7u);
    std::vector<float> d2(3 * 4 + 1, 7.0f);
    nd_pad_rows(3, 4, rows.data(), d2.data(), cnt.data());
    for (size_t i = 0; i < 12; ++i) CHECK(rows[i] == ND_NONE && d2[i] == inf);
    for (size_t i = 0; i < 3; ++i) CHECK(cnt[i] == 0);
    CHECK(rows[12] == 7u && d2[12] == 7.0f && cnt[3] == 7u);
    std::vector<uint32_t> only(2 * 5, 7u);
    nd_pad_rows(2, 5, only.data(), nullptr, nullptr);
    for (const uint32_t v : only) CHECK(v == ND_NONE);
    nd_pad_rows(0, 5, nullptr, nullptr, nullptr);      // nothing is touched
  }
  {
    std::vector<uint64_t> o(5, 7u);
    size_t total = 9;
    nd_empty_offsets(3, o.data(), &total);
    CHECK(o[0] == 0 && o[1] == 0 && o[2] == 0 && o[3] == 0 && o[4] == 7u && total == 0);
    nd_empty_offsets(0, o.data() + 4, nullptr);
    CHECK(o[4] == 0);
  }

  // the capacity protocol
  CHECK(nd_radius_plan(nullptr, 100, 10) == 0);
  CHECK(nd_radius_plan(idx.data(), 0, 10) == 0);
  CHECK(nd_radius_plan(idx.data(), 9, 10) == 0);
  CHECK(nd_radius_plan(idx.data(), 10, 10) == 1);
  CHECK(nd_radius_plan(idx.data(), 11, 10) == 1);
  CHECK(nd_radius_plan(idx.data(), 10, 0) == 0);
  CHECK(nd_radius_plan(idx.data(), (size_t)-1, ND_MAX_COUNT) == 1);
  CHECK(nd_radius_plan(idx.data(), (size_t)-1, ND_MAX_COUNT + 1) == -3);
  CHECK(nd_radius_plan(idx.data(), 5, ND_MAX_COUNT + 1) == 0);      // (no room: the caller learns the total first)

  // the slices of a k-NN call
  CHECK(nd_slices(100000, 300000, 10) == 1);                 // the queries fill the device
  CHECK(nd_slices(1023, 300, 10) == 1 && nd_slices(1024, 300, 10) == 2 && nd_slices(1500, 300, 10) == 2);      // no slice below 512 points
  CHECK(nd_slices(100000, 100000, 10) == 3 && nd_slices(15531, 15531, 10) == 17 && nd_slices(15531, 15531, 30) == 17);
  CHECK(nd_slices(1u << 20, 256, 1) == 32);                  // at most 32
  CHECK(nd_slices(1u << 20, 200000, 32) == 1 && nd_slices(1u << 20, 50000, 32) == 5);      // at most 64 MiB of partial lists
  CHECK(nd_slices(0, 0, 0) == 1 && nd_slices(5, 0, 3) == 1 && nd_slices(0, 5, 3) == 1);
  for (const size_t n : {1u, 3u, 4u, 5u, 1024u, 1025u, 15531u, 4294967279u})
    for (const size_t s : {1u, 2u, 17u, 32u}) {
      const size_t len = nd_slice_length(n, s, 4);
      CHECK(len % 4 == 0 && len * s >= n && len < n / s + 8 && len <= 0xFFFFFFFFull);
    }

  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("host OK\n");
  return 0;
}

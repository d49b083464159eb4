// test_components_nd_host.cpp -- csrc/components_nd_host.hpp on its own: no HIP, no library call.  Every refusal of
// cilhip_connected_components_nd in the order the entry applies them, the call without a point, the form choice, the order-preserving key,
// the sweep axis, R for 10 000 random and edge radii (fl(R * R) >= radius_sq and fl(prev(R)^2) < radius_sq), the prune rule on random tiles
// (no skipped tile pair holds an edge, the bisection equals the literal scan), the full and pruned plans, and the cut into launches
// (DESIGN.md section 23).  tests/test_ccn_refs_cpu.py builds it twice (plainly, and under ASan / UBSan) and runs both; prints "host OK".
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../cilantro_amd/csrc/components_nd_host.hpp"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static bool says(const cilhip::NdVerdict& v, int status, const char* needle) { return v.status == status && v.what && std::strstr(v.what, needle); }

static uint64_t lcg_state = 0x9E3779B97F4A7C15ull;
static uint32_t lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(lcg_state >> 32); }
static float unit() { return (float)(lcg() >> 8) * (1.0f / 16777216.0f); }
static float from_bits(uint32_t u) { float v; std::memcpy(&v, &u, 4); return v; }
static uint32_t to_bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

int main() {
  using namespace cilhip;
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float fmax = std::numeric_limits<float>::max(), denorm = std::numeric_limits<float>::denorm_min();
  std::vector<float> pts(5 * 16, 1.0f);
  std::vector<uint32_t> labels(5, 7u), seeds = {0u, 4u};
  size_t nseg = 77;
  cilhip_cc_params prm{};
  prm.radius_sq = 1.0f; prm.min_segment_size = 1; prm.max_segment_size = (size_t)-1;
  const CcnCall good{pts.data(), nullptr, nullptr, 5, 16, 0, &prm, 0, nullptr, 0, labels.data(), &nseg};
  const size_t big = (size_t)ND_MAX_COUNT;

  // ---- the rules ----
  CHECK(ccn_check(good).status == 0);
  { CcnCall c = good; c.dim = 1; c.mem = 1; c.form = 2; c.seeds = seeds.data(); c.n_seeds = 2; CHECK(ccn_check(c).status == 0); }
  { CcnCall c = good; c.form = 1; c.seeds = seeds.data(); c.n_seeds = 0; CHECK(ccn_check(c).status == 0); }      // an empty seed list is a list
  { CcnCall c = good; c.points = nullptr; c.n = 0; c.labels_out = nullptr; CHECK(ccn_check(c).status == 0); }      // no point: no arrays needed
  { CcnCall c = good; c.n = big - 1; CHECK(ccn_check(c).status == 0); }
  { CcnCall c = good; c.params = nullptr; CHECK(says(ccn_check(c), -1, "params is null")); }
  { CcnCall c = good; c.n_segments_out = nullptr; CHECK(says(ccn_check(c), -1, "n_segments_out is null")); }
  { CcnCall c = good; c.dim = 0; CHECK(says(ccn_check(c), -1, "dim is 0")); }
  for (const int bad : {-1, 3, 100}) { CcnCall c = good; c.form = bad; CHECK(says(ccn_check(c), -1, "form")); }
  { CcnCall c = good; c.n = big; CHECK(says(ccn_check(c), -1, "n must be below 2^32 - 16")); }
  for (const int bad : {-1, 2}) { CcnCall c = good; c.mem = bad; CHECK(says(ccn_check(c), -1, "mem")); }
  { CcnCall c = good; c.labels_out = nullptr; CHECK(says(ccn_check(c), -1, "labels_out is null")); }
  { CcnCall c = good; c.n_seeds = 2; CHECK(says(ccn_check(c), -1, "seed array")); }
  { CcnCall c = good; std::vector<uint32_t> s = {0u, 5u}; c.seeds = s.data(); c.n_seeds = 2; CHECK(says(ccn_check(c), -1, "seed index")); }
  for (const float bad : {nan, inf, -inf}) { cilhip_cc_params p = prm; p.radius_sq = bad; CcnCall c = good; c.params = &p; CHECK(says(ccn_check(c), -1, "radius_sq")); }
  for (const float fine : {0.0f, -1.0f, fmax, denorm}) { cilhip_cc_params p = prm; p.radius_sq = fine; CcnCall c = good; c.params = &p; CHECK(ccn_check(c).status == 0); }
  { cilhip_cc_params p = prm; p.use_normals = 1; CcnCall c = good; c.params = &p; CHECK(says(ccn_check(c), -1, "normals clause")); c.normals = pts.data(); CHECK(ccn_check(c).status == 0); }
  { cilhip_cc_params p = prm; p.use_colors = 1; CcnCall c = good; c.params = &p; CHECK(says(ccn_check(c), -1, "colours clause")); c.rgb = pts.data(); CHECK(ccn_check(c).status == 0); }
  { CcnCall c = good; c.points = nullptr; CHECK(says(ccn_check(c), -1, "points is null")); }
  { CcnCall c = good; c.dim = 17; CHECK(says(ccn_check(c), -3, "dim > 16")); }
  { CcnCall c = good; c.dim = 17; c.points = nullptr; CHECK(says(ccn_check(c), -1, "points is null")); }      // an invalid argument is named before the unsupported one
  CHECK(labels[0] == 7u && nseg == 77);      // a check writes nothing

  {      // no point at all
    uint32_t off[2] = {7u, 7u};
    ccn_answer_empty(CILHIP_MEM_HOST, off, &nseg);
    CHECK(nseg == 0 && off[0] == 0 && off[1] == 7u);
    nseg = 77; off[0] = 7u;
    ccn_answer_empty(CILHIP_MEM_DEVICE, off, &nseg);      // a device array is not the host's to write
    CHECK(nseg == 0 && off[0] == 7u);
    ccn_answer_empty(CILHIP_MEM_HOST, nullptr, &nseg);
  }

  // ---- the form: the sort is taken from the measured crossover up ----
  CHECK(ccn_form(1, 1u << 20) == 1 && ccn_form(2, 1) == 2 && ccn_form(0, 1) == 1 && ccn_form(0, CCN_FORM2_MIN_POINTS - 1) == 1 && ccn_form(0, CCN_FORM2_MIN_POINTS) == 2);
  CHECK(CCN_FORM2_MIN_POINTS > CCN_TILE && ccn_form(0, big - 1) == 2);
  CHECK(ccn_tiles(0) == 0 && ccn_tiles(1) == 1 && ccn_tiles(CCN_TILE) == 1 && ccn_tiles(CCN_TILE + 1) == 2 && ccn_tiles(big - 1) == (big - 1 + CCN_TILE - 1) / CCN_TILE);

  // ---- keys ----
  {
    const float ladder[] = {-inf, -fmax, -1.0f, -denorm, -0.0f, 0.0f, denorm, 1.0f, fmax, inf};
    for (size_t k = 0; k + 1 < sizeof(ladder) / sizeof(ladder[0]); ++k) CHECK(ccn_key(ladder[k]) < ccn_key(ladder[k + 1]));
    for (const float v : ladder) CHECK(to_bits(ccn_unkey(ccn_key(v))) == to_bits(v) && ccn_key(v) < CCN_KEY_DROPPED);
    for (int k = 0; k < 100000; ++k) {
      const float a = from_bits(lcg()), b = from_bits(lcg());
      if (a != a || b != b) continue;
      CHECK((a < b) ? ccn_key(a) < ccn_key(b) : (a > b ? ccn_key(a) > ccn_key(b) : true));
      CHECK(to_bits(ccn_unkey(ccn_key(a))) == to_bits(a));
    }
  }

  // ---- the sweep axis: largest extent, lowest axis on ties, no overflow ----
  {
    const float lo[4] = {0.0f, -1.0f, 5.0f, -fmax}, hi[4] = {1.0f, 1.0f, 7.0f, fmax};
    uint32_t kl[4], kh[4];
    for (int a = 0; a < 4; ++a) { kl[a] = ccn_key(lo[a]); kh[a] = ccn_key(hi[a]); }
    CHECK(ccn_pick_axis(kl, kh, 1) == 0 && ccn_pick_axis(kl, kh, 2) == 1 && ccn_pick_axis(kl, kh, 3) == 1 && ccn_pick_axis(kl, kh, 4) == 3);
    const uint32_t same[3] = {ccn_key(2.0f), ccn_key(2.0f), ccn_key(2.0f)};
    CHECK(ccn_pick_axis(same, same, 3) == 0);      // one point: every extent is 0
  }

  // ---- R ----
  {
    std::vector<float> radii = {denorm, 2 * denorm, 3 * denorm, std::numeric_limits<float>::min(), 1e-30f, 1.0f, 2.0f, 0.32f, 4.0f, 1e30f, fmax, std::nextafterf(fmax, 0.0f),
                                std::nextafterf(1.0f, 2.0f), std::nextafterf(1.0f, 0.0f)};
    while (radii.size() < 10000) {
      const uint32_t bits = lcg() & 0x7FFFFFFFu;      // every exponent, subnormals among them
      const float v = from_bits(bits);
      if (v > 0.0f && v <= fmax) radii.push_back(v);
    }
    for (const float r2 : radii) {
      const float R = ccn_prune_radius(r2);
      CHECK(R > 0.0f && R <= fmax && ccn_sq(R) >= r2);
      CHECK(ccn_sq(std::nextafterf(R, 0.0f)) < r2);      // the smallest such float
    }
    CHECK(ccn_prune_radius(4.0f) == 2.0f && ccn_prune_radius(1.0f) == 1.0f && ccn_prune_radius(std::nextafterf(4.0f, 5.0f)) == std::nextafterf(2.0f, 3.0f));
    CHECK(ccn_prune_radius(denorm) > 0.0f && ccn_sq(ccn_prune_radius(fmax)) >= fmax);
  }

  // ---- the prune rule and the pruned plan on random sorted streams ----
  for (int round = 0; round < 40; ++round) {
    const size_t tile = 8;      // (the rule does not know the tile size: small tiles make many of them)
    const size_t m = 1 + lcg() % 200, tiles = (m + tile - 1) / tile;
    const float r2 = 0.0005f + unit() * (round % 2 ? 0.02f : 2.0f), R = ccn_prune_radius(r2);
    std::vector<float> x(m), y(m);
    for (size_t k = 0; k < m; ++k) { x[k] = (unit() - 0.5f) * 4.0f + (k % 3 == 0 ? 3.0f : 0.0f); y[k] = unit() * 0.01f; }
    std::vector<size_t> order(m);
    for (size_t k = 0; k < m; ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return ccn_key(x[a]) < ccn_key(x[b]); });
    std::vector<float> tmin(tiles), tmax(tiles);
    for (size_t t = 0; t < tiles; ++t) { tmin[t] = x[order[t * tile]]; tmax[t] = x[order[std::min((t + 1) * tile, m) - 1]]; }
    const CcnPlan plan = ccn_plan_pruned(tmin.data(), tmax.data(), tiles, R);
    CHECK(plan.first.size() == tiles && plan.begin.size() == tiles + 1 && plan.total == (unsigned long long)tiles * (tiles + 1) / 2 && plan.tested <= plan.total && plan.begin[0] == 0);
    unsigned long long at = 0;
    for (size_t I = 0; I < tiles; ++I) {
      size_t scan = 0;      // the literal rule
      while (scan < I && ccn_skips(tmin[I], tmax[scan], R)) ++scan;
      CHECK(plan.first[I] == scan && plan.first[I] <= I && plan.begin[I] == at);
      at += I - scan + 1;
      for (size_t J = 0; J < plan.first[I]; ++J)      // no skipped tile pair holds an edge (two axes: d2 = (0 + sx) + sy as N1 adds them)
        for (size_t a = I * tile; a < std::min((I + 1) * tile, m); ++a)
          for (size_t b = J * tile; b < std::min((J + 1) * tile, m); ++b) {
            volatile float tx = x[order[a]] - x[order[b]], ty = y[order[a]] - y[order[b]];
            volatile float sx = tx * tx, sy = ty * ty;
            volatile float d2 = sx + sy;
            CHECK(!(d2 < r2));
          }
    }
    CHECK(plan.begin[tiles] == at && plan.tested == at);
  }
  {      // tiles far apart: only the diagonal; everything within R: the whole triangle; equal coordinates (and -0 / +0) are never skipped
    const float mn[4] = {0.0f, 10.0f, 20.0f, 30.0f}, mx[4] = {1.0f, 11.0f, 21.0f, 31.0f};
    CHECK(ccn_plan_pruned(mn, mx, 4, 2.0f).tested == 4 && ccn_plan_pruned(mn, mx, 4, 100.0f).tested == 10 && ccn_plan_pruned(mn, mx, 4, 9.0f).tested == 4);
    CHECK(ccn_plan_pruned(mn, mx, 4, std::nextafterf(9.0f, 10.0f)).tested == 7);      // strictly: a gap of exactly R is skipped, a hair less is not
    const float z0[3] = {-0.0f, 0.0f, 0.0f}, z1[3] = {-0.0f, 0.0f, 0.0f};
    CHECK(ccn_plan_pruned(z0, z1, 3, denorm).tested == 6);
    CHECK(ccn_skips(fmax, -fmax, fmax) && !ccn_skips(1.0f, 1.0f, denorm));      // an overflowing difference is +inf: skipped, and rightly (d2 = +inf)
    CHECK(ccn_plan_pruned(nullptr, nullptr, 0, 1.0f).tested == 0 && ccn_plan_full(0).tested == 0);
  }
  for (const size_t tiles : {1u, 2u, 3u, 17u, 4096u}) {
    const CcnPlan full = ccn_plan_full(tiles);
    CHECK(full.total == full.tested && full.tested == (unsigned long long)tiles * (tiles + 1) / 2 && full.first.size() == tiles && full.begin.size() == tiles + 1);
    for (size_t I = 0; I < tiles; ++I) CHECK(full.first[I] == 0 && full.begin[I + 1] - full.begin[I] == I + 1);
  }

  // ---- the launches: the cap holds, the launches cover the list once and in order ----
  CHECK(CCN_MAX_PAIRS_PER_LAUNCH <= (unsigned long long)(0.25 * 4.1e11) && CCN_MAX_PAIRS_PER_LAUNCH <= (unsigned long long)(0.25 * 3.1e11));      // a quarter of a second at the slowest measured pair rates
  CHECK(ccn_tile_pairs_per_launch(0) == CCN_MAX_PAIRS_PER_LAUNCH / (CCN_TILE * CCN_TILE) && ccn_tile_pairs_per_launch(0) * CCN_TILE * CCN_TILE <= CCN_MAX_PAIRS_PER_LAUNCH);
  CHECK(ccn_tile_pairs_per_launch(1) == 1 && ccn_tile_pairs_per_launch(CCN_TILE * CCN_TILE * 3 + 5) == 3 && ccn_tile_pairs_per_launch(~0ull) == 0x7FFFFFFFull);
  for (const unsigned long long tested : {0ull, 1ull, 2ull, 7ull, 1000ull, 1ull << 40})
    for (const unsigned long long per : {1ull, 3ull, 1000ull, 915527ull}) {
      const unsigned long long launches = ccn_launches(tested, per);
      CHECK(launches * per >= tested && (launches == 0 || (launches - 1) * per < tested));
      CHECK((tested == 0) == (launches == 0));
    }

  if (failures) { std::fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
  std::printf("host OK\n");
  return 0;
}

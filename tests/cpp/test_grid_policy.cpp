// Host-only check of cilantro_amd/csrc/grid_policy.hpp: the shape of the grid build_grid() lays over a cloud, on boxes at the
// edges of the f32 range, degenerate, inverted and non-finite.  Nothing here is a tolerance: every assertion is a property the
// search kernels rely on (dimension caps, finite normal f32 parameters, every box coordinate in a data cell) or a bound on the
// loop's length derived below.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#ifndef GRID_POLICY_HEADER
#define GRID_POLICY_HEADER "../../cilantro_amd/csrc/grid_policy.hpp"
#endif
#include GRID_POLICY_HEADER

using namespace cilhip;

static int g_fail = 0;
static std::string g_what;
#define CHECK(cond) do { if (!(cond)) { if (g_fail < 40) std::printf("FAIL line %d [%s]: %s\n", __LINE__, g_what.c_str(), #cond); ++g_fail; } } while (0)

struct Box { const char* name; float lo[3], hi[3]; };

static const float INF = INFINITY, QNAN = NAN;

// The growth loop multiplies the cell by 1.1 per trip, starts at or above maxext / 2047 (the floor the policy applies first) and
// must have ended when the cell has reached maxext: every axis then holds floor(ext / cell) + 1 <= 2 data cells (one more where
// rounding asked for it), 7^3 cells with the padding.  1.1^t >= 2047 at t = ceil(ln 2047 / ln 1.1) = 80; one trip for the rounding of
// the products.
static int trip_bound() { return (int)std::ceil(std::log((double)(GRID_MAX_DIM - 1)) / std::log(GRID_GROWTH)) + 1; }

// does the policy have the right to refuse this (cleaned) box?  Only when origin or span can leave the f32 range.
static bool may_refuse(const float lo[3], const float hi[3], double cell) {
  double maxext = 0.0, maxabs = 0.0;
  for (int c = 0; c < 3; ++c) {
    maxext = std::fmax(maxext, (double)hi[c] - (double)lo[c]);
    maxabs = std::fmax(maxabs, std::fmax(std::fabs((double)lo[c]), std::fabs((double)hi[c])));
  }
  const double reach = std::fmax(maxext, std::isfinite(cell) ? cell : 0.0);
  return maxabs + 4.0 * reach >= 0.25 * (double)FLT_MAX;      // (a refusal far inside the range would be a bug of its own)
}

static void check_shape(const GridShape& g) {
  const int dims[3] = {g.nx, g.ny, g.nz};
  const float org[3] = {g.ox, g.oy, g.oz};
  CHECK(g.trips >= 0 && g.trips <= trip_bound());
  for (int c = 0; c < 3; ++c) CHECK(dims[c] >= 1 + 2 * GRID_PAD && dims[c] <= GRID_MAX_DIM);
  CHECK((double)g.nx * (double)g.ny * (double)g.nz <= GRID_MAX_CELLS);
  CHECK(std::isfinite(g.cell) && g.cell > 0.0f && std::fpclassify(g.cell) == FP_NORMAL);
  CHECK(std::isfinite(g.inv_cell) && g.inv_cell > 0.0f);
  CHECK(std::isfinite(g.margin) && g.margin > 0.0f);
  for (int c = 0; c < 3; ++c) {
    CHECK(std::isfinite(org[c]));
    CHECK(std::isfinite(g.lo[c]) && std::isfinite(g.hi[c]) && g.lo[c] <= g.hi[c]);
    // the far end of the grid is a finite f32 too (the searches form origin + n * cell)
    CHECK(std::isfinite(org[c] + (float)dims[c] * g.cell));
    const float lo = g.lo[c], hi = g.hi[c];
    const float mid = (float)(0.5 * ((double)lo + (double)hi));
    const float probe[5] = {lo, std::nextafterf(lo, hi), mid, std::nextafterf(hi, lo), hi};
    int prev = -1;
    for (int k = 0; k < 5; ++k) {
      if (!(probe[k] >= lo && probe[k] <= hi)) continue;
      const int cc = grid_cell_coord(probe[k], org[c], g.inv_cell);
      CHECK(cc >= GRID_PAD && cc <= dims[c] - 1 - GRID_PAD);
      CHECK(cc >= prev);      // monotone: the two ends decide for the whole box
      prev = cc;
    }
  }
}

int main() {
  CHECK(GRID_PAD == 2 && GRID_MAX_DIM == 2048 && GRID_MAX_CELLS == 67108864.0);
  CHECK(trip_bound() < GRID_MAX_TRIPS);

  std::vector<Box> boxes = {
      {"unit cube", {0, 0, 0}, {1, 1, 1}},
      {"single point", {0.5f, -2.0f, 7.0f}, {0.5f, -2.0f, 7.0f}},
      {"single point at 0", {0, 0, 0}, {0, 0, 0}},
      {"line", {0, 1, 2}, {5, 1, 2}},
      {"plane", {0, 1, 2}, {5, 3, 2}},
      {"1e6:1:1", {0, 0, 0}, {1e6f, 1, 1}},
      {"1:1e6:1 off origin", {-3e5f, 10, 10}, {-3e5f + 1, 1e6f, 11}},
      {"+-3e38", {-3e38f, -3e38f, -3e38f}, {3e38f, 3e38f, 3e38f}},
      {"+-3e38 on x", {-3e38f, 0, 0}, {3e38f, 1, 1}},
      {"point at 3e38", {3e38f, 3e38f, 3e38f}, {3e38f, 3e38f, 3e38f}},
      {"FLT_MAX corner", {-FLT_MAX, 0, 0}, {FLT_MAX, 0, 0}},
      {"1e-38 at origin", {0, 0, 0}, {1e-38f, 1e-38f, 1e-38f}},
      {"1e-38 at origin, one axis", {0, 0, 0}, {1e-38f, 0, 0}},
      {"1e-38 at 1e3", {1e3f, 1e3f, 1e3f}, {1e3f + 1e-38f, 1e3f + 1e-38f, 1e3f + 1e-38f}},
      {"subnormal box", {-1e-42f, 0, 0}, {1e-42f, 1e-44f, 0}},
      {"unit cube at 1e3", {1e3f, 1e3f, 1e3f}, {1e3f + 1, 1e3f + 1, 1e3f + 1}},
      {"unit cube at 1e7", {1e7f, -1e7f, 1e7f}, {1e7f + 1, -1e7f + 1, 1e7f + 1}},
      {"one ulp wide at 1e3", {1e3f, 1e3f, 1e3f}, {std::nextafterf(1e3f, INF), 1e3f, 1e3f}},
      {"lo > hi on x", {1, 0, 0}, {0, 1, 1}},
      {"lo > hi on all", {1, 1, 1}, {0, 0, 0}},
      {"no finite coordinate on y", {0, INF, 0}, {1, -INF, 1}},
      {"no finite coordinate at all", {INF, INF, INF}, {-INF, -INF, -INF}},
      {"NaN lo.x", {QNAN, 0, 0}, {1, 1, 1}},
      {"NaN hi.z", {0, 0, 0}, {1, 1, QNAN}},
      {"NaN everywhere", {QNAN, QNAN, QNAN}, {QNAN, QNAN, QNAN}},
  };
  static const char* axis[3] = {"x", "y", "z"};
  static std::vector<std::string> names;
  names.reserve(16);
  for (int c = 0; c < 3; ++c)
    for (int side = 0; side < 4; ++side) {      // +inf / -inf at hi / lo of one axis, the rest a unit cube
      Box b{nullptr, {0, 0, 0}, {1, 1, 1}};
      const float v = (side & 1) ? -INF : INF;
      if (side & 2) b.lo[c] = v; else b.hi[c] = v;
      names.push_back(std::string((side & 1) ? "-inf at " : "+inf at ") + ((side & 2) ? "lo." : "hi.") + axis[c]);
      b.name = names.back().c_str();
      boxes.push_back(b);
    }

  const uint64_t counts[5] = {1ull, 2ull, 1000ull, 1ull << 20, (1ull << 32) - 17ull};
  const double occupancy[3] = {0.25, 1.0, 8.0};
  int refused = 0, shaped = 0;
  for (const Box& b : boxes)
    for (uint64_t n : counts)
      for (double occ : occupancy) {
        g_what = std::string(b.name) + " n=" + std::to_string(n) + " occ=" + std::to_string(occ);
        float lo[3], hi[3];
        grid_clean_box(b.lo, b.hi, lo, hi);
        for (int c = 0; c < 3; ++c) {
          const bool ok = std::isfinite(b.lo[c]) && std::isfinite(b.hi[c]) && b.lo[c] <= b.hi[c];
          CHECK(lo[c] == (ok ? b.lo[c] : 0.0f) && hi[c] == (ok ? b.hi[c] : 0.0f));
        }
        const double first = grid_first_cell(lo, hi, n, occ);
        CHECK(!std::isnan(first) && first >= 0.0);
        // build_grid's first call, and its refinement steps (a shrunk cell), and cells no caller should pass
        const double cells[9] = {first, first * 0.3, first * 0.85 * 0.85 * 0.85, 0.0, -1.0, (double)NAN, (double)INFINITY, 1e-300, 1e300};
        for (double cell : cells) {
          GridShape g{};
          const int rc = grid_set_dims(g, b.lo, b.hi, cell);      // (the raw box: the policy cleans it itself)
          CHECK(rc == GRID_POLICY_OK || rc == GRID_POLICY_RANGE);
          if (rc != GRID_POLICY_OK) {
            CHECK(may_refuse(lo, hi, cell));
            CHECK(g.trips <= trip_bound());
            ++refused;
            continue;
          }
          ++shaped;
          for (int c = 0; c < 3; ++c) CHECK(g.lo[c] == lo[c] && g.hi[c] == hi[c]);
          check_shape(g);
        }
      }
  // the +-3e38 cube cannot be indexed in f32 (its span is not an f32 number): refused, not mis-shaped
  {
    g_what = "+-3e38 refused";
    const float lo[3] = {-3e38f, -3e38f, -3e38f}, hi[3] = {3e38f, 3e38f, 3e38f};
    GridShape g{};
    CHECK(grid_set_dims(g, lo, hi, 1e36) == GRID_POLICY_RANGE);
  }
  CHECK(refused > 0 && shaped > refused);

  // finite boxes at offsets where f32 rounding of the origin and of (x - origin) / cell matters: random extents and cells
  {
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto rnd = [&s]() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
    const double offsets[6] = {0.0, 1.0, 1e3, -1e5, 1e7, 3e30};
    for (int it = 0; it < 20000; ++it) {
      const double off = offsets[it % 6];
      const double scale = off == 0.0 ? 1.0 : std::fabs(off) * std::pow(10.0, -6.0 * rnd());
      float lo[3], hi[3];
      for (int c = 0; c < 3; ++c) {
        lo[c] = (float)(off + scale * (rnd() - 0.5));
        hi[c] = (float)((double)lo[c] + scale * rnd() * ((it % 7) == c ? 0.0 : 1.0));
        if (hi[c] < lo[c]) hi[c] = lo[c];
      }
      const uint64_t n = 1ull + (uint64_t)(rnd() * 1e6);
      const double cell = grid_first_cell(lo, hi, n, 1.0) * (0.3 + rnd());
      g_what = "random box " + std::to_string(it);
      GridShape g{};
      CHECK(grid_set_dims(g, lo, hi, cell) == GRID_POLICY_OK);
      check_shape(g);
    }
  }

  // a well-conditioned cloud gets exactly the textbook grid: cell as asked, origin = lo - GRID_PAD * cell, n = floor(ext / cell) + 1 + 2 GRID_PAD
  {
    g_what = "textbook";
    const float lo[3] = {-1.0f, 0.0f, 2.0f}, hi[3] = {1.0f, 0.5f, 2.25f};
    GridShape g{};
    CHECK(grid_set_dims(g, lo, hi, 0.125) == GRID_POLICY_OK);
    CHECK(g.cell == 0.125f && g.inv_cell == 8.0f && g.margin == 0.125f / 512.0f && g.trips == 0);
    CHECK(g.ox == -1.25f && g.oy == -0.25f && g.oz == 1.75f);
    CHECK(g.nx == 16 + 1 + 4 && g.ny == 4 + 1 + 4 && g.nz == 2 + 1 + 4);
    // the dimension cap: 1e6 : 1 : 1 asked for cell 1 -> the floor maxext / 2047, grown until 2048 cells hold the axis
    const float lo2[3] = {0, 0, 0}, hi2[3] = {1e6f, 1, 1};
    CHECK(grid_set_dims(g, lo2, hi2, 1.0) == GRID_POLICY_OK);
    CHECK(g.nx <= GRID_MAX_DIM && g.nx > GRID_MAX_DIM / 2 && g.trips >= 1 && g.trips <= 2);
    // non-finite coordinates map to a clamped cell coordinate, never to an undefined cast
    CHECK(grid_cell_coord(NAN, 0.0f, 1.0f) == -1 && grid_cell_coord(-INFINITY, 0.0f, 1.0f) == -1 && grid_cell_coord(INFINITY, 0.0f, 1.0f) == 1000000000);
  }

  if (g_fail) { std::printf("%d FAILED\n", g_fail); return 1; }
  std::printf("ALL OK (%d grids shaped, %d refused, trip bound %d)\n", shaped, refused, trip_bound());
  return 0;
}

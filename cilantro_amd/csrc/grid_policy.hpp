// grid_policy.hpp -- the shape of the uniform grid build_grid() lays over a cloud: the box it accepts, the first guess of the
// cell edge, the dimensions and the f32 origin / cell / reciprocal the kernels index with, and that index expression itself.
// Plain C++17, no HIP: compiled by the host compiler for tests/cpp/test_grid_policy.cpp, and by hipcc for grid_build.hip (the
// cell index is a host/device function, so the kernels and the test run the same code).
//
// What the policy guarantees for every input, finite or not (the test asserts each point):
//   * it returns: the growth loop runs at most GRID_MAX_TRIPS times and is never entered with a non-finite extent;
//   * every dimension lies in [1 + 2 GRID_PAD, GRID_MAX_DIM], their product is at most GRID_MAX_CELLS;
//   * cell, 1 / cell, origin and margin are finite f32 values, the cell a normal positive one;
//   * with the f32 index expression every coordinate of the (cleaned) box lands in a DATA cell, GRID_PAD <= c <= n - 1 - GRID_PAD
//     per axis: GRID_PAD layers of empty cells surround the data, so every cell that can hold a point and the first layer around
//     it have all 26 neighbours inside the grid (the fast search path has no boundary cases);
//   * or it refuses (GRID_POLICY_RANGE): a finite box so large that origin or span leave the f32 range.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CILHIP_GRID_HD __host__ __device__
#else
#define CILHIP_GRID_HD
#endif

namespace cilhip {

// Layers of empty cells around the data's bounding box.  Two: queries up to one cell outside the data (source points
// that noise / the current transform pushed just past the target's bounding box) still have all 26 neighbour cells
// inside the grid and stay on the fast search path.
constexpr int GRID_PAD = 2;
constexpr int GRID_MAX_DIM = 2048;
constexpr double GRID_MAX_CELLS = 67108864.0;   // 2^26
constexpr double GRID_GROWTH = 1.1;             // the cell grows by this factor until the dimensions fit the caps
// The loop starts at or above maxext / (GRID_MAX_DIM - 1) and has certainly ended once the cell reaches maxext (every axis then
// spans at most two data cells): ceil(ln 2047 / ln 1.1) = 80 trips; the cap leaves room and is never met.
constexpr int GRID_MAX_TRIPS = 128;
// Smallest cell edge: far inside the normal f32 range, so that the cell, its reciprocal (2^96) and the margin (2^-105) are
// normal numbers whatever the cloud's extent (a box of extent 1e-38 would otherwise get a subnormal cell and 1 / cell = inf).
constexpr double GRID_MIN_CELL = 1.262177448353619e-29;   // 2^-96
// ... and relative to the coordinates: a cell narrower than a few ulps of the largest coordinate cannot be told from its
// neighbours in f32 (the origin lo - GRID_PAD * cell rounds back onto lo).
constexpr double GRID_MIN_CELL_ULPS = 8.0;

enum { GRID_POLICY_OK = 0, GRID_POLICY_RANGE = 1 };

struct GridShape {
  float lo[3], hi[3];          // the box the grid was laid over (cleaned: see grid_clean_box)
  float ox, oy, oz;            // origin: GRID_PAD cells (a little more where f32 rounding asks for it) below lo
  float cell, inv_cell, margin;
  int nx, ny, nz;
  int trips;                   // growth steps the dimension loop took (the test bounds it)
};

// Cell coordinate of v along one axis, before the clamp to the grid: THE f32 expression of the index build (cell_of,
// cube_key_of).  NaN maps to -1 (fmaxf drops it), -inf to -1, +inf to 1e9; the cast is always in range.
CILHIP_GRID_HD inline int grid_cell_coord(float v, float o, float inv_cell) {
  return (int)floorf(fminf(fmaxf((v - o) * inv_cell, -1.0f), 1.0e9f));
}

// An axis is usable when both bounds are finite and ordered.  Anything else (no finite coordinate on the axis: lo = +inf,
// hi = -inf; a NaN or infinite bound) becomes extent 0 at origin 0.
inline void grid_clean_box(const float lo_in[3], const float hi_in[3], float lo[3], float hi[3]) {
  for (int c = 0; c < 3; ++c) {
    const bool ok = std::isfinite(lo_in[c]) && std::isfinite(hi_in[c]) && lo_in[c] <= hi_in[c];
    lo[c] = ok ? lo_in[c] : 0.0f;
    hi[c] = ok ? hi_in[c] : 0.0f;
  }
}

// First guess of the cell edge from the density: target_occupancy points per cell of a volumetric cloud; degenerate extents
// are floored so planar / linear clouds still get a sane guess.  (lo, hi: a cleaned box.)  May return 0 (a single point) or a
// value the f32 range cannot hold: grid_set_dims() takes care of both.
inline double grid_first_cell(const float lo[3], const float hi[3], uint64_t n, double target_occupancy) {
  const double ext[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};
  const double maxext = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
  double vol = 1.0;
  for (int c = 0; c < 3; ++c) vol *= std::fmax(ext[c], maxext * 1e-3);
  const double target = target_occupancy > 0.0 ? target_occupancy : 1.0;
  return std::cbrt(vol * target / (double)(n ? n : 1));
}

inline double grid_ulp32(double a) {      // spacing of the f32 numbers at |a| (a finite, within the f32 range)
  const float f = (float)std::fabs(a);
  const float up = std::nextafterf(f, INFINITY);
  return std::isfinite(up) ? (double)up - (double)f : (double)f - (double)std::nextafterf(f, 0.0f);
}

// Dimensions, origin and cell for the box [lo_in, hi_in] and the wanted cell edge.  For a cloud whose coordinates are
// well inside the f32 range and whose cell is wider than a few ulps of them, this is: cell = max(cell, maxext / 2047), grown
// by 1.1 until the caps hold, origin = lo - GRID_PAD * cell, n = floor(ext / cell) + 1 + 2 GRID_PAD.  The f32 index
// expression is then CHECKED on lo and hi of every axis (it is monotone in the coordinate: the two ends decide for the whole
// box); where rounding put lo below cell GRID_PAD the origin moves down by a quarter cell, where it put hi past the last data
// cell the axis gets the cells it needs, and a grid that then breaks a cap grows like any other.
inline int grid_set_dims(GridShape& g, const float lo_in[3], const float hi_in[3], double cell) {
  grid_clean_box(lo_in, hi_in, g.lo, g.hi);
  const float* lo = g.lo; const float* hi = g.hi;
  const double ext[3] = {(double)hi[0] - lo[0], (double)hi[1] - lo[1], (double)hi[2] - lo[2]};   // finite, >= 0
  double maxext = std::fmax(ext[0], std::fmax(ext[1], ext[2]));
  double maxabs = 0.0;
  for (int c = 0; c < 3; ++c) maxabs = std::fmax(maxabs, std::fmax(std::fabs((double)lo[c]), std::fabs((double)hi[c])));
  g.trips = 0;
  if (!(maxext > 0.0)) maxext = 1.0;
  if (!(cell > 0.0) || !std::isfinite(cell)) cell = maxext;
  cell = std::fmax(cell, maxext / (GRID_MAX_DIM - 1));
  cell = std::fmax(cell, std::fmax(GRID_MIN_CELL, GRID_MIN_CELL_ULPS * grid_ulp32(maxabs)));
  // the cell grows to max(cell, maxext) at most: origin (lo - 2.25 cell) and span (hi - origin) must stay inside the f32 range
  if (!(maxabs + 4.0 * std::fmax(maxext, cell) < (double)FLT_MAX)) return GRID_POLICY_RANGE;
  for (;;) {
    const float cf = (float)cell, inv = 1.0f / cf;
    double nd[3];
    float o[3];
    bool ok = std::isfinite(cf) && cf >= FLT_MIN && std::isfinite(inv);
    for (int c = 0; c < 3 && ok; ++c) {
      nd[c] = std::floor(ext[c] / cell) + 1 + 2 * GRID_PAD;
      o[c] = lo[c] - (float)GRID_PAD * cf;
      if (grid_cell_coord(lo[c], o[c], inv) < GRID_PAD) o[c] = lo[c] - ((float)GRID_PAD + 0.25f) * cf;
      const int clo = grid_cell_coord(lo[c], o[c], inv), chi = grid_cell_coord(hi[c], o[c], inv);
      if (!std::isfinite(o[c]) || clo < GRID_PAD || chi < clo) { ok = false; break; }
      nd[c] = std::fmax(nd[c], (double)chi + 1 + GRID_PAD);
    }
    if (ok && nd[0] * nd[1] * nd[2] <= GRID_MAX_CELLS && nd[0] <= GRID_MAX_DIM && nd[1] <= GRID_MAX_DIM && nd[2] <= GRID_MAX_DIM) {
      g.nx = (int)nd[0]; g.ny = (int)nd[1]; g.nz = (int)nd[2];
      g.cell = cf; g.inv_cell = inv; g.margin = cf * (1.0f / 512.0f);
      g.ox = o[0]; g.oy = o[1]; g.oz = o[2];
      return GRID_POLICY_OK;
    }
    if (++g.trips > GRID_MAX_TRIPS) return GRID_POLICY_RANGE;
    cell *= GRID_GROWTH;
  }
}

}  // namespace cilhip

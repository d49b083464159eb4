// components_nd_host.hpp -- the host half of cilhip_connected_components_nd (csrc/components_nd.hip): plain C++, no HIP.
//   ccn_check          the argument rules C5 of DESIGN.md section 23, in the order the entry applies them; the text is what
//                      cilhip_last_error(NULL) then says
//   ccn_answer_empty   the call without a point: no kernel, no device
//   ccn_form           which hook form a call runs (form 0: the code decides)
//   ccn_key / ccn_unkey   the order-preserving integer image of a float (ascending keys = ascending floats, -0 before +0)
//   ccn_pick_axis      form 2's sweep axis from the per-axis minimum and maximum keys of the finite rows
//   ccn_prune_radius   R: the smallest f32 with fl(R * R) >= radius_sq
//   ccn_skips          the prune rule for one (row tile, column tile) pair
//   ccn_plan_full / ccn_plan_pruned   which column tiles every row tile meets: one interval [first[I], I] each, and where the row's
//                      tile pairs begin in the flat list the launches walk
//   ccn_tile_pairs_per_launch / ccn_launches   the cut of that list into launches that test at most `max_pairs` pairs each
// tests/cpp/test_components_nd_host.cpp runs all of it stand-alone (also under ASan / UBSan).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/cilantro_hip/c_api.h"
#include "knn_nd_host.hpp"

namespace cilhip {

constexpr size_t CCN_TILE = 256;      // points of a row tile (one per lane of a block) and of a column tile (staged in LDS)

// No launch tests more than this many pairs -- a launch must not hold a shared card for seconds: under a quarter of a second at the slowest
// N-D pair rate the project had measured before this unit, 4.1e11 pairs/s at dim = 16 (profiles/mean_shift_nd_bench.json: 0.15 s), and at
// the slowest rate of this unit's own bench with 30 000 points and more, 3.1e11 pairs/s on one dense ball of 30 000 points
// (profiles/components_nd_bench.json: 0.19 s; two runs gave 3.4e11 and 3.1e11 there, and 8.0e11 and more everywhere else).
constexpr unsigned long long CCN_MAX_PAIRS_PER_LAUNCH = 60000000000ull;      // 6e10

// the arguments of cilhip_connected_components_nd that a rule looks at
struct CcnCall {
  const float *points, *normals, *rgb;
  size_t n, dim;
  int mem;
  const cilhip_cc_params* params;
  int form;
  const uint32_t* seeds; size_t n_seeds;
  const uint32_t* labels_out;
  const size_t* n_segments_out;
};

inline NdVerdict ccn_check(const CcnCall& c) {
  if (!c.params) return {-1, "params is null"};
  if (!c.n_segments_out) return {-1, "n_segments_out is null"};
  if (c.dim == 0) return {-1, "dim is 0"};
  if (c.form < 0 || c.form > 2) return {-1, "form: 0 (chosen by the code), 1 (exhaustive) or 2 (sweep and prune)"};
  if (c.n >= ND_MAX_COUNT) return {-1, "n must be below 2^32 - 16"};
  if (c.mem != CILHIP_MEM_HOST && c.mem != CILHIP_MEM_DEVICE) return {-1, "mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE"};
  if (c.n && !c.labels_out) return {-1, "labels_out is null"};
  if (c.n_seeds && !c.seeds) return {-1, "n_seeds > 0 without a seed array"};
  for (size_t k = 0; k < c.n_seeds; ++k)
    if (c.seeds[k] >= c.n) return {-1, "a seed index is not below n"};
  if (!std::isfinite(c.params->radius_sq)) return {-1, "radius_sq must be finite"};
  if (c.params->use_normals && !c.normals) return {-1, "a normals clause without the normals array"};
  if (c.params->use_colors && !c.rgb) return {-1, "a colours clause without the colours array"};
  if (c.n && !c.points) return {-1, "points is null"};
  if (c.dim > ND_MAX_DIM) return {-3, "dim > 16"};
  return {0, nullptr};
}

// no point at all: zero segments; an offsets array in host memory gets its one word
inline void ccn_answer_empty(int mem, uint32_t* offsets_out_or_null, size_t* n_segments_out) {
  *n_segments_out = 0;
  if (offsets_out_or_null && mem == CILHIP_MEM_HOST) offsets_out_or_null[0] = 0;
}

// Form 0: below CCN_FORM2_MIN_POINTS the sort costs more than it saves.  Measured on the uniform cloud, where pruning gains least
// (profiles/components_nd_bench.json; whole-call times, dim 2, 3, 6, 9, 16): up to 16 384 points form 1 is ahead or
// level at every dim (the sort, the gather and their two synchronisations cost 0.1 to 0.2 ms, the whole triangle less); at 32 768 the two
// are within 0.1 ms of each other either way (0.3 ms for form 1 at dim 16); at 65 536 form 2 is ahead at dim 2 to 9 (0.07 to 0.2 ms) and
// form 1 at dim 16 (0.17 ms); at 262 144 form 2 is ahead at every dim (1.2 to 3.4 times).  The crossover lies between 32 768 and 65 536.
constexpr size_t CCN_FORM2_MIN_POINTS = 65536;
inline int ccn_form(int form, size_t n) { return form ? form : (n >= CCN_FORM2_MIN_POINTS ? 2 : 1); }

inline size_t ccn_tiles(size_t rows) { return (rows + CCN_TILE - 1) / CCN_TILE; }

// ---- keys -----------------------------------------------------------------------------------------------------------------------
// (constexpr: usable in device code as well)
constexpr uint32_t ccn_key_bits(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
constexpr uint32_t ccn_unkey_bits(uint32_t k) { return (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; }
constexpr uint32_t CCN_KEY_DROPPED = 0xFFFFFFFFu;      // above the key of every finite float and of +inf: a row with a non-finite coordinate sorts last
inline uint32_t ccn_key(float v) { uint32_t u; std::memcpy(&u, &v, 4); return ccn_key_bits(u); }
inline float ccn_unkey(uint32_t k) { const uint32_t u = ccn_unkey_bits(k); float v; std::memcpy(&v, &u, 4); return v; }

// the axis of largest finite extent (max - min of the rows that are finite on every axis), lowest axis on ties.  The extents are compared
// in double: the difference of two floats is exact there or, beyond 2^53 ulps apart, rounded monotonically -- and never overflows.
inline size_t ccn_pick_axis(const uint32_t* min_keys, const uint32_t* max_keys, size_t dim) {
  size_t best = 0;
  double best_extent = -1.0;
  for (size_t a = 0; a < dim; ++a) {
    const double extent = (double)ccn_unkey(max_keys[a]) - (double)ccn_unkey(min_keys[a]);
    if (extent > best_extent) { best_extent = extent; best = a; }
  }
  return best;
}

// ---- the prune ------------------------------------------------------------------------------------------------------------------
inline float ccn_sq(float r) { volatile float p = r * r; return p; }      // one f32 product, whatever the host compiler would like to keep wider

// R = the smallest f32 with fl(R * R) >= radius_sq (radius_sq finite and > 0).  fl(r * r) is monotone in r >= 0 and the bit patterns of
// the non-negative floats ascend with their values, so R is found by bisection over the bit pattern: sqrtf alone can be one step off
// either way, and near the subnormals millions of floats share one square.  fl(FLT_MAX * FLT_MAX) = +inf >= everything: R exists.
inline float ccn_prune_radius(float radius_sq) {
  uint32_t lo = 0u, hi = 0x7F7FFFFFu;      // fl(lo * lo) = 0 < radius_sq; hi = FLT_MAX holds
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    float r; std::memcpy(&r, &mid, 4);
    if (ccn_sq(r) >= radius_sq) hi = mid; else lo = mid;
  }
  float R; std::memcpy(&R, &hi, 4);
  return R;
}

// Column tile J lies before row tile I in sorted order along the sweep axis.  It is skipped iff fl(min_a(I) - max_a(J)) >= R: then for every
// row i of I and j of J, t = fl(x_ia - x_ja) >= R (rounding is monotone), fl(t * t) >= fl(R * R) >= radius_sq, and d2, a sum of
// non-negative rounded terms that holds fl(t * t), is at least that: no skipped pair is an edge.
inline bool ccn_skips(float min_row_tile, float max_col_tile, float R) {
  volatile float t = min_row_tile - max_col_tile;
  return t >= R;
}

// first[I]: the first column tile row tile I meets -- it meets [first[I], I]; begin[I]: how many tile pairs the rows before I hold
// (begin[tiles] = all of them: tested).
struct CcnPlan {
  std::vector<uint32_t> first;
  std::vector<unsigned long long> begin;
  unsigned long long total = 0, tested = 0;      // tile pairs of the whole triangle, and those met
};

inline CcnPlan ccn_plan_full(size_t tiles) {
  CcnPlan p;
  p.first.assign(tiles, 0u);
  p.begin.resize(tiles + 1);
  for (size_t I = 0; I <= tiles; ++I) p.begin[I] = (unsigned long long)I * (I + 1) / 2;
  p.total = p.tested = p.begin[tiles];
  return p;
}

// tile_min[I] / tile_max[I]: the sweep coordinate of tile I's first / last row in sorted order (non-descending in I).  max_a(J) does not
// descend with J, so fl(min_a(I) - max_a(J)) does not ascend: the skipped tiles of a row are a prefix, found by bisection.
inline CcnPlan ccn_plan_pruned(const float* tile_min, const float* tile_max, size_t tiles, float R) {
  CcnPlan p;
  p.first.resize(tiles);
  p.begin.resize(tiles + 1);
  unsigned long long at = 0;
  for (size_t I = 0; I < tiles; ++I) {
    size_t lo = 0, hi = I;      // the answer lies in [lo, hi]: tile I itself is never skipped (its difference is <= 0 < R)
    while (lo < hi) {
      const size_t mid = lo + (hi - lo) / 2;
      if (ccn_skips(tile_min[I], tile_max[mid], R)) lo = mid + 1; else hi = mid;
    }
    p.first[I] = (uint32_t)lo;
    p.begin[I] = at;
    at += I - lo + 1;
  }
  p.begin[tiles] = at;
  p.tested = at;
  p.total = (unsigned long long)tiles * (tiles + 1) / 2;
  return p;
}

// ---- the launches ---------------------------------------------------------------------------------------------------------------
// a block tests one tile pair: at most CCN_TILE^2 pairs.  max_pairs = 0: the default above.
inline unsigned long long ccn_tile_pairs_per_launch(unsigned long long max_pairs) {
  const unsigned long long cap = max_pairs ? max_pairs : CCN_MAX_PAIRS_PER_LAUNCH;
  unsigned long long per = cap / (CCN_TILE * CCN_TILE);
  if (per < 1) per = 1;
  if (per > 0x7FFFFFFFull) per = 0x7FFFFFFFull;      // a grid's x extent
  return per;
}
// launch k walks the tile pairs [k * per, min((k + 1) * per, tested))
inline unsigned long long ccn_launches(unsigned long long tested, unsigned long long per) { return (tested + per - 1) / per; }

}  // namespace cilhip

// mds_host.hpp -- the scalar decisions of the multidimensional-scaling solver (rules M3-M5), plain C++ for the host:
//   mds_sizes             M3: dimension, estimation, number of wanted pairs
//   magnitude_order       M4: indices by descending |theta|, equal magnitudes by ascending index
//   mds_filter_plan       the filter of one outer iteration: damped interval [-e, e] and the adaptive degree
//   mds_accepts           M4: Spectra's test on a true residual
//   mds_embedding_dim     M5: estimateEmbeddingDimensionEigengap (utilities/multidimensional_scaling.hpp:10-31), literally in f32
// No allocation, no dependency: tests/cpp/test_mds_host.cpp runs it alone.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>

namespace cilhip {

// utilities/multidimensional_scaling.hpp:106-118 and :40-42
struct MdsSizes { size_t dim; bool estimate; size_t nev; };
inline MdsSizes mds_sizes(size_t n, size_t max_dim, bool estimate_dim) {
  MdsSizes z{max_dim, estimate_dim, 0};
  if (max_dim == 0 || max_dim >= n) { z.dim = 2; z.estimate = false; }
  const size_t plus = z.dim + 1, cap = n - 1;
  z.nev = z.estimate ? (plus < cap ? plus : cap) : z.dim;
  return z;
}

// order[0 .. m): the indices of v by descending |v| (insertion sort: stable, so equal magnitudes keep ascending index)
inline void magnitude_order(const double* v, int m, int* order) {
  for (int i = 0; i < m; ++i) {
    int k = i;
    while (k > 0 && std::fabs(v[order[k - 1]]) < std::fabs(v[i])) { order[k] = order[k - 1]; --k; }
    order[k] = i;
  }
}

// Spectra's test (HermEigsBase.h:152-167) with the float literal of multidimensional_scaling.hpp:44; residual of a unit vector
inline bool mds_accepts(double residual, double theta) {
  const double tol = (double)1e-7f, eps23 = (double)std::pow(FLT_EPSILON, 2.0f / 3.0f);
  const double at = std::fabs(theta);
  return residual < tol * (eps23 > at ? eps23 : at);
}

// a0: the first unlocked magnitude (the filter is 1 there), least: the smallest magnitude of the block, lowest_wanted: the smallest
// magnitude among the wanted pairs, top_locked: the largest locked magnitude (0: nothing is locked).  e: the filter damps [-e, e] --
// `least`, or a0 / 2 when `least` is not below a0 (1 - 1e-3).  degree: the largest m <= max_degree that keeps two gains of the filter,
// exp(m (acosh(hi / e) - acosh(lo / e))), in bounds -- at least 1:
//   between a0 and the lowest wanted magnitude (clipped to e from below) within 1e6: beyond it the lower columns drown in the rounding of
//     the upper ones;
//   between the largest locked magnitude and a0 within 1e10: the unlocked columns keep a component of rounding size (1e-16) along the
//     locked vectors, the filter amplifies it by that gain, and the two projections that follow remove it only while it stays below 1.
struct MdsFilterPlan { double e; int degree; };
inline MdsFilterPlan mds_filter_plan(double a0, double least, double lowest_wanted, double top_locked, int max_degree) {
  MdsFilterPlan p{least, 1};
  if (!(p.e < a0 * (1.0 - 1e-3)) || !(p.e > 0.0)) p.e = 0.5 * a0;
  const double lo = lowest_wanted > p.e ? lowest_wanted : p.e;
  const double at_a0 = std::acosh(a0 / p.e);
  const double spread = at_a0 - std::acosh(lo / p.e), above = top_locked > a0 ? std::acosh(top_locked / p.e) - at_a0 : 0.0;
  int m = max_degree;
  if (spread > 0.0 && (double)m * spread > std::log(1e6)) m = (int)std::floor(std::log(1e6) / spread);
  if (above > 0.0 && (double)m * above > std::log(1e10)) m = (int)std::floor(std::log(1e10) / above);
  p.degree = m < 1 ? 1 : m;
  return p;
}

// estimateEmbeddingDimensionEigengap, utilities/multidimensional_scaling.hpp:10-31
inline size_t mds_embedding_dim(const float* ev, size_t count, size_t max_dim) {
  float min_val = INFINITY, max_val = -INFINITY, max_diff = -INFINITY;
  size_t max_ind = 0;
  for (size_t i = 0; i + 1 < count; ++i) {
    const float diff = ev[i] - ev[i + 1];
    if (diff > max_diff) { max_diff = diff; max_ind = i; }
    if (ev[i] < min_val) min_val = ev[i];
    if (ev[i] > max_val) max_val = ev[i];
  }
  if (ev[count - 1] < min_val) min_val = ev[count - 1];
  if (ev[count - 1] > max_val) max_val = ev[count - 1];
  if (max_val - min_val < FLT_EPSILON) return max_dim;
  return max_ind + 1;
}

}  // namespace cilhip

// mean_shift_nd_host.hpp -- the host half of cilhip_mean_shift_nd (csrc/mean_shift_nd.hip): plain C++, no HIP.
//   msn_check          the argument rules of DESIGN.md section 22, in the order the entry applies them; the text is what
//                      cilhip_last_error(NULL) then says
//   msn_answer_empty   the call without a single seed: no kernel, no device
//   msn_slices         into how many slices of consecutive point indices a pass cuts the point stream (rule M3: the one thing beside the
//                      input that the last bit of a step may depend on), msn_slice_length: how long a slice is, msn_part_doubles: the
//                      room the slices' partial sums need over a whole run
// tests/cpp/test_mean_shift_nd_host.cpp runs all of it stand-alone (also under ASan / UBSan).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/cilantro_hip/c_api.h"
#include "knn_nd_host.hpp"

namespace cilhip {

constexpr size_t MSN_TILE = 4;      // candidates evaluated together: a slice is a multiple of it

inline bool msn_tolerance(float v) { return std::isfinite(v) && v >= 0.0f; }

// the arguments of cilhip_mean_shift_nd that a rule looks at
struct MsnCall {
  const float* points; size_t n, dim;
  const float* seeds; size_t n_seeds;
  int mem;
  const cilhip_ms_params* params;
  const float* shifted_out; const uint32_t* labels_out;
  const size_t *n_clusters_out, *iterations_out;
};

inline NdVerdict msn_check(const MsnCall& c) {
  if (!c.params) return {-1, "params is null"};
  if (!c.n_clusters_out) return {-1, "n_clusters_out is null"};
  if (!c.iterations_out) return {-1, "iterations_out is null"};
  if (c.dim == 0) return {-1, "dim is 0"};
  if (c.n >= ND_MAX_COUNT) return {-1, "n must be below 2^32 - 16"};
  if (c.n_seeds >= ND_MAX_COUNT) return {-1, "n_seeds must be below 2^32 - 16"};
  if (c.mem != CILHIP_MEM_HOST && c.mem != CILHIP_MEM_DEVICE) return {-1, "mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE"};
  if (c.n && !c.points) return {-1, "points is null"};
  if (c.n_seeds && !c.seeds) return {-1, "n_seeds > 0 without a seed array"};
  const cilhip_ms_params& p = *c.params;
  if (!msn_tolerance(p.kernel_radius)) return {-1, "kernel_radius must be finite and not negative"};
  if (!msn_tolerance(p.cluster_tol)) return {-1, "cluster_tol must be finite and not negative"};
  if (!msn_tolerance(p.convergence_tol)) return {-1, "convergence_tol must be finite and not negative"};
  if (p.kernel_kind != 0 && p.kernel_kind != 1 && p.kernel_kind != 2) return {-1, "kernel_kind: 0 (Unity), 1 (Identity) or 2 (RBF)"};
  if (p.kernel_kind == 2 && !(std::isfinite(p.kernel_sigma) && p.kernel_sigma > 0.0f)) return {-1, "kernel_sigma must be finite and positive"};
  if (p.form != 0) return {-1, "form must be 0 (there is one shift kernel in dim dimensions)"};
  const size_t ns = c.seeds ? c.n_seeds : c.n;
  if (ns && !c.shifted_out) return {-1, "shifted_seeds_out is null"};
  if (ns && !c.labels_out) return {-1, "labels_out is null"};
  if (c.dim > ND_MAX_DIM) return {-3, "dim > 16"};
  return {0, nullptr};
}

// no seed at all: zero clusters, zero iterations; an offsets array in host memory gets its one word
inline void msn_answer_empty(int mem, uint32_t* offsets_out_or_null, size_t* n_clusters_out, size_t* iterations_out) {
  *n_clusters_out = 0;
  *iterations_out = 0;
  if (offsets_out_or_null && mem == CILHIP_MEM_HOST) offsets_out_or_null[0] = 0;
}

// How many slices of the point stream a pass over n_active seeds scans side by side (each slice of every 256 active seeds is one block; the
// slices' f64 partial sums are added afterwards in ascending slice order).  One slice when the seeds alone fill the device; otherwise enough
// for about MSN_TARGET_BLOCKS blocks, never slices shorter than MSN_MIN_SLICE points, more than MSN_MAX_SLICES of them, or more than
// MSN_PART_BYTES of partial sums (17 doubles per seed and slice: the widest case, so that the plan does not depend on dim).
// The first two constants are nd_slices'; the cap is higher because a run's last passes hold a handful of seeds.  Measured (NOTEBOOK
// 2026-10-20, profiles/mean_shift_nd_bench.json): a minimum slice of 2048 slows 1500 x 1500 points 1.7 times and changes nothing at 1e10
// pairs per pass; a cap of 32 changes no case by more than 2 %, which one run each does not resolve.
#ifndef MSN_MIN_SLICE_POINTS      // (tools/mean_shift_nd_bench.py builds variant libraries with other values of these two to sweep them)
#define MSN_MIN_SLICE_POINTS 512
#endif
#ifndef MSN_SLICE_CAP
#define MSN_SLICE_CAP 256
#endif
constexpr size_t MSN_TARGET_BLOCKS = 1024, MSN_MIN_SLICE = MSN_MIN_SLICE_POINTS, MSN_MAX_SLICES = MSN_SLICE_CAP, MSN_PART_BYTES = (size_t)64 << 20;
constexpr size_t MSN_PART_ROW_BYTES = (ND_MAX_DIM + 1) * sizeof(double);
inline size_t msn_slices(size_t n, size_t n_active) {
  const size_t nblk = (n_active + 255) / 256;
  if (nblk == 0) return 1;
  size_t s = (MSN_TARGET_BLOCKS + nblk - 1) / nblk;
  if (s > n / MSN_MIN_SLICE) s = n / MSN_MIN_SLICE;
  if (s > MSN_MAX_SLICES) s = MSN_MAX_SLICES;
  if (s > MSN_PART_BYTES / MSN_PART_ROW_BYTES / n_active) s = MSN_PART_BYTES / MSN_PART_ROW_BYTES / n_active;
  return s < 1 ? 1 : s;
}
// the slice length: a multiple of MSN_TILE, slices * length >= n; slice y is the points [y * length, min((y + 1) * length, n))
inline size_t msn_slice_length(size_t n, size_t slices) { return nd_slice_length(n, slices, MSN_TILE); }

// doubles that hold slices * n_active * (dim + 1) partial sums for every pass of a run that starts with n_seeds active seeds: a pass with
// more than one slice stays below MSN_PART_BYTES, a pass with one slice needs a row per active seed
inline size_t msn_part_doubles(size_t n, size_t n_seeds, size_t dim) {
  size_t rows = n_seeds;      // one slice
  if (n / MSN_MIN_SLICE > 1) {
    size_t sliced = MSN_PART_BYTES / MSN_PART_ROW_BYTES;
    if (sliced > MSN_MAX_SLICES * n_seeds) sliced = MSN_MAX_SLICES * n_seeds;
    if (rows < sliced) rows = sliced;
  }
  return rows * (dim + 1);
}

}  // namespace cilhip

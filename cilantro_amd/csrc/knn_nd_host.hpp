// knn_nd_host.hpp -- the host half of cilhip_knn_nd / cilhip_radius_search_nd (csrc/knn_nd.hip): plain C++, no HIP.
//   nd_check_knn / nd_check_radius   the argument rules N4 of DESIGN.md section 21, in the order the entries apply them; the text
//                                    is what cilhip_last_error(NULL) then says
//   nd_knn_trivial / nd_radius_trivial   calls no candidate can enter a list of: no kernel, no device
//   nd_pad_rows                      the rows of such a call: 0xFFFFFFFF / +inf padding, count 0
//   nd_empty_offsets                 its radius lists: n_query + 1 zeros
//   nd_radius_plan                   the two-call capacity protocol: given the total, are the lists produced in this call?
// tests/cpp/test_knn_nd_host.cpp runs all of it stand-alone (also under ASan / UBSan).
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

namespace cilhip {

constexpr size_t ND_MAX_DIM = 16;
constexpr size_t ND_MAX_K = 32;
constexpr unsigned long long ND_MAX_COUNT = 0xFFFFFFF0ull;      // 2^32 - 16: sizes stay below it, the radius lists hold at most this many entries
constexpr uint32_t ND_NONE = 0xFFFFFFFFu;

// status: 0 fine, -1 CILHIP_ERR_INVALID, -3 CILHIP_ERR_UNSUPPORTED (the values of c_api.h); what: the rule, null when fine
struct NdVerdict { int status; const char* what; };

inline NdVerdict nd_check_common(const float* ref, size_t n_ref, size_t n_query, size_t dim, int mem) {
  if (!ref && n_ref) return {-1, "ref is NULL with n_ref > 0"};
  if (dim == 0) return {-1, "dim is 0"};
  if (mem != 0 && mem != 1) return {-1, "mem is neither CILHIP_MEM_HOST nor CILHIP_MEM_DEVICE"};
  if (n_ref >= ND_MAX_COUNT || n_query >= ND_MAX_COUNT) return {-1, "n_ref and n_query must be below 2^32 - 16"};
  if (dim > ND_MAX_DIM) return {-3, "dim > 16"};
  return {0, nullptr};
}

inline NdVerdict nd_check_knn(const float* ref, size_t n_ref, size_t n_query, size_t dim, int mem, size_t k, float max_sq_dist, const uint32_t* idx_out) {
  if (!idx_out) return {-1, "idx_out is NULL"};
  if (k == 0) return {-1, "k is 0"};
  if (std::isnan(max_sq_dist)) return {-1, "max_sq_dist is NaN"};
  const NdVerdict v = nd_check_common(ref, n_ref, n_query, dim, mem);
  if (v.status) return v;
  if (k > ND_MAX_K) return {-3, "k > 32"};
  return {0, nullptr};
}

inline NdVerdict nd_check_radius(const float* ref, size_t n_ref, size_t n_query, size_t dim, int mem, float radius_sq, const uint64_t* offsets_out) {
  if (!offsets_out) return {-1, "offsets_out is NULL"};
  if (!std::isfinite(radius_sq)) return {-1, "radius_sq is not finite"};
  return nd_check_common(ref, n_ref, n_query, dim, mem);
}

// nothing can be within a bound that is not positive (d2 >= 0, the test is strict), or among no points
inline bool nd_knn_trivial(size_t n_ref, size_t n_query, float max_sq_dist) { return n_ref == 0 || n_query == 0 || !(max_sq_dist > 0.0f); }
inline bool nd_radius_trivial(size_t n_ref, size_t n_query, float radius_sq) { return n_ref == 0 || n_query == 0 || !(radius_sq > 0.0f); }

inline void nd_pad_rows(size_t n_query, size_t k, uint32_t* idx_out, float* d2_out, uint32_t* counts_out) {
  for (size_t i = 0; i < n_query * k; ++i) {
    idx_out[i] = ND_NONE;
    if (d2_out) d2_out[i] = std::numeric_limits<float>::infinity();
  }
  if (counts_out)
    for (size_t i = 0; i < n_query; ++i) counts_out[i] = 0;
}

inline void nd_empty_offsets(size_t n_query, uint64_t* offsets_out, size_t* total_out_or_null) {
  for (size_t i = 0; i <= n_query; ++i) offsets_out[i] = 0;
  if (total_out_or_null) *total_out_or_null = 0;
}

// How many slices of the reference stream a k-NN call scans side by side (each slice of every 256 queries is one block; the slices' lists are
// merged afterwards).  One slice when the queries alone fill the device; otherwise enough for about ND_TARGET_BLOCKS blocks, never slices
// shorter than ND_MIN_SLICE points, more than ND_MAX_SLICES of them, or more than ND_PART_BYTES of partial lists.
constexpr size_t ND_TARGET_BLOCKS = 1024, ND_MIN_SLICE = 512, ND_MAX_SLICES = 32, ND_PART_BYTES = (size_t)64 << 20;
inline size_t nd_slices(size_t n_ref, size_t n_query, size_t k) {
  const size_t nblk = (n_query + 255) / 256;
  if (nblk == 0 || k == 0) return 1;
  size_t s = (ND_TARGET_BLOCKS + nblk - 1) / nblk;
  if (s > n_ref / ND_MIN_SLICE) s = n_ref / ND_MIN_SLICE;
  if (s > ND_MAX_SLICES) s = ND_MAX_SLICES;
  if (s > ND_PART_BYTES / (n_query * k * 8)) s = ND_PART_BYTES / (n_query * k * 8);
  return s < 1 ? 1 : s;
}
// the slice length: a multiple of `tile`, slices * length >= n_ref
inline size_t nd_slice_length(size_t n_ref, size_t slices, size_t tile) {
  const size_t len = (n_ref + slices - 1) / slices;
  return (len + tile - 1) / tile * tile;
}

// 0: offsets and total only (no room, or nothing to list); 1: fill, sort and unpack now; -3: more than 2^32 - 16 entries together
inline int nd_radius_plan(const uint32_t* idx_out, size_t capacity, unsigned long long total) {
  if (!idx_out || capacity < total || total == 0) return 0;
  return total > ND_MAX_COUNT ? -3 : 1;
}

}  // namespace cilhip

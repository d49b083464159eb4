// knn_lists.hpp -- what the 3-D grid search (knn.hip) and the exhaustive N-D search (knn_nd.hip) keep in ONE copy:
//   KList                 a lane's k best candidates: a column of 64-bit keys (bits(d2) << 32 | index) in LDS, lists[k][KNN_THREADS] -- kept sorted
//                         (insert: knn.hip) or unordered and sorted at the end (put / sort: knn_nd.hip)
//   radius_sort_unpack    the tail of a radius search: filled packed keys -> one segmented radix sort of all lists -> indices / distances on the host
//   k_unpack_radius, k_offsets32   its two kernels
// Included by .hip files only; everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <cstdint>

#include "device_prims.hpp"
#include "stateless.hpp"

namespace cilhip {
namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_MAX_K = 32;

// per-lane sorted list of the k best keys, column `tid` of lists[k][KNN_THREADS]
struct KList {
  unsigned long long* col;   // &lists[threadIdx.x]
  uint32_t k, cnt;
  unsigned long long worst;  // a candidate enters iff key < worst
  unsigned long long none_key;
  uint32_t tie_bits;         // bits of the distance at which a candidate last fell off (or stayed out of) a FULL list while an entry at exactly that
                             // distance stayed in: the k-th place is tied iff this is the final k-th distance (the k-th distance only shrinks)
  __device__ __forceinline__ float worst_d2() const { return __uint_as_float((uint32_t)(worst >> 32)); }
  __device__ __forceinline__ void insert(unsigned long long key) {
    if (key >= worst) { if (cnt == k && (uint32_t)(key >> 32) == (uint32_t)(worst >> 32)) tie_bits = (uint32_t)(key >> 32); return; }
    const bool full = cnt == k;
    const unsigned long long out = full ? col[(size_t)(k - 1) * KNN_THREADS] : 0ull;
    uint32_t j = cnt < k ? cnt : k - 1;
    while (j > 0 && col[(size_t)(j - 1) * KNN_THREADS] > key) { col[(size_t)j * KNN_THREADS] = col[(size_t)(j - 1) * KNN_THREADS]; --j; }
    col[(size_t)j * KNN_THREADS] = key;
    if (cnt < k) ++cnt;
    worst = cnt < k ? none_key : col[(size_t)(k - 1) * KNN_THREADS];
    if (full && (uint32_t)(out >> 32) == (uint32_t)(worst >> 32)) tie_bits = (uint32_t)(out >> 32);
  }

  // ---- the unordered form (knn_nd.hip; a list is kept in one form or the other, never both): the same k best keys in any order, `worst` their
  // largest -- at row wpos -- once the list is full.  An entry costs one pass of independent reads instead of a chain of dependent shifts, which
  // is what a wave pays whenever ANY of its lanes inserts; sort() orders the column once, at the end.
  uint32_t wpos;
  __device__ __forceinline__ void put(unsigned long long key) {      // the caller has seen key < worst
    col[(size_t)(cnt < k ? cnt : wpos) * KNN_THREADS] = key;
    if (cnt < k && ++cnt < k) return;
    unsigned long long w = 0;
    uint32_t wp = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < k; ++j) {
      const unsigned long long v = col[(size_t)j * KNN_THREADS];
      if (v >= w) { w = v; wp = j; }
    }
    worst = w; wpos = wp;
  }
  __device__ __forceinline__ void sort() {      // ascending
    for (uint32_t i = 1; i < cnt; ++i) {
      const unsigned long long key = col[(size_t)i * KNN_THREADS];
      uint32_t j = i;
      while (j > 0 && col[(size_t)(j - 1) * KNN_THREADS] > key) { col[(size_t)j * KNN_THREADS] = col[(size_t)(j - 1) * KNN_THREADS]; --j; }
      col[(size_t)j * KNN_THREADS] = key;
    }
  }
};

__global__ void k_unpack_radius(const unsigned long long* __restrict__ keys, size_t total, uint32_t* __restrict__ idx, float* __restrict__ d2) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const unsigned long long k = keys[i];
    idx[i] = (uint32_t)k;
    if (d2) d2[i] = __uint_as_float((uint32_t)(k >> 32));
  }
}
__global__ void k_offsets32(const unsigned long long* __restrict__ off64, uint32_t n, uint32_t* __restrict__ off32) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) off32[i] = (uint32_t)off64[i];
}

// d_keys[0 .. total): the lists' packed keys, list i at [d_off64[i], d_off64[i + 1]), in any order inside a list (1 <= total <= 2^32 - 16).
// Sorts every list ascending (all lists in one segmented radix sort), unpacks and copies to the HOST arrays idx_out / d2_out (d2_out may be
// null); returns with the stream drained.
inline int radius_sort_unpack(const char* family, DevPool& pool, hipStream_t s, const unsigned long long* d_off64, size_t n_query, size_t total,
                              unsigned long long* d_keys, uint32_t* idx_out, float* d2_out) {
  unsigned long long* d_keys2 = nullptr;
  uint32_t *d_off32 = nullptr, *d_idx = nullptr;
  float* d_d2 = nullptr;
  ST_CK(family, pool.get(&d_keys2, total));
  ST_CK(family, pool.get(&d_off32, n_query + 1));
  hipLaunchKernelGGL(k_offsets32, dim3(256), dim3(256), 0, s, d_off64, (uint32_t)(n_query + 1), d_off32);
  ST_CK(family, prim_run(pool, [&](void* tmp, size_t& bytes) {
    return rocprim::segmented_radix_sort_keys(tmp, bytes, d_keys, d_keys2, (unsigned int)total, (unsigned int)n_query, d_off32, d_off32 + 1, 0, 64, s);
  }));
  ST_CK(family, pool.get(&d_idx, total));
  if (d2_out) ST_CK(family, pool.get(&d_d2, total));
  hipLaunchKernelGGL(k_unpack_radius, dim3(2048), dim3(256), 0, s, (const unsigned long long*)d_keys2, total, d_idx, d_d2);
  ST_CK(family, hipGetLastError());
  ST_CK(family, hipMemcpyAsync(idx_out, d_idx, total * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (d2_out) ST_CK(family, hipMemcpyAsync(d2_out, d_d2, total * sizeof(float), hipMemcpyDeviceToHost, s));
  ST_CK(family, hipStreamSynchronize(s));
  return CILHIP_OK;
}

}  // namespace
}  // namespace cilhip

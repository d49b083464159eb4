// device_prims.hpp -- the scan, sort and compaction plumbing every feature family uses, written once.  Integer-only: nothing here rounds.
//   host    prim_sort_pairs / prim_sort_keys / prim_exclusive_sum / prim_inclusive_sum / prim_exclusive_scan / prim_inclusive_scan
//           a rocPRIM call with its argument list written ONCE, as a callable op(void* tmp, size_t& bytes) -> hipError_t:
//             op(nullptr, bytes)   asks how much temporary storage the call needs (nothing runs)
//             op(block, bytes)     runs in a block of at least that size
//             prim_run(pool, op)   both, the block taken from the call's DevPool in between
//           key_bits          the end_bit of a radix sort over keys 0 .. v
//           group_by_label    labels -> members[] (indices sorted stably by label) + offsets[] (where each label's run starts)
//   kernels k_iota, k_run_offsets, k_scan_counts (one lane: the exclusive scan of at most 1024 block counts); templates over the word
//           type T (uint32_t everywhere today), so that a file that includes this header carries only the kernels it launches
//   device  block_rank<THREADS>   order-preserving compaction inside a block: a lane's rank among the lanes whose flag holds
//           wave_append           unordered append to a list: one atomicAdd per wave
// Included by .hip files only; everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/reverse_iterator.hpp>

#include <algorithm>
#include <cstdint>
#include <iterator>

#include "device_mem.hpp"

namespace {

constexpr int PRIM_THREADS = 256;
inline int prim_blocks(size_t n) { return (int)std::min<size_t>((n + PRIM_THREADS - 1) / PRIM_THREADS, 2048) + (n == 0); }

// ---- host side ----------------------------------------------------------------------------------------------------------------------
template <class Op> hipError_t prim_run(cilhip::DevPool& pool, Op&& op) {
  size_t bytes = 0;
  void* tmp = nullptr;
  hipError_t e = op(nullptr, bytes);
  if (e == hipSuccess) e = pool.bytes(&tmp, bytes);
  return e != hipSuccess ? e : op(tmp, bytes);
}

// stable LSD radix sort over the key bits [begin_bit, end_bit)
template <class KIn, class KOut, class VIn, class VOut>
auto prim_sort_pairs(KIn keys_in, KOut keys_out, VIn vals_in, VOut vals_out, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  return [=](void* tmp, size_t& bytes) { return rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, n, begin_bit, end_bit, s); };
}
template <class KIn, class KOut> auto prim_sort_keys(KIn keys_in, KOut keys_out, size_t n, unsigned begin_bit, unsigned end_bit, hipStream_t s) {
  return [=](void* tmp, size_t& bytes) { return rocprim::radix_sort_keys(tmp, bytes, keys_in, keys_out, n, begin_bit, end_bit, s); };
}

// out[i] = init (+) in[0] (+) ... (+) in[i - 1]; in place (out == in) is fine
template <class In, class Out, class T, class BinaryOp> auto prim_exclusive_scan(In in, Out out, T init, size_t n, BinaryOp op, hipStream_t s) {
  return [=](void* tmp, size_t& bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, init, n, op, s); };
}
// out[i] = in[0] (+) ... (+) in[i]
template <class In, class Out, class BinaryOp> auto prim_inclusive_scan(In in, Out out, size_t n, BinaryOp op, hipStream_t s) {
  return [=](void* tmp, size_t& bytes) { return rocprim::inclusive_scan(tmp, bytes, in, out, n, op, s); };
}
template <class In, class Out> auto prim_exclusive_sum(In in, Out out, size_t n, hipStream_t s) {
  using T = typename std::iterator_traits<Out>::value_type;
  return prim_exclusive_scan(in, out, T(0), n, rocprim::plus<T>(), s);
}
template <class In, class Out> auto prim_inclusive_sum(In in, Out out, size_t n, hipStream_t s) {
  return prim_inclusive_scan(in, out, n, rocprim::plus<typename std::iterator_traits<Out>::value_type>(), s);
}

inline unsigned key_bits(uint32_t v) {      // bits that hold 0 .. v
  unsigned b = 1;
  while (b < 32 && (1ull << b) <= (unsigned long long)v) ++b;
  return b;
}

template <class T> __global__ __launch_bounds__(PRIM_THREADS) void k_iota(T* __restrict__ a, size_t n) {      // a[i] = i
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] = (T)i;
}
// offsets[k] = first sorted position of label k; a label nobody carries keeps what its entry held
template <class T> __global__ __launch_bounds__(PRIM_THREADS) void k_run_offsets(const T* __restrict__ labels_sorted, size_t n, T* __restrict__ offsets) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const T l = labels_sorted[i];
    if (i == 0 || labels_sorted[i - 1] != l) offsets[l] = (T)i;
  }
}

// labels[0 .. n) hold 0 .. n_labels (n_labels: "no group", sorted behind every group).  members[] = the indices 0 .. n - 1 sorted stably by
// label: every group's members in ascending index; offsets[k] = where group k begins, offsets[n_labels] (preset to n) = where the
// unlabelled indices begin.  iota / labels_sorted: n words of scratch each, the caller's; the sort's temporary comes from the pool.
template <class T> hipError_t group_by_label(cilhip::DevPool& pool, hipStream_t s, T* labels, size_t n, T n_labels, T* iota, T* labels_sorted, T* members, T* offsets) {
  hipLaunchKernelGGL(k_iota<T>, dim3(prim_blocks(n)), dim3(PRIM_THREADS), 0, s, iota, n);
  hipError_t e = prim_run(pool, prim_sort_pairs(labels, labels_sorted, iota, members, n, 0u, key_bits(n_labels), s));
  if (e != hipSuccess) return e;
  const T n_as_t = (T)n;
  if ((e = hipMemcpyAsync(offsets + n_labels, &n_as_t, sizeof(T), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(k_run_offsets<T>, dim3(prim_blocks(n)), dim3(PRIM_THREADS), 0, s, (const T*)labels_sorted, n, offsets);
  return hipSuccess;
}

// counts[0 .. nblocks) -> their exclusive sums in place, the total in *total.  One lane; nblocks <= 1024
template <class T> __global__ void k_scan_counts(T* counts, int nblocks, T* total) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    T run = 0;
    for (int g = 0; g < nblocks; ++g) { const T c = counts[g]; counts[g] = run; run += c; }
    *total = run;
  }
}

// ---- device side --------------------------------------------------------------------------------------------------------------------
// Lanes of the block before this one among those whose `flag` holds, and the block's number of them in *total.  Every lane of a block of
// THREADS calls it (it synchronises the block); ranks ascend with threadIdx.x, so writing at base + rank keeps the block's order.
template <int THREADS> __device__ __forceinline__ uint32_t block_rank(bool flag, uint32_t* total) {
  __shared__ uint32_t s_cnt[THREADS / 64];
  const unsigned long long mask = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  __syncthreads();      // (a second call: the first one's readers are done)
  if (lane == 0) s_cnt[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull)), sum = 0;
  for (uint32_t v = 0; v < wave; ++v) before += s_cnt[v];
#pragma unroll
  for (int v = 0; v < THREADS / 64; ++v) sum += s_cnt[v];
  *total = sum;
  return before;
}

// A slot of the list whose length is *cursor, for every lane whose `flag` holds (the value means nothing elsewhere): the wave's first such
// lane takes the wave's slots with one atomicAdd.  Slots within a wave ascend with the lane; the order of the waves is the atomics'.
__device__ __forceinline__ unsigned int wave_append(bool flag, unsigned int* cursor) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long b = __ballot(flag);
  if (!b) return 0u;
  const int first = __ffsll((long long)b) - 1;
  unsigned int base = 0;
  if ((int)lane == first) base = atomicAdd(cursor, (unsigned int)__popcll(b));
  base = (unsigned int)__shfl((int)base, first, 64);
  return base + (unsigned int)__popcll(b & ((1ull << lane) - 1ull));
}

}  // namespace

// components_device.hpp -- what the connected-component units (components.hip: 3-D over the grid and over given lists; components_nd.hip:
// 1 to 16 dimensions) share: the clause record, the lock-free union-find over original indices with its memory-model argument
// (DESIGN.md section 11.5), and everything after the hook step -- cc_finish: flatten, seed marks, sizes, keep flags, ranks, labels, member
// lists.  Included by .hip files only; everything has internal linkage.
// Memory model: inside a hook kernel a load of parent[] may be stale; a stale value is the entry's former value, i.e. the point itself or a
// former parent, and either is an ancestor-or-self in the same component, with parent[x] <= x always: find may stop early but never leaves
// the component and always terminates; a link succeeds only through a device-scope CAS that sees the entry still naming itself.  Path
// halving only ever replaces a non-root's parent by one of its ancestors.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "internal.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

constexpr int CC_THREADS = 256;

struct CcClauses {
  float radius_sq;
  int use_distance; float max_distance;
  int use_normals; float max_angle; int angle_inclusive;
  int use_colors; float color_thr2;      // fl(color_thresh * color_thresh), formed once on the host
};

// ---- union-find over original indices ---------------------------------------------------------------------------------------
// CILHIP_CC_PLAIN_FIND: plain loads in find (may be served from a stale L1 / another XCD's L2 line); default: relaxed agent-scope
// atomic loads.  CILHIP_CC_NO_HALVING: find without path halving.  (dev A/B builds: NOTEBOOK.md has what was kept and why.)
__device__ __forceinline__ uint32_t cc_load(const uint32_t* p) {
#ifdef CILHIP_CC_PLAIN_FIND
  return *p;
#else
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
__device__ __forceinline__ uint32_t cc_find(uint32_t* parent, uint32_t x) {
  uint32_t p = cc_load(parent + x);
  while (p != x) {
    const uint32_t gp = cc_load(parent + p);
#ifndef CILHIP_CC_NO_HALVING
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // x is not a root and never becomes one again
#endif
    x = p; p = gp;
  }
  return x;
}
// -> the root both end under, as far as this lane knows
__device__ __forceinline__ uint32_t cc_unite(uint32_t* parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = cc_find(parent, a); b = cc_find(parent, b);
    if (a == b) return a;
    const uint32_t hi = max(a, b), lo = min(a, b);
    const uint32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = old; b = lo;      // hi had a parent already (the find stopped on a stale value, or another lane linked it first): go on from there
  }
}

// x x' + (y y' + z z'), every operation rounded (grid_downsample.hip gd_dot)
__device__ __forceinline__ float cc_dot(const F3& a, const F3& b) { return __fadd_rn(__fmul_rn(a.x, b.x), __fadd_rn(__fmul_rn(a.y, b.y), __fmul_rn(a.z, b.z))); }

// ---- everything after the hook step ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CC_THREADS) void k_cc_flatten(const uint32_t* __restrict__ parent, uint32_t* __restrict__ root, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    uint32_t x = (uint32_t)i, p = parent[x];
    while (p != x) { x = p; p = parent[x]; }
    root[i] = x;
  }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_mark_seeds(const uint32_t* __restrict__ root, const uint32_t* __restrict__ seeds, size_t n_seeds, uint32_t* __restrict__ seeded) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_seeds; k += (size_t)gridDim.x * blockDim.x) seeded[root[seeds[k]]] = 1u;
}

// count[r] = members of root r.  One atomic per distinct root of a wave (a cloud that is one component would otherwise send
// every lane's add to the same word).
__global__ __launch_bounds__(CC_THREADS) void k_cc_sizes(const uint32_t* __restrict__ root, size_t n, uint32_t* __restrict__ count) {
  const unsigned lane = threadIdx.x & 63u;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t base = (size_t)blockIdx.x * blockDim.x; base < n; base += stride) {      // (wave-uniform trip count)
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    const uint32_t r = active ? root[i] : 0u;
    unsigned long long todo = __ballot(active);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const uint32_t r0 = (uint32_t)__shfl((int)r, leader, 64);
      const unsigned long long same = __ballot(active && r == r0) & todo;
      if ((int)lane == leader) atomicAdd(count + r0, (uint32_t)__popcll(same));
      todo &= ~same;
    }
  }
}

// key of a kept root: (~size << 32) | root -- ascending keys = size descending, equal sizes by lowest member; everything else: all ones
__global__ __launch_bounds__(CC_THREADS) void k_cc_keys(const uint32_t* __restrict__ root, const uint32_t* __restrict__ count, const uint32_t* __restrict__ seeded, size_t n,
                                                        unsigned long long min_size, unsigned long long max_size, unsigned long long* __restrict__ keys, unsigned int* n_kept) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t base = (size_t)blockIdx.x * blockDim.x; base < n; base += stride) {
    const size_t i = base + threadIdx.x;
    bool kept = false;
    if (i < n) {
      const uint32_t sz = count[i];
      kept = root[i] == (uint32_t)i && (!seeded || seeded[i]) && sz >= min_size && sz <= max_size;
      keys[i] = kept ? (((unsigned long long)(~sz) << 32) | (unsigned long long)i) : ~0ull;
    }
    const unsigned long long b = __ballot(kept);
    if ((threadIdx.x & 63u) == 0 && b) atomicAdd(n_kept, (unsigned int)__popcll(b));
  }
}

__global__ __launch_bounds__(CC_THREADS) void k_cc_rank(const unsigned long long* __restrict__ keys_sorted, uint32_t n_kept, uint32_t* __restrict__ rank) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_kept; p += (size_t)gridDim.x * blockDim.x) rank[(uint32_t)keys_sorted[p]] = (uint32_t)p;
}

// rank[] holds NONE for everything that is not a kept root
__global__ __launch_bounds__(CC_THREADS) void k_cc_labels(const uint32_t* __restrict__ root, const uint32_t* __restrict__ rank, uint32_t n_kept, size_t n, uint32_t* __restrict__ labels) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t r = rank[root[i]];
    labels[i] = r == NONE_U32 ? n_kept : r;
  }
}

static_assert(CC_THREADS == PRIM_THREADS, "the grid-stride kernels here are launched with prim_blocks() blocks");

struct CcOut {
  int mem;
  size_t n;
  unsigned long long min_size, max_size;
  const uint32_t* seeds;      // host array, or null: every point is a seed
  size_t n_seeds;
  uint32_t *labels, *offsets, *members;      // where `mem` says; offsets / members may be null
  size_t* n_segments;
};

// everything after the hook step: parent[] (device, over original indices) -> the caller's outputs
inline int cc_finish(const CcOut& o, DevPool& pool, hipStream_t s, uint32_t* parent) {
  const size_t n = o.n;
  const dim3 grid(prim_blocks(n)), block(CC_THREADS);
  uint32_t *root = nullptr, *count = nullptr, *seeded = nullptr, *rank = nullptr;
  unsigned long long *keys = nullptr, *keys_sorted = nullptr;
  unsigned int* n_kept_d = nullptr;
  ST_CK("connected_components", pool.bytes(&root, n * sizeof(uint32_t)));
  ST_CK("connected_components", pool.bytes(&count, n * sizeof(uint32_t)));
  ST_CK("connected_components", pool.bytes(&keys, n * sizeof(unsigned long long)));
  ST_CK("connected_components", pool.bytes(&keys_sorted, n * sizeof(unsigned long long)));
  ST_CK("connected_components", pool.bytes(&n_kept_d, sizeof(unsigned int)));
  hipLaunchKernelGGL(k_cc_flatten, grid, block, 0, s, (const uint32_t*)parent, root, n);
  if (o.seeds) {
    uint32_t* d_seeds = nullptr;
    ST_CK("connected_components", pool.bytes(&seeded, n * sizeof(uint32_t)));
    ST_CK("connected_components", pool.bytes(&d_seeds, o.n_seeds * sizeof(uint32_t)));
    ST_CK("connected_components", hipMemsetAsync(seeded, 0, n * sizeof(uint32_t), s));
    if (o.n_seeds) {
      ST_CK("connected_components", hipMemcpyAsync(d_seeds, o.seeds, o.n_seeds * sizeof(uint32_t), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(k_cc_mark_seeds, dim3(prim_blocks(o.n_seeds)), block, 0, s, (const uint32_t*)root, (const uint32_t*)d_seeds, o.n_seeds, seeded);
    }
  }
  ST_CK("connected_components", hipMemsetAsync(count, 0, n * sizeof(uint32_t), s));
  ST_CK("connected_components", hipMemsetAsync(n_kept_d, 0, sizeof(unsigned int), s));
  hipLaunchKernelGGL(k_cc_sizes, grid, block, 0, s, (const uint32_t*)root, n, count);
  hipLaunchKernelGGL(k_cc_keys, grid, block, 0, s, (const uint32_t*)root, (const uint32_t*)count, (const uint32_t*)seeded, n, o.min_size, o.max_size, keys, n_kept_d);
  ST_CK("connected_components", hipGetLastError());
  ST_CK("connected_components", prim_run(pool, prim_sort_keys(keys, keys_sorted, n, 0u, 64u, s)));
  unsigned int n_kept = 0;      // the one host round trip of the chain
  ST_CK("connected_components", hipMemcpyAsync(&n_kept, n_kept_d, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  ST_CK("connected_components", hipStreamSynchronize(s));
  rank = count;      // (the sizes are in the keys now)
  ST_CK("connected_components", hipMemsetAsync(rank, 0xFF, n * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_cc_rank, dim3(prim_blocks(n_kept)), block, 0, s, (const unsigned long long*)keys_sorted, (uint32_t)n_kept, rank);
  const bool host = o.mem == CILHIP_MEM_HOST;
  uint32_t* d_labels = o.labels;
  if (host) ST_CK("connected_components", pool.bytes(&d_labels, n * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_cc_labels, grid, block, 0, s, (const uint32_t*)root, (const uint32_t*)rank, (uint32_t)n_kept, n, d_labels);
  ST_CK("connected_components", hipGetLastError());
  if (host) ST_CK("connected_components", hipMemcpyAsync(o.labels, d_labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (o.offsets || o.members) {
    // a stable sort of the point indices by label: every segment's members in ascending index, the unlabelled points behind them
    uint32_t *iota = root, *lab_sorted = reinterpret_cast<uint32_t*>(keys), *d_members = o.members, *d_offsets = o.offsets;      // (roots and unsorted keys are done with)
    if (host || !d_members) ST_CK("connected_components", pool.bytes(&d_members, n * sizeof(uint32_t)));
    if (host || !d_offsets) ST_CK("connected_components", pool.bytes(&d_offsets, ((size_t)n_kept + 1) * sizeof(uint32_t)));
    ST_CK("connected_components", group_by_label(pool, s, d_labels, n, (uint32_t)n_kept, iota, lab_sorted, d_members, d_offsets));
    ST_CK("connected_components", hipGetLastError());
    if (host && o.offsets) ST_CK("connected_components", hipMemcpyAsync(o.offsets, d_offsets, ((size_t)n_kept + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (host && o.members) ST_CK("connected_components", hipMemcpyAsync(o.members, d_members, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  ST_CK("connected_components", hipStreamSynchronize(s));
  *o.n_segments = n_kept;
  return CILHIP_OK;
}

}  // namespace

}  // namespace cilhip

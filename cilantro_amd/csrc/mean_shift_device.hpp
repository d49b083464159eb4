// mean_shift_device.hpp -- what the mean-shift units (mean_shift.hip: 3-D over the grid; mean_shift_nd.hip: 1 to 16 dimensions, exhaustive)
// share: the call record, the shift's parameters, the grouping's state words, and everything after the grouping -- ms_finish: leader
// flags, ranks, labels, member lists, modes, the copies to the caller.  The shift and the grouping rounds differ for good reason (a grid
// walk against a stream over all points) and stay in their units.  Included by .hip files only; everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "internal.hpp"
#include "search_device.hpp"      // wave_sum
#include "stateless.hpp"

namespace cilhip {

namespace {

constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
static_assert(MS_THREADS == PRIM_THREADS, "the grid-stride kernels of both units are launched with prim_blocks() blocks");
// a seed in the grouping: a non-finite seed is a leader from the start (~ nobody: its own cluster)
constexpr uint32_t MS_UNDECIDED = 0u, MS_MEMBER = 1u, MS_LEADER = 2u;

struct MsShift {
  float radius_sq, conv_tol_sq;
  int kind; float coeff;      // corr_weight's: CW_RBF: -0.5 / sigma^2
};

struct MsArgs {
  int device, mem;
  const float* points; size_t n, dim;
  const float* seeds; size_t ns;      // seeds: the caller's array, or `points` (every point is a seed)
  cilhip_ms_params prm;
  float *shifted, *modes;
  uint32_t *labels, *offsets, *members;
  size_t *n_clusters, *iterations;
};

// blocks of `per_block` slots that hold `slots` (slots < 2^32: below 2^24 blocks)
inline unsigned ms_launch(size_t slots, size_t per_block) { return (unsigned)((slots + per_block - 1) / per_block); }

// flags[i] = seed i is a leader, flags[ns] = 0: the exclusive sum over ns + 1 words then ends in the number of leaders
__global__ __launch_bounds__(MS_THREADS) void k_ms_leader_flags(const uint32_t* __restrict__ state, size_t ns, uint32_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= ns; i += (size_t)gridDim.x * blockDim.x) flags[i] = i < ns && state[i] == MS_LEADER ? 1u : 0u;
}
// rank[] = exclusive sum of the leader flags: a leader's rank is its cluster's number
__global__ __launch_bounds__(MS_THREADS) void k_ms_labels(const uint32_t* __restrict__ lead_of, const uint32_t* __restrict__ rank, size_t ns, uint32_t* __restrict__ labels) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (size_t)gridDim.x * blockDim.x) labels[i] = rank[lead_of[i]];
}
// one wave per cluster: lane l sums members l, l + 64, ... in f64, a fixed shuffle tree adds the 64 partials, lane 0 divides by the size
template <int DIM>
__global__ __launch_bounds__(MS_THREADS) void k_ms_modes(const float* __restrict__ cur, const uint32_t* __restrict__ members, const uint32_t* __restrict__ offsets,
                                                         uint32_t n_clusters, float* __restrict__ modes) {
  const unsigned lane = threadIdx.x & 63u;
  const size_t n_waves = (size_t)gridDim.x * MS_WAVES;
  for (size_t c = (size_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6); c < n_clusters; c += n_waves) {
    const uint32_t beg = offsets[c], end = offsets[c + 1];
    double sum[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) sum[a] = 0.0;
    for (uint32_t k = beg + lane; k < end; k += 64u) {
      const float* __restrict__ s = cur + (size_t)members[k] * DIM;
#pragma unroll
      for (int a = 0; a < DIM; ++a) sum[a] += (double)s[a];
    }
    const double size = (double)(end - beg);
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const double t = wave_sum(sum[a]);
      if (lane == 0) modes[c * DIM + a] = (float)(t / size);
    }
  }
}

// Everything after the grouping.  cur: the ns shifted seeds (device, DIM floats each); state / lead_of: what the grouping rounds left
// (state == null: every seed leads its own cluster -- labels are the seed indices, nothing is ranked); list_a / list_b: ns + 1 words of
// scratch each.  Cluster numbers are the ranks of the leaders in ascending index.  *group_ms = the host clock since t_group0, taken after
// the last synchronisation the labels need (the label kernel is in flight).  Writes every output of `a` but *a.iterations.
template <int DIM>
int ms_finish(const char* family, const MsArgs& a, DevPool& pool, hipStream_t s, const float* cur, const uint32_t* state, const uint32_t* lead_of, uint32_t* list_a, uint32_t* list_b,
              double t_group0, double* group_ms) {
  const size_t ns = a.ns;
  const bool host = a.mem == CILHIP_MEM_HOST;
  const dim3 grid(prim_blocks(ns)), block(MS_THREADS);
  uint32_t n_clusters = (uint32_t)ns;
  uint32_t* d_labels = a.labels;
  if (host) ST_CK(family, pool.get(&d_labels, ns));
  if (!state) {
    hipLaunchKernelGGL(k_iota<uint32_t>, grid, block, 0, s, d_labels, ns);
  } else {
    uint32_t *flags = list_a, *rank = list_b;
    hipLaunchKernelGGL(k_ms_leader_flags, dim3(prim_blocks(ns + 1)), block, 0, s, state, ns, flags);
    ST_CK(family, prim_run(pool, prim_exclusive_sum(flags, rank, ns + 1, s)));
    ST_CK(family, hipMemcpyAsync(&n_clusters, rank + ns, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ST_CK(family, hipStreamSynchronize(s));
    hipLaunchKernelGGL(k_ms_labels, grid, block, 0, s, lead_of, (const uint32_t*)rank, ns, d_labels);
  }
  ST_CK(family, hipGetLastError());
  *group_ms = st_now_ms() - t_group0;

  // ---- member lists and modes ----
  if (a.offsets || a.members || a.modes) {
    uint32_t *iota = list_a, *lab_sorted = list_b, *d_members = a.members, *d_offsets = a.offsets;      // (flags and ranks are done with: the stream orders it)
    float* d_modes = a.modes;
    if (host || !d_members) ST_CK(family, pool.get(&d_members, ns));
    if (host || !d_offsets) ST_CK(family, pool.get(&d_offsets, (size_t)n_clusters + 1));
    ST_CK(family, group_by_label(pool, s, d_labels, ns, n_clusters, iota, lab_sorted, d_members, d_offsets));
    if (a.modes) {
      if (host) ST_CK(family, pool.get(&d_modes, (size_t)n_clusters * DIM));
      hipLaunchKernelGGL(k_ms_modes<DIM>, dim3(std::min<unsigned>(ms_launch(n_clusters, MS_WAVES), 4096u)), block, 0, s, cur, (const uint32_t*)d_members, (const uint32_t*)d_offsets,
                         n_clusters, d_modes);
    }
    ST_CK(family, hipGetLastError());
    if (host && a.offsets) ST_CK(family, hipMemcpyAsync(a.offsets, d_offsets, ((size_t)n_clusters + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (host && a.members) ST_CK(family, hipMemcpyAsync(a.members, d_members, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (host && a.modes) ST_CK(family, hipMemcpyAsync(a.modes, d_modes, (size_t)n_clusters * DIM * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  if (host) {
    ST_CK(family, hipMemcpyAsync(a.shifted, cur, ns * DIM * sizeof(float), hipMemcpyDeviceToHost, s));
    ST_CK(family, hipMemcpyAsync(a.labels, d_labels, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  ST_CK(family, hipStreamSynchronize(s));
  *a.n_clusters = n_clusters;
  return CILHIP_OK;
}

}  // namespace

}  // namespace cilhip

// mean_shift_nd.hip -- mean-shift clustering of n x dim float points, 1 <= dim <= 16: cilantro's MeanShift2f / MeanShiftXf
// (clustering/mean_shift.hpp:38-124, :142-164).  DESIGN.md section 22 has the contract in full; it is section 13's (mean_shift.hip) with
// three changes: the distance is rule N1 of section 21 (nd_device.hpp), the step's summation order is stated (M3), and nothing walks a
// grid -- a cell grid does not survive 9 or 16 dimensions, so the shift and the grouping are exhaustive, like k_knn_nd.
//   M1 ball      point j is in seed i's ball iff d2(seed_i, p_j) < radius_sq (strict), radius_sq = fl(radius * radius); a point with a
//                non-finite coordinate is in no ball (its d2 is NaN or +inf)
//   M2 weights   w_j = corr_weight(kind, coeff, d2_j): 1, d2_j or pinned_expf(coeff * d2_j)
//   M3 step      S_a = sum (double)w_j * (double)p_ja, W = sum (double)w_j, new_a = (float)(S_a / W).  The point stream is cut into
//                s = msn_slices(n, n_active) slices of consecutive indices; within a slice the sum ascends by point index, the slices are
//                added in ascending order.  No floating-point atomics.
//   M4 converged d2(old, new) < fl(tol * tol); the seed takes `new` and is never examined again
//   M5 empty     W == 0: the seed becomes NaN on all dim axes, never converges, is never examined again; iterations = max_iter
//   M6 grouping  a ~ b iff d2(s_a, s_b) < fl(cluster_tol * cluster_tol); leaders = the serial first-fit's; clusters numbered by
//                ascending leader index; labels[i] = rank of the lowest leader ~ i; a non-finite seed is a singleton
//   M7 modes     per cluster and axis the f64 sum of the members' shifted seeds (member k in partial k mod 64, a fixed tree) / size
//
// Kernels (all templated on DIM so that N1 unrolls with its exact grouping):
//   k_msn_shift    one active seed per lane, its coordinates in registers, blockIdx.y = slice; the points arrive in ascending index by
//                  wave-uniform loads (no LDS, no barrier); DIM + 1 f64 partials per lane -> part[slice][axis][active position]
//   k_msn_finish   one lane per active seed: adds the slices in ascending order, divides, applies M5 and M4, writes the seed and appends
//                  it to the next active list unless it converged or became NaN (list order affects no value)
//   k_msn_lead / k_msn_claim   one grouping round over the undecided set U (ascending seed index, coordinates packed alongside): a member
//                  of U without a ~-neighbour before it in U is a leader; then a lane per seed streams the round's leaders in ascending
//                  index and keeps the first one it is ~ to.  Every lane owns its seed: no atomics at all.
//   k_msn_modes    one wave per cluster
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "internal.hpp"
#include "mean_shift_nd_host.hpp"
#include "nd_device.hpp"
#include "search_device.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

constexpr int MSN_THREADS = 256;
constexpr int MSN_WAVES = MSN_THREADS / 64;
constexpr uint32_t MSN_UNDECIDED = 0u, MSN_MEMBER = 1u, MSN_LEADER = 2u;
static_assert(MSN_TILE == 4, "k_msn_shift evaluates four candidates together");

struct MsnShift {
  float radius_sq, conv_tol_sq;
  int kind; float coeff;
};

thread_local cilhip_msn_stats g_msn_stats{};

template <int DIM> __device__ __forceinline__ bool msn_finite(const float* __restrict__ p) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < DIM; ++a) ok = ok && fabsf(p[a]) < INFINITY;      // (false for NaN too)
  return ok;
}

// ---- the shift ---------------------------------------------------------------------------------------------------------------------
// one candidate: N1, the one-word test (N2: d2 < radius_sq, false for +inf and NaN), the weight, DIM + 1 accumulations.  A candidate
// outside the ball is branched over, never multiplied by a zero weight: a non-finite row would give 0 * inf = NaN.
template <int DIM>
__device__ __forceinline__ void msn_take(const float* __restrict__ p, float d2, uint32_t rbits, const MsnShift& m, double (&S)[DIM], double& W) {
  if (__float_as_uint(d2) < rbits) {
    const double w = (double)corr_weight(m.kind, m.coeff, d2);
#pragma unroll
    for (int a = 0; a < DIM; ++a) S[a] += w * (double)p[a];      // (each product is exact: 24 x 24 bits)
    W += w;
  }
}

// Block (x, y): the active seeds act[256 x .. 256 x + 255] against the points [y * slice, (y + 1) * slice) (slice: a multiple of MSN_TILE).
// part[(y * (DIM + 1) + a) * n_act + position] = the slice's S_a (a < DIM) or W (a == DIM).
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_shift(const float* __restrict__ pts, uint32_t n, uint32_t slice, const float* __restrict__ cur,
                                                           const uint32_t* __restrict__ act, uint32_t n_act, MsnShift m, double* __restrict__ part) {
  const uint32_t pos = blockIdx.x * MSN_THREADS + threadIdx.x;
  if (pos >= n_act) return;      // (no barrier below)
  NdQuery<DIM> q;
  q.load(cur + (size_t)act[pos] * DIM);
  double S[DIM], W = 0.0;
#pragma unroll
  for (int a = 0; a < DIM; ++a) S[a] = 0.0;
  const uint32_t rbits = __float_as_uint(m.radius_sq);
  const unsigned long long first = (unsigned long long)blockIdx.y * slice;
  const uint32_t end = (uint32_t)min(first + slice, (unsigned long long)n);
  uint32_t j = (uint32_t)min(first, (unsigned long long)n);
  for (; j + MSN_TILE <= end; j += MSN_TILE) {
    const float* __restrict__ p = pts + (size_t)j * DIM;      // wave-uniform
    float d[MSN_TILE];
#pragma unroll
    for (int t = 0; t < (int)MSN_TILE; ++t) d[t] = q.d2(p + t * DIM);
#pragma unroll
    for (int t = 0; t < (int)MSN_TILE; ++t) msn_take<DIM>(p + t * DIM, d[t], rbits, m, S, W);      // ascending index
  }
  for (; j < end; ++j) {
    const float* __restrict__ p = pts + (size_t)j * DIM;
    msn_take<DIM>(p, q.d2(p), rbits, m, S, W);
  }
  double* __restrict__ out = part + (size_t)blockIdx.y * (DIM + 1) * n_act + pos;
#pragma unroll
  for (int a = 0; a < DIM; ++a) out[(size_t)a * n_act] = S[a];
  out[(size_t)DIM * n_act] = W;
}

// One lane per active seed: the slices' partials added in ascending slice order, the division, M5 and M4.
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_finish(const double* __restrict__ part, uint32_t slices, float* cur, const uint32_t* __restrict__ act,
                                                            uint32_t n_act, float conv_tol_sq, uint32_t* __restrict__ next, unsigned int* cursor, unsigned int* nan_flag) {
  const uint32_t pos = blockIdx.x * MSN_THREADS + threadIdx.x;
  const bool live = pos < n_act;
  bool keep = false;
  uint32_t i = 0u;
  if (live) {
    i = act[pos];
    double W = 0.0;
    for (uint32_t y = 0; y < slices; ++y) W += part[((size_t)y * (DIM + 1) + DIM) * n_act + pos];
    float nw[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      double S = 0.0;
      for (uint32_t y = 0; y < slices; ++y) S += part[((size_t)y * (DIM + 1) + a) * n_act + pos];
      nw[a] = (float)(S / W);      // W == 0: S == 0 as well, 0 / 0 = NaN on every axis
    }
    float* seed = cur + (size_t)i * DIM;
    NdQuery<DIM> old;
    old.load(seed);
#pragma unroll
    for (int a = 0; a < DIM; ++a) seed[a] = nw[a];
    if (nw[0] != nw[0]) *nan_flag = 1u;      // (every writer stores the same word)
    else keep = !(old.d2(nw) < conv_tol_sq);
  }
  const unsigned int at = wave_append(keep, cursor);
  if (keep) next[at] = i;
}

// ---- grouping ------------------------------------------------------------------------------------------------------------------
// state: MSN_LEADER for a non-finite seed (~ nobody: its own cluster), MSN_UNDECIDED otherwise; flags[i] = undecided, flags[ns] = 0
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_group_init(const float* __restrict__ cur, size_t ns, uint32_t* __restrict__ state, uint32_t* __restrict__ lead_of,
                                                                uint32_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= ns; i += (size_t)gridDim.x * blockDim.x) {
    if (i == ns) { flags[i] = 0u; continue; }
    const bool und = msn_finite<DIM>(cur + i * DIM);
    state[i] = und ? MSN_UNDECIDED : MSN_LEADER;
    lead_of[i] = und ? NONE_U32 : (uint32_t)i;
    flags[i] = und ? 1u : 0u;
  }
}

// The entries k < n_in whose flag holds, in order: out_idx[at[k]] = idx_in[k] (idx_in null: k itself), out_xyz[at[k]] = xyz_in[k] (DIM floats);
// at[] = the exclusive sum of flags[].
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_pack(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ at, const uint32_t* __restrict__ idx_in,
                                                          const float* __restrict__ xyz_in, size_t n_in, uint32_t* __restrict__ out_idx, float* __restrict__ out_xyz) {
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_in; k += (size_t)gridDim.x * blockDim.x) {
    if (!flags[k]) continue;
    const size_t o = at[k];
    out_idx[o] = idx_in ? idx_in[k] : (uint32_t)k;
#pragma unroll
    for (int a = 0; a < DIM; ++a) out_xyz[o * DIM + a] = xyz_in[k * DIM + a];
  }
}

// A lane per member k of U: it streams U's coordinates from the front (wave-uniform) and stops at the first ~-neighbour (not a leader) or
// at its own position (a leader of this round); the wave leaves when all its lanes have stopped.  U is in ascending seed index, so "before
// it in U" is "a lower index".  lead_flags[k] = leader, lead_flags[n_u] = 0.
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_lead(const float* __restrict__ u_xyz, uint32_t n_u, float tol_sq, uint32_t* __restrict__ lead_flags) {
  const uint32_t k = blockIdx.x * MSN_THREADS + threadIdx.x;
  if (k == n_u) lead_flags[k] = 0u;
  const bool live = k < n_u;
  NdQuery<DIM> q;
  q.load(u_xyz + (size_t)(live ? k : 0u) * DIM);
  bool leader = live, running = live;
  for (uint32_t j = 0; ; ++j) {
    running = running && j < k;
    if (!__any(running)) break;
    if (running && q.d2(u_xyz + (size_t)j * DIM) < tol_sq) { leader = false; running = false; }
  }
  if (live) lead_flags[k] = leader ? 1u : 0u;
}

// A lane per seed i: it streams the round's new leaders (ascending index, *n_lead of them) and stops at the first one it is ~ to -- the lowest.
// An undecided seed is decided now (the leader itself: d2 = 0 with its own entry, and no two leaders are ~ each other); a seed decided in an
// earlier round keeps the LOWEST leader index it has met (a leader elected later can have the lower index).
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_claim(const float* __restrict__ cur, uint32_t ns, float tol_sq, const uint32_t* __restrict__ lead_idx,
                                                           const float* __restrict__ lead_xyz, const uint32_t* __restrict__ n_lead, uint32_t* __restrict__ state,
                                                           uint32_t* __restrict__ lead_of) {
  const uint32_t i = blockIdx.x * MSN_THREADS + threadIdx.x;
  const bool live = i < ns;
  const uint32_t n_l = *n_lead;
  NdQuery<DIM> q;
  q.load(cur + (size_t)(live ? i : 0u) * DIM);
  bool running = live;
  uint32_t hit = NONE_U32;
  for (uint32_t j = 0; j < n_l; ++j) {
    if (!__any(running)) break;
    if (running && q.d2(lead_xyz + (size_t)j * DIM) < tol_sq) { hit = lead_idx[j]; running = false; }
  }
  if (hit != NONE_U32) {
    if (state[i] == MSN_UNDECIDED) state[i] = hit == i ? MSN_LEADER : MSN_MEMBER;
    if (hit < lead_of[i]) lead_of[i] = hit;
  }
}

// flags[k] = U[k] is still undecided, flags[n_u] = 0
__global__ __launch_bounds__(MSN_THREADS) void k_msn_undecided(const uint32_t* __restrict__ state, const uint32_t* __restrict__ U, uint32_t n_u, uint32_t* __restrict__ flags) {
  const uint32_t k = blockIdx.x * MSN_THREADS + threadIdx.x;
  if (k <= n_u) flags[k] = k < n_u && state[U[k]] == MSN_UNDECIDED ? 1u : 0u;
}

__global__ __launch_bounds__(MSN_THREADS) void k_msn_leader_flags(const uint32_t* __restrict__ state, size_t ns, uint32_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (size_t)gridDim.x * blockDim.x) flags[i] = state[i] == MSN_LEADER ? 1u : 0u;
}
// rank[] = exclusive sum of the leader flags: a leader's rank is its cluster's number
__global__ __launch_bounds__(MSN_THREADS) void k_msn_labels(const uint32_t* __restrict__ lead_of, const uint32_t* __restrict__ rank, size_t ns, uint32_t* __restrict__ labels) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (size_t)gridDim.x * blockDim.x) labels[i] = rank[lead_of[i]];
}
// one wave per cluster: lane l sums members l, l + 64, ... in f64, a fixed shuffle tree adds the 64 partials, lane 0 divides by the size
template <int DIM>
__global__ __launch_bounds__(MSN_THREADS) void k_msn_modes(const float* __restrict__ cur, const uint32_t* __restrict__ members, const uint32_t* __restrict__ offsets,
                                                           uint32_t n_clusters, float* __restrict__ modes) {
  const unsigned lane = threadIdx.x & 63u;
  const size_t n_waves = (size_t)gridDim.x * MSN_WAVES;
  for (size_t c = (size_t)blockIdx.x * MSN_WAVES + (threadIdx.x >> 6); c < n_clusters; c += n_waves) {
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

inline int msn_blocks(size_t n) { return (int)std::min<size_t>((n + MSN_THREADS - 1) / MSN_THREADS, 2048) + (n == 0); }
inline unsigned msn_launch(size_t slots, size_t per_block) { return (unsigned)((slots + per_block - 1) / per_block); }      // (slots < 2^32: below 2^24 blocks)
double msn_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define MSN_CK(call) ST_CK("mean_shift_nd", call)

struct MsnArgs {
  int device, mem;
  const float* points; size_t n, dim;
  const float* seeds; size_t ns;      // seeds: the caller's array, or `points` (every point is a seed)
  cilhip_ms_params prm;
  float *shifted, *modes;
  uint32_t *labels, *offsets, *members;
  size_t *n_clusters, *iterations;
};

// the exclusive sum of flags[0 .. count] (count + 1 words: the last one becomes the number of flags that hold) and that number on the host.
// The scan's temporary is taken from the pool once and again only when a call asks for more than the block has.
struct MsnScan {
  void* tmp = nullptr;
  size_t cap = 0;
  hipError_t run(DevPool& pool, hipStream_t s, const uint32_t* flags, uint32_t* at, size_t count, unsigned int* total) {
    const auto op = prim_exclusive_sum(flags, at, count + 1, s);
    size_t bytes = 0;
    hipError_t e = op(nullptr, bytes);
    if (e != hipSuccess) return e;
    if (bytes > cap || !tmp) {
      if ((e = pool.bytes(&tmp, bytes)) != hipSuccess) return e;
      cap = bytes;
    }
    bytes = cap;
    if ((e = op(tmp, bytes)) != hipSuccess) return e;
    if (!total) return hipSuccess;
    if ((e = hipMemcpyAsync(total, at + count, sizeof(unsigned int), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    return hipStreamSynchronize(s);
  }
};

template <int DIM> int msn_run(const MsnArgs& a) {
  DevPool pool;
  StreamGuard st;      // (declared last: the stream is drained and destroyed before anything is freed)
  if (const int open = st_open("mean_shift_nd", a.device)) return open;
  MSN_CK(st.create());
  hipStream_t s = st.s;
  const size_t n = a.n, ns = a.ns;
  const bool host = a.mem == CILHIP_MEM_HOST;
  const dim3 block(MSN_THREADS);
  cilhip_msn_stats stats{};

  unsigned int* d_words = nullptr;      // [0] the next active list's cursor, [1] nan flag
  MSN_CK(pool.bytes(&d_words, 2 * sizeof(unsigned int)));
  MSN_CK(hipMemsetAsync(d_words, 0, 2 * sizeof(unsigned int), s));

  // ---- the seeds: shifted in place ----
  float* cur = a.shifted;
  if (host) {
    MSN_CK(pool.get(&cur, ns * DIM));
    MSN_CK(hipMemcpyAsync(cur, a.seeds, ns * DIM * sizeof(float), hipMemcpyHostToDevice, s));
  } else if (cur != a.seeds) {
    MSN_CK(hipMemcpyAsync(cur, a.seeds, ns * DIM * sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  uint32_t *list_a = nullptr, *list_b = nullptr, *state = nullptr, *lead_of = nullptr;
  MSN_CK(pool.get(&list_a, ns + 1));
  MSN_CK(pool.get(&list_b, ns + 1));
  MSN_CK(pool.get(&state, ns));
  MSN_CK(pool.get(&lead_of, ns));

  // ---- the shift passes ----
  size_t it = 0;
  const double t_shift0 = msn_now_ms();
  if (a.prm.max_iter > 0) {
    const float* d_pts = nullptr;
    if (n) MSN_CK(st_stage(pool, s, a.mem, a.points, n * DIM, &d_pts));
    double* part = nullptr;
    MSN_CK(pool.get(&part, msn_part_doubles(n, ns, DIM)));
    hipLaunchKernelGGL(k_iota<uint32_t>, dim3(msn_blocks(ns)), block, 0, s, list_a, ns);
    const MsnShift m{a.prm.kernel_radius * a.prm.kernel_radius, a.prm.convergence_tol * a.prm.convergence_tol, a.prm.kernel_kind,
                     a.prm.kernel_kind == CW_RBF ? -0.5f / (a.prm.kernel_sigma * a.prm.kernel_sigma) : 0.0f};
    unsigned int n_act = (unsigned int)ns;
    while (it < a.prm.max_iter && n_act > 0) {
      const size_t slices = msn_slices(n, n_act), slice = msn_slice_length(n, slices);      // M3: once per pass
      if (it == 0) stats.slices_first = slices;
      stats.slices_last = slices;
      MSN_CK(hipMemsetAsync(d_words, 0, sizeof(unsigned int), s));
      hipLaunchKernelGGL(k_msn_shift<DIM>, dim3(msn_launch(n_act, MSN_THREADS), (unsigned)slices), block, 0, s, d_pts, (uint32_t)n, (uint32_t)slice, (const float*)cur,
                         (const uint32_t*)list_a, (uint32_t)n_act, m, part);
      hipLaunchKernelGGL(k_msn_finish<DIM>, dim3(msn_launch(n_act, MSN_THREADS)), block, 0, s, (const double*)part, (uint32_t)slices, cur, (const uint32_t*)list_a,
                         (uint32_t)n_act, m.conv_tol_sq, list_b, d_words, d_words + 1);
      MSN_CK(hipGetLastError());
      ++it;
      MSN_CK(hipMemcpyAsync(&n_act, d_words, sizeof(unsigned int), hipMemcpyDeviceToHost, s));      // the pass's one readback
      MSN_CK(hipStreamSynchronize(s));
      std::swap(list_a, list_b);
    }
    stats.passes = it;
    if (it < a.prm.max_iter) {      // nobody is active: with a NaN seed the reference would idle through its remaining passes
      unsigned int nan_any = 0;
      MSN_CK(hipMemcpyAsync(&nan_any, d_words + 1, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
      MSN_CK(hipStreamSynchronize(s));
      if (nan_any) it = a.prm.max_iter;
    }
  }
  stats.shift_ms = msn_now_ms() - t_shift0;

  // ---- grouping ----
  const double t_group0 = msn_now_ms();
  const float tol_sq = a.prm.cluster_tol * a.prm.cluster_tol;
  uint32_t n_clusters = 0;
  uint32_t* d_labels = a.labels;
  if (host) MSN_CK(pool.get(&d_labels, ns));
  size_t rounds = 0;
  if (tol_sq == 0.0f) {      // d2 < 0 never holds: every seed is a leader, without the quadratic scan
    hipLaunchKernelGGL(k_iota<uint32_t>, dim3(msn_blocks(ns)), block, 0, s, d_labels, ns);
    MSN_CK(hipGetLastError());
    n_clusters = (uint32_t)ns;
  } else {
    MsnScan scan;
    float *u_a = nullptr, *u_b = nullptr, *lead_xyz = nullptr;
    uint32_t *lead_idx = nullptr, *flags = nullptr, *at = nullptr;
    MSN_CK(pool.get(&flags, ns + 1));
    MSN_CK(pool.get(&at, ns + 1));
    MSN_CK(pool.get(&u_a, ns * DIM));
    MSN_CK(pool.get(&u_b, ns * DIM));
    MSN_CK(pool.get(&lead_xyz, ns * DIM));
    MSN_CK(pool.get(&lead_idx, ns));
    unsigned int n_u = 0;
    hipLaunchKernelGGL(k_msn_group_init<DIM>, dim3(msn_blocks(ns + 1)), block, 0, s, (const float*)cur, ns, state, lead_of, flags);
    MSN_CK(scan.run(pool, s, flags, at, ns, &n_u));
    hipLaunchKernelGGL(k_msn_pack<DIM>, dim3(msn_blocks(ns)), block, 0, s, (const uint32_t*)flags, (const uint32_t*)at, (const uint32_t*)nullptr, (const float*)cur, ns, list_a, u_a);
    MSN_CK(hipGetLastError());
    while (n_u > 0) {
      // this round's leaders, packed in ascending index; their number stays on the device (at[n_u])
      hipLaunchKernelGGL(k_msn_lead<DIM>, dim3(msn_launch((size_t)n_u + 1, MSN_THREADS)), block, 0, s, (const float*)u_a, (uint32_t)n_u, tol_sq, flags);
      MSN_CK(scan.run(pool, s, flags, at, n_u, nullptr));
      hipLaunchKernelGGL(k_msn_pack<DIM>, dim3(msn_blocks(n_u)), block, 0, s, (const uint32_t*)flags, (const uint32_t*)at, (const uint32_t*)list_a, (const float*)u_a, (size_t)n_u,
                         lead_idx, lead_xyz);
      hipLaunchKernelGGL(k_msn_claim<DIM>, dim3(msn_launch(ns, MSN_THREADS)), block, 0, s, (const float*)cur, (uint32_t)ns, tol_sq, (const uint32_t*)lead_idx, (const float*)lead_xyz,
                         (const uint32_t*)(at + n_u), state, lead_of);
      // U without the seeds the round decided, in order
      unsigned int n_next = 0;
      hipLaunchKernelGGL(k_msn_undecided, dim3(msn_launch((size_t)n_u + 1, MSN_THREADS)), block, 0, s, (const uint32_t*)state, (const uint32_t*)list_a, (uint32_t)n_u, flags);
      MSN_CK(hipGetLastError());
      MSN_CK(scan.run(pool, s, flags, at, n_u, &n_next));
      hipLaunchKernelGGL(k_msn_pack<DIM>, dim3(msn_blocks(n_u)), block, 0, s, (const uint32_t*)flags, (const uint32_t*)at, (const uint32_t*)list_a, (const float*)u_a, (size_t)n_u,
                         list_b, u_b);
      MSN_CK(hipGetLastError());
      std::swap(list_a, list_b);
      std::swap(u_a, u_b);
      n_u = n_next;
      if (++rounds > ns) return st_fail(CILHIP_ERR_HIP, "mean_shift_nd", "the grouping did not finish");      // (every round decides the first member of U: never met)
    }
    // cluster numbers = ranks of the leaders
    unsigned int n_lead = 0;
    hipLaunchKernelGGL(k_msn_leader_flags, dim3(msn_blocks(ns)), block, 0, s, (const uint32_t*)state, ns, flags);
    MSN_CK(hipMemsetAsync(flags + ns, 0, sizeof(uint32_t), s));
    MSN_CK(scan.run(pool, s, flags, at, ns, &n_lead));
    n_clusters = n_lead;
    hipLaunchKernelGGL(k_msn_labels, dim3(msn_blocks(ns)), block, 0, s, (const uint32_t*)lead_of, (const uint32_t*)at, ns, d_labels);
    MSN_CK(hipGetLastError());
  }
  stats.group_ms = msn_now_ms() - t_group0;      // (host clock up to the last synchronisation; the label kernel is in flight)
  stats.rounds = rounds;

  // ---- member lists and modes ----
  if (a.offsets || a.members || a.modes) {
    uint32_t *iota = list_a, *lab_sorted = list_b, *d_members = a.members, *d_offsets = a.offsets;      // (the lists are done with)
    float* d_modes = a.modes;
    if (host || !d_members) MSN_CK(pool.get(&d_members, ns));
    if (host || !d_offsets) MSN_CK(pool.get(&d_offsets, (size_t)n_clusters + 1));
    MSN_CK(group_by_label(pool, s, d_labels, ns, n_clusters, iota, lab_sorted, d_members, d_offsets));
    if (a.modes) {
      if (host) MSN_CK(pool.get(&d_modes, (size_t)n_clusters * DIM));
      hipLaunchKernelGGL(k_msn_modes<DIM>, dim3(std::min<unsigned>(msn_launch(n_clusters, MSN_WAVES), 4096u)), block, 0, s, (const float*)cur, (const uint32_t*)d_members,
                         (const uint32_t*)d_offsets, n_clusters, d_modes);
    }
    MSN_CK(hipGetLastError());
    if (host && a.offsets) MSN_CK(hipMemcpyAsync(a.offsets, d_offsets, ((size_t)n_clusters + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (host && a.members) MSN_CK(hipMemcpyAsync(a.members, d_members, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    if (host && a.modes) MSN_CK(hipMemcpyAsync(a.modes, d_modes, (size_t)n_clusters * DIM * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  if (host) {
    MSN_CK(hipMemcpyAsync(a.shifted, cur, ns * DIM * sizeof(float), hipMemcpyDeviceToHost, s));
    MSN_CK(hipMemcpyAsync(a.labels, d_labels, ns * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  MSN_CK(hipStreamSynchronize(s));
  *a.n_clusters = n_clusters;
  *a.iterations = it;
  g_msn_stats = stats;
  return CILHIP_OK;
}

}  // namespace

}  // namespace cilhip

extern "C" int cilhip_msn_last_stats(cilhip_msn_stats* out) {
  if (!out) return CILHIP_ERR_INVALID;
  *out = cilhip::g_msn_stats;
  return CILHIP_OK;
}

extern "C" int cilhip_mean_shift_nd(int device, const float* points, size_t n, size_t dim, const float* seeds_or_null, size_t n_seeds, int mem, const cilhip_ms_params* params,
                                    float* shifted_seeds_out, uint32_t* labels_out, float* modes_out_or_null, uint32_t* offsets_out_or_null, uint32_t* members_out_or_null,
                                    size_t* n_clusters_out, size_t* iterations_out) {
  using namespace cilhip;
  const NdVerdict v = msn_check(MsnCall{points, n, dim, seeds_or_null, n_seeds, mem, params, shifted_seeds_out, labels_out, n_clusters_out, iterations_out});
  if (v.status) return st_fail(v.status, "mean_shift_nd", v.what);
  st_clear();
  const size_t ns = seeds_or_null ? n_seeds : n;
  if (ns == 0) {      // (without touching a device)
    msn_answer_empty(mem, offsets_out_or_null, n_clusters_out, iterations_out);
    return CILHIP_OK;
  }
  const MsnArgs a{device, mem, points, n, dim, seeds_or_null ? seeds_or_null : points, ns, *params, shifted_seeds_out, modes_out_or_null, labels_out, offsets_out_or_null,
                  members_out_or_null, n_clusters_out, iterations_out};
  try {
#define MSN_RUN(D) return msn_run<D>(a)
    ND_DISPATCH(dim, MSN_RUN)
#undef MSN_RUN
  } catch (...) {      // (out of host memory: never across the C boundary)
    return st_fail(CILHIP_ERR_HIP, "mean_shift_nd", "out of host memory");
  }
  return CILHIP_ERR_INVALID;      // (not reached)
}

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
//   then ms_finish (mean_shift_device.hpp, shared with mean_shift.hip): k_ms_leader_flags, ranks, k_ms_labels, member lists, and
//   k_ms_modes<DIM>, one wave per cluster
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "internal.hpp"
#include "mean_shift_device.hpp"      // what mean_shift.hip shares: MsArgs, MsShift, the state words, ms_finish
#include "mean_shift_nd_host.hpp"
#include "nd_device.hpp"
#include "search_device.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

static_assert(MSN_TILE == 4, "k_msn_shift evaluates four candidates together");

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
__device__ __forceinline__ void msn_take(const float* __restrict__ p, float d2, uint32_t rbits, const MsShift& m, double (&S)[DIM], double& W) {
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
__global__ __launch_bounds__(MS_THREADS) void k_msn_shift(const float* __restrict__ pts, uint32_t n, uint32_t slice, const float* __restrict__ cur,
                                                          const uint32_t* __restrict__ act, uint32_t n_act, MsShift m, double* __restrict__ part) {
  const uint32_t pos = blockIdx.x * MS_THREADS + threadIdx.x;
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
__global__ __launch_bounds__(MS_THREADS) void k_msn_finish(const double* __restrict__ part, uint32_t slices, float* cur, const uint32_t* __restrict__ act,
                                                           uint32_t n_act, float conv_tol_sq, uint32_t* __restrict__ next, unsigned int* cursor, unsigned int* nan_flag) {
  const uint32_t pos = blockIdx.x * MS_THREADS + threadIdx.x;
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
// state: MS_LEADER for a non-finite seed (~ nobody: its own cluster), MS_UNDECIDED otherwise; flags[i] = undecided, flags[ns] = 0
template <int DIM>
__global__ __launch_bounds__(MS_THREADS) void k_msn_group_init(const float* __restrict__ cur, size_t ns, uint32_t* __restrict__ state, uint32_t* __restrict__ lead_of,
                                                               uint32_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i <= ns; i += (size_t)gridDim.x * blockDim.x) {
    if (i == ns) { flags[i] = 0u; continue; }
    const bool und = msn_finite<DIM>(cur + i * DIM);
    state[i] = und ? MS_UNDECIDED : MS_LEADER;
    lead_of[i] = und ? NONE_U32 : (uint32_t)i;
    flags[i] = und ? 1u : 0u;
  }
}

// The entries k < n_in whose flag holds, in order: out_idx[at[k]] = idx_in[k] (idx_in null: k itself), out_xyz[at[k]] = xyz_in[k] (DIM floats);
// at[] = the exclusive sum of flags[].
template <int DIM>
__global__ __launch_bounds__(MS_THREADS) void k_msn_pack(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ at, const uint32_t* __restrict__ idx_in,
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
__global__ __launch_bounds__(MS_THREADS) void k_msn_lead(const float* __restrict__ u_xyz, uint32_t n_u, float tol_sq, uint32_t* __restrict__ lead_flags) {
  const uint32_t k = blockIdx.x * MS_THREADS + threadIdx.x;
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
__global__ __launch_bounds__(MS_THREADS) void k_msn_claim(const float* __restrict__ cur, uint32_t ns, float tol_sq, const uint32_t* __restrict__ lead_idx,
                                                          const float* __restrict__ lead_xyz, const uint32_t* __restrict__ n_lead, uint32_t* __restrict__ state,
                                                          uint32_t* __restrict__ lead_of) {
  const uint32_t i = blockIdx.x * MS_THREADS + threadIdx.x;
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
    if (state[i] == MS_UNDECIDED) state[i] = hit == i ? MS_LEADER : MS_MEMBER;
    if (hit < lead_of[i]) lead_of[i] = hit;
  }
}

// flags[k] = U[k] is still undecided, flags[n_u] = 0
__global__ __launch_bounds__(MS_THREADS) void k_msn_undecided(const uint32_t* __restrict__ state, const uint32_t* __restrict__ U, uint32_t n_u, uint32_t* __restrict__ flags) {
  const uint32_t k = blockIdx.x * MS_THREADS + threadIdx.x;
  if (k <= n_u) flags[k] = k < n_u && state[U[k]] == MS_UNDECIDED ? 1u : 0u;
}

#define MSN_CK(call) ST_CK("mean_shift_nd", call)

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

template <int DIM> int msn_run(const MsArgs& a) {
  DevPool pool;
  StreamGuard st;      // (declared last: the stream is drained and destroyed before anything is freed)
  if (const int open = st_open("mean_shift_nd", a.device)) return open;
  MSN_CK(st.create());
  hipStream_t s = st.s;
  const size_t n = a.n, ns = a.ns;
  const bool host = a.mem == CILHIP_MEM_HOST;
  const dim3 block(MS_THREADS);
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
  const double t_shift0 = st_now_ms();
  if (a.prm.max_iter > 0) {
    const float* d_pts = nullptr;
    if (n) MSN_CK(st_stage(pool, s, a.mem, a.points, n * DIM, &d_pts));
    double* part = nullptr;
    MSN_CK(pool.get(&part, msn_part_doubles(n, ns, DIM)));
    hipLaunchKernelGGL(k_iota<uint32_t>, dim3(prim_blocks(ns)), block, 0, s, list_a, ns);
    const MsShift m{a.prm.kernel_radius * a.prm.kernel_radius, a.prm.convergence_tol * a.prm.convergence_tol, a.prm.kernel_kind,
                     a.prm.kernel_kind == CW_RBF ? -0.5f / (a.prm.kernel_sigma * a.prm.kernel_sigma) : 0.0f};
    unsigned int n_act = (unsigned int)ns;
    while (it < a.prm.max_iter && n_act > 0) {
      const size_t slices = msn_slices(n, n_act), slice = msn_slice_length(n, slices);      // M3: once per pass
      if (it == 0) stats.slices_first = slices;
      stats.slices_last = slices;
      MSN_CK(hipMemsetAsync(d_words, 0, sizeof(unsigned int), s));
      hipLaunchKernelGGL(k_msn_shift<DIM>, dim3(ms_launch(n_act, MS_THREADS), (unsigned)slices), block, 0, s, d_pts, (uint32_t)n, (uint32_t)slice, (const float*)cur,
                         (const uint32_t*)list_a, (uint32_t)n_act, m, part);
      hipLaunchKernelGGL(k_msn_finish<DIM>, dim3(ms_launch(n_act, MS_THREADS)), block, 0, s, (const double*)part, (uint32_t)slices, cur, (const uint32_t*)list_a,
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
  stats.shift_ms = st_now_ms() - t_shift0;

  // ---- grouping ----
  const double t_group0 = st_now_ms();
  const float tol_sq = a.prm.cluster_tol * a.prm.cluster_tol;
  size_t rounds = 0;
  const bool grouped = tol_sq != 0.0f;      // d2 < 0 never holds: every seed is a leader, without the quadratic scan
  if (grouped) {
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
    hipLaunchKernelGGL(k_msn_group_init<DIM>, dim3(prim_blocks(ns + 1)), block, 0, s, (const float*)cur, ns, state, lead_of, flags);
    MSN_CK(scan.run(pool, s, flags, at, ns, &n_u));
    hipLaunchKernelGGL(k_msn_pack<DIM>, dim3(prim_blocks(ns)), block, 0, s, (const uint32_t*)flags, (const uint32_t*)at, (const uint32_t*)nullptr, (const float*)cur, ns, list_a, u_a);
    MSN_CK(hipGetLastError());
    while (n_u > 0) {
      // this round's leaders, packed in ascending index; their number stays on the device (at[n_u])
      hipLaunchKernelGGL(k_msn_lead<DIM>, dim3(ms_launch((size_t)n_u + 1, MS_THREADS)), block, 0, s, (const float*)u_a, (uint32_t)n_u, tol_sq, flags);
      MSN_CK(scan.run(pool, s, flags, at, n_u, nullptr));
      hipLaunchKernelGGL(k_msn_pack<DIM>, dim3(prim_blocks(n_u)), block, 0, s, (const uint32_t*)flags, (const uint32_t*)at, (const uint32_t*)list_a, (const float*)u_a, (size_t)n_u,
                         lead_idx, lead_xyz);
      hipLaunchKernelGGL(k_msn_claim<DIM>, dim3(ms_launch(ns, MS_THREADS)), block, 0, s, (const float*)cur, (uint32_t)ns, tol_sq, (const uint32_t*)lead_idx, (const float*)lead_xyz,
                         (const uint32_t*)(at + n_u), state, lead_of);
      // U without the seeds the round decided, in order
      unsigned int n_next = 0;
      hipLaunchKernelGGL(k_msn_undecided, dim3(ms_launch((size_t)n_u + 1, MS_THREADS)), block, 0, s, (const uint32_t*)state, (const uint32_t*)list_a, (uint32_t)n_u, flags);
      MSN_CK(hipGetLastError());
      MSN_CK(scan.run(pool, s, flags, at, n_u, &n_next));
      hipLaunchKernelGGL(k_msn_pack<DIM>, dim3(prim_blocks(n_u)), block, 0, s, (const uint32_t*)flags, (const uint32_t*)at, (const uint32_t*)list_a, (const float*)u_a, (size_t)n_u,
                         list_b, u_b);
      MSN_CK(hipGetLastError());
      std::swap(list_a, list_b);
      std::swap(u_a, u_b);
      n_u = n_next;
      if (++rounds > ns) return st_fail(CILHIP_ERR_HIP, "mean_shift_nd", "the grouping did not finish");      // (every round decides the first member of U: never met)
    }
  }
  stats.rounds = rounds;
  if (const int rc = ms_finish<DIM>("mean_shift_nd", a, pool, s, cur, grouped ? state : nullptr, lead_of, list_a, list_b, t_group0, &stats.group_ms)) return rc;
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
  const MsArgs a{device, mem, points, n, dim, seeds_or_null ? seeds_or_null : points, ns, *params, shifted_seeds_out, modes_out_or_null, labels_out, offsets_out_or_null,
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

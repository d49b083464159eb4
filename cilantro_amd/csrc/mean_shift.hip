// mean_shift.hip -- mean-shift clustering on the device: cilantro's MeanShift3f (clustering/mean_shift.hpp:38-124 over
// core/common_pair_evaluators.hpp:13-79), the flow of the reference's examples/mean_shift.cpp.
//
// The contract (DESIGN.md section 13 has it in full; every rule cites the reference lines it restates):
//   ball      point j is in seed i's ball iff d2_pinned(seed_i, p_j) < radius_sq (strict), radius_sq = fl(radius * radius); a point with
//             a non-finite coordinate is in no ball                                                        mean_shift.hpp:46, :60
//   weights   w_j = corr_weight(kind, coeff, d2_j): 1, d2_j or pinned_expf(coeff * d2_j)                   :64-66
//   step      S = sum (double)w_j * (double)p_j, W = sum (double)w_j, new = (float)(S / W); fixed summation order, no floating-point
//             atomics: a run is reproducible bit for bit                                                   :61-70
//   converged d2_pinned(old, new) < fl(tol * tol); the seed takes `new` and is never examined again        :71-76
//   empty     W == 0: the seed becomes (NaN, NaN, NaN), never converges, is never examined again; iterations = max_iter
//   grouping  a ~ b iff d2_pinned(s_a, s_b) < fl(cluster_tol * cluster_tol); leaders = the lexicographically first maximal
//             independent set of ~ (the reference's serial first-fit, :84-100); clusters numbered by ascending leader index;
//             labels[i] = rank of the lowest leader ~ i; a NaN seed is a singleton
//   modes     per cluster the f64 sum of the members' shifted seeds / size                                 :102-112
//
// Kernels (every walk over a ball's cells is grid_ball.hpp's: ball_cells, ball_rows):
//   k_points_clean     (grid_ball.hpp) a point with a non-finite coordinate becomes (NaN, NaN, NaN): in no cell, in nobody's ball
//   k_ms_seed_keys     the seeds' starting cells: the sort keys of the first active list
//   k_ms_shift<false>  one lane per active seed, the active list sorted once by the seeds' initial grid cell (a wave's lanes walk the
//                      same cells): many seeds, small balls
//   k_ms_shift<true>   one wave per active seed, the lanes stride over the x-runs of the ball's (z, y) rows, f64 partials per lane and a
//                      fixed __shfl_down tree: few seeds whose balls hold a large part of the cloud
//   both write the new seed and append an unconverged seed to the next active list (one integer atomicAdd per wave).
//   k_ms_group_init / k_ms_lead / k_ms_claim / k_ms_compact   the grouping: U = the finite seeds; per round a seed of U without a
//                      lower-index ~-neighbour in U is a leader (k_ms_lead walks its ball cell by cell and leaves early); a wave per new
//                      leader marks every ~ seed as decided and hands it min(leader index) by an integer atomicMin; U is compacted.
//                      Exact; a chain of leaders needs about one round per two seeds.
//   then ms_finish (mean_shift_device.hpp, shared with mean_shift_nd.hip): k_ms_leader_flags, their ranks (rocPRIM scan), k_ms_labels, a
//   stable rocPRIM sort of the seed indices by label, offsets, and k_ms_modes<3>, one wave per cluster.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "grid_ball.hpp"      // ball_cells / ball_rows, the points-clean step; d2_pinned and query_is_finite (search_device.hpp)
#include "internal.hpp"
#include "mean_shift_device.hpp"      // what mean_shift_nd.hip shares: MsArgs, MsShift, the state words, ms_finish
#include "stateless.hpp"

namespace cilhip {

namespace {

// form 0: one wave per seed from this estimated mean ball population on.  Measured (NOTEBOOK 2026-10-19, profiles/mean_shift_bench.json:
// frame_1 downsampled, 15 531 seeds, time per pass wave / lane): x1.30 at an estimate of 189, x0.79 at 638 -- the crossover is near 380;
// with fewer seeds the wave form wins earlier (1500 seeds: x0.19 at 612), so the constant errs towards the lane form only where both are fast.
constexpr double MS_WAVE_FORM_MIN_BALL = 384.0;

thread_local cilhip_ms_stats g_ms_stats{};

// the grid cell of every seed's starting position (clamped into the grid; 0 for a non-finite seed): the sort key of the first active list
__global__ __launch_bounds__(MS_THREADS) void k_ms_seed_keys(GridDev g, const F3* __restrict__ seeds, size_t ns, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ns; i += (size_t)gridDim.x * blockDim.x) {
    const F3 q = seeds[i];
    uint32_t key = 0u;
    if (query_is_finite(q.x, q.y, q.z)) {
      const int cx = min(max(grid_cell_coord(q.x, g.ox, g.inv_cell), 0), g.nx - 1), cy = min(max(grid_cell_coord(q.y, g.oy, g.inv_cell), 0), g.ny - 1),
                cz = min(max(grid_cell_coord(q.z, g.oz, g.inv_cell), 0), g.nz - 1);
      key = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
  }
}

// One pass over the active seeds act[0 .. n_act).  WAVE: seed = wave index, otherwise seed = lane index.  have_grid == 0: every ball is
// empty (no finite point, or radius_sq == 0).  Writes cur[i]; appends i to next[] unless it converged or became NaN.
template <bool WAVE>
__global__ __launch_bounds__(MS_THREADS) void k_ms_shift(GridDev g, int have_grid, MsShift m, F3* __restrict__ cur, const uint32_t* __restrict__ act, uint32_t n_act,
                                                         uint32_t* __restrict__ next, unsigned int* cursor, unsigned int* nan_flag) {
  const unsigned lane = threadIdx.x & 63u;
  const size_t slot = WAVE ? (size_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6) : (size_t)blockIdx.x * MS_THREADS + threadIdx.x;
  const bool live = slot < n_act;      // (WAVE: the same for a wave's 64 lanes)
  const uint32_t i = live ? act[slot] : 0u;
  F3 q{NAN, NAN, NAN};
  if (live) q = cur[i];
  double sx = 0.0, sy = 0.0, sz = 0.0, sw = 0.0;
  if (live && have_grid && query_is_finite(q.x, q.y, q.z))      // the step's fixed summation order: ball_rows' (per lane when WAVE)
    ball_rows(g, ball_cells(g, q.x, q.y, q.z, m.radius_sq), WAVE ? lane : 0u, WAVE ? 64u : 1u, [&](const float4& p) {
      const float d2 = d2_pinned(q.x, q.y, q.z, p.x, p.y, p.z);
      if (!(d2 < m.radius_sq)) return;
      const double w = (double)corr_weight(m.kind, m.coeff, d2);
      sx += w * (double)p.x; sy += w * (double)p.y; sz += w * (double)p.z;      // (each product is exact: 24 x 24 bits)
      sw += w;
    });
  if (WAVE) { sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); sw = wave_sum(sw); }
  bool keep = false;
  if (live && (!WAVE || lane == 0)) {
    const F3 nw{(float)(sx / sw), (float)(sy / sw), (float)(sz / sw)};      // sw == 0: 0 / 0 = NaN on every axis
    cur[i] = nw;
    if (nw.x != nw.x) *nan_flag = 1u;      // (every writer stores the same word)
    else keep = !(d2_pinned(q.x, q.y, q.z, nw.x, nw.y, nw.z) < m.conv_tol_sq);
  }
  const unsigned int at = wave_append(keep, cursor);
  if (keep) next[at] = i;
}

// ---- grouping ------------------------------------------------------------------------------------------------------------------
// state: MS_LEADER for a non-finite seed (~ nobody: its own cluster), MS_UNDECIDED otherwise; U = the undecided seeds
__global__ __launch_bounds__(MS_THREADS) void k_ms_group_init(const F3* __restrict__ cur, size_t ns, uint32_t* __restrict__ state, uint32_t* __restrict__ lead_of,
                                                              uint32_t* __restrict__ U, unsigned int* cursor) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t base_i = (size_t)blockIdx.x * blockDim.x; base_i < ns; base_i += stride) {      // (wave-uniform trip count)
    const size_t i = base_i + threadIdx.x;
    bool und = false;
    if (i < ns) {
      const F3 q = cur[i];
      und = query_is_finite(q.x, q.y, q.z);
      state[i] = und ? MS_UNDECIDED : MS_LEADER;
      lead_of[i] = und ? NONE_U32 : (uint32_t)i;
    }
    const unsigned int at = wave_append(und, cursor);
    if (und) U[at] = (uint32_t)i;
  }
}

// a seed of U with no lower-index ~-neighbour in U becomes a leader of this round.  state[] is only READ here (k_ms_claim writes it in a
// launch of its own), so every lane sees U as it was when the round began.  A cell's records are in ascending index (build_grid sorts
// stably by cell), so a cell is left at the first index >= i: the lowest seed of a collapsed mode looks at one record of its cell, every
// other one stops at the first record that is still undecided and close.
__global__ __launch_bounds__(MS_THREADS) void k_ms_lead(GridDev g, float tol_sq, const F3* __restrict__ cur, const uint32_t* __restrict__ state, const uint32_t* __restrict__ U,
                                                        uint32_t n_u, uint32_t* __restrict__ new_leaders, unsigned int* cursor) {
  const size_t slot = (size_t)blockIdx.x * MS_THREADS + threadIdx.x;
  bool leader = false;
  uint32_t i = 0u;
  if (slot < n_u) {
    i = U[slot];
    leader = true;
    const F3 q = cur[i];
    const BallCells b = ball_cells(g, q.x, q.y, q.z, tol_sq);      // (walked cell by cell, with the two early exits: not ball_rows)
    for (int z = b.z0; z <= b.z1 && leader; ++z)
      for (int y = b.y0; y <= b.y1 && leader; ++y) {
        const uint32_t row = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx;
        for (int x = b.x0; x <= b.x1 && leader; ++x) {
          const uint32_t beg = g.cell_start[row + x], end = g.cell_start[row + x + 1];
          for (uint32_t k = beg; k < end; ++k) {
            const float4 p = g.pts[k];
            const uint32_t j = __float_as_uint(p.w);
            if (j >= i) break;
            if (state[j] != MS_UNDECIDED) continue;
            if (d2_pinned(q.x, q.y, q.z, p.x, p.y, p.z) < tol_sq) { leader = false; break; }
          }
        }
      }
  }
  const unsigned int at = wave_append(leader, cursor);
  if (leader) new_leaders[at] = i;
}

// one wave per new leader L: every seed ~ L that is still undecided is decided now (a member), and every seed ~ L, decided in this round
// or an earlier one, keeps the LOWEST leader index it has met (a leader elected later can have the lower index).  Two leaders are never ~
// each other, so no leader's word is touched.  *n_leaders is the count k_ms_lead left.
__global__ __launch_bounds__(MS_THREADS) void k_ms_claim(GridDev g, float tol_sq, const F3* __restrict__ cur, uint32_t* state, uint32_t* lead_of,
                                                         const uint32_t* __restrict__ new_leaders, const unsigned int* n_leaders) {
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t n_l = *n_leaders;
  const size_t n_waves = (size_t)gridDim.x * MS_WAVES;
  for (size_t w = (size_t)blockIdx.x * MS_WAVES + (threadIdx.x >> 6); w < n_l; w += n_waves) {
    const uint32_t L = new_leaders[w];
    const F3 q = cur[L];
    if (lane == 0) { state[L] = MS_LEADER; lead_of[L] = L; }
    ball_rows(g, ball_cells(g, q.x, q.y, q.z, tol_sq), lane, 64u, [&](const float4& p) {
      const uint32_t j = __float_as_uint(p.w);
      if (j == L || !(d2_pinned(q.x, q.y, q.z, p.x, p.y, p.z) < tol_sq)) return;
      if (state[j] == MS_UNDECIDED) state[j] = MS_MEMBER;      // (several leaders may store the same word)
      atomicMin(lead_of + j, L);
    });
  }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_compact(const uint32_t* __restrict__ state, const uint32_t* __restrict__ U, uint32_t n_u, uint32_t* __restrict__ next,
                                                           unsigned int* cursor) {
  const size_t slot = (size_t)blockIdx.x * MS_THREADS + threadIdx.x;
  uint32_t i = 0u;
  bool keep = false;
  if (slot < n_u) { i = U[slot]; keep = state[i] == MS_UNDECIDED; }
  const unsigned int at = wave_append(keep, cursor);
  if (keep) next[at] = i;
}

#define MS_CK(call) ST_CK("mean_shift", call)

int ms_run(const MsArgs& a) {
  DevPool pool;
  GridBuildResult pgrid{}, sgrid{};      // over the points; over the shifted seeds
  StreamGuard st;      // (declared last: the stream is drained and destroyed before anything is freed)
  if (const int open = st_open("mean_shift", a.device)) return open;
  MS_CK(st.create());
  hipStream_t s = st.s;
  const size_t n = a.n, ns = a.ns;
  const bool host = a.mem == CILHIP_MEM_HOST;
  const dim3 block(MS_THREADS);
  cilhip_ms_stats stats{};

  // ---- the points' grid ----
  const float radius_sq = a.prm.kernel_radius * a.prm.kernel_radius;
  int have_grid = 0;
  unsigned int* d_words = nullptr;      // [0] U cursor, [1] nan flag, [2], [3] list cursors
  MS_CK(pool.bytes(&d_words, 4 * sizeof(unsigned int)));
  MS_CK(hipMemsetAsync(d_words, 0, 4 * sizeof(unsigned int), s));
  unsigned int n_finite = 0;
  if (n && radius_sq > 0.0f && a.prm.max_iter > 0) {
    const F3* d_pts = nullptr;
    F3* clean = nullptr;
    MS_CK(st_stage(pool, s, a.mem, a.points, n, &d_pts));
    MS_CK(clean_points(pool, s, d_pts, n, &clean, &n_finite));
    if (n_finite) {
      double mean[3];
      // no cell below an eighth of the radius: a ball is at most 17 x 17 rows however dense the cloud
      GRID_CK("mean_shift", "mean_shift", build_grid(reinterpret_cast<const float*>(clean), nullptr, (uint32_t)n, s, &pgrid, mean, 2.0, 1.0, 0.125 * std::sqrt((double)radius_sq)));
      have_grid = 1;
    }
  }

  // ---- the seeds: shifted in place ----
  F3* cur = reinterpret_cast<F3*>(a.shifted);
  if (host) {
    MS_CK(pool.bytes(&cur, ns * sizeof(F3)));
    MS_CK(hipMemcpyAsync(cur, a.seeds, ns * sizeof(F3), hipMemcpyHostToDevice, s));
  } else {
    MS_CK(hipMemcpyAsync(cur, a.seeds, ns * sizeof(F3), hipMemcpyDeviceToDevice, s));
  }
  uint32_t *list_a = nullptr, *list_b = nullptr, *keys = nullptr, *keys_sorted = nullptr;
  MS_CK(pool.get(&list_a, ns + 1));      // (ns + 1 words: ms_finish)
  MS_CK(pool.get(&list_b, ns + 1));
  MS_CK(pool.bytes(&keys, ns * sizeof(uint32_t)));
  MS_CK(pool.bytes(&keys_sorted, ns * sizeof(uint32_t)));

  // ---- the shift passes ----
  size_t it = 0;
  const double t_shift0 = st_now_ms();
  if (a.prm.max_iter > 0) {
    bool wave = a.prm.form == 2;
    if (have_grid) {
      // mean ball population: the density the points see around them (own-cell population / cell volume) times the ball's volume
      const double cell = (double)pgrid.grid.cell, r = std::sqrt((double)radius_sq);
      stats.est_ball = std::min((double)n_finite, pgrid.avg_occupancy / (cell * cell * cell) * (4.18879020478639 * r * r * r));
      if (a.prm.form == 0) wave = stats.est_ball >= MS_WAVE_FORM_MIN_BALL;
      // the first active list: the seeds in the order of their starting cells (a wave's lanes then walk the same cells)
      hipLaunchKernelGGL(k_ms_seed_keys, dim3(prim_blocks(ns)), block, 0, s, pgrid.grid, (const F3*)cur, ns, keys, list_b);
      MS_CK(prim_run(pool, prim_sort_pairs(keys, keys_sorted, list_b, list_a, ns, 0u, key_bits((uint32_t)pgrid.n_cells), s)));
    } else {
      hipLaunchKernelGGL(k_iota<uint32_t>, dim3(prim_blocks(ns)), block, 0, s, list_a, ns);
    }
    stats.form_used = wave ? 2 : 1;
    const MsShift m{radius_sq, a.prm.convergence_tol * a.prm.convergence_tol, a.prm.kernel_kind,
                    a.prm.kernel_kind == CW_RBF ? -0.5f / (a.prm.kernel_sigma * a.prm.kernel_sigma) : 0.0f};
    unsigned int n_act = (unsigned int)ns;
    while (it < a.prm.max_iter && n_act > 0) {
      MS_CK(hipMemsetAsync(d_words + 2, 0, sizeof(unsigned int), s));
      if (wave) hipLaunchKernelGGL(k_ms_shift<true>, dim3(ms_launch(n_act, MS_WAVES)), block, 0, s, pgrid.grid, have_grid, m, cur, (const uint32_t*)list_a, (uint32_t)n_act, list_b, d_words + 2, d_words + 1);
      else hipLaunchKernelGGL(k_ms_shift<false>, dim3(ms_launch(n_act, MS_THREADS)), block, 0, s, pgrid.grid, have_grid, m, cur, (const uint32_t*)list_a, (uint32_t)n_act, list_b, d_words + 2, d_words + 1);
      MS_CK(hipGetLastError());
      ++it;
      MS_CK(hipMemcpyAsync(&n_act, d_words + 2, sizeof(unsigned int), hipMemcpyDeviceToHost, s));      // the pass's one readback
      MS_CK(hipStreamSynchronize(s));
      std::swap(list_a, list_b);
    }
    stats.passes = it;
    if (it < a.prm.max_iter) {      // nobody is active: with a NaN seed the reference would idle through its remaining passes
      unsigned int nan_any = 0;
      MS_CK(hipMemcpyAsync(&nan_any, d_words + 1, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
      MS_CK(hipStreamSynchronize(s));
      if (nan_any) it = a.prm.max_iter;
    }
  }
  stats.shift_ms = st_now_ms() - t_shift0;

  // ---- grouping ----
  const double t_group0 = st_now_ms();
  const float tol_sq = a.prm.cluster_tol * a.prm.cluster_tol;
  uint32_t *state = keys, *lead_of = keys_sorted, *new_leaders = nullptr;      // (the sort keys are done with)
  MS_CK(pool.bytes(&new_leaders, ns * sizeof(uint32_t)));
  MS_CK(hipMemsetAsync(d_words, 0, sizeof(unsigned int), s));
  hipLaunchKernelGGL(k_ms_group_init, dim3(prim_blocks(ns)), block, 0, s, (const F3*)cur, ns, state, lead_of, list_a, d_words);
  unsigned int n_u = 0;
  MS_CK(hipMemcpyAsync(&n_u, d_words, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
  MS_CK(hipStreamSynchronize(s));
  size_t rounds = 0;
  if (n_u) {
    double mean[3];
    // no cell below the tolerance: k_ms_lead visits every cell of a seed's ball, and a collapsed seed set would otherwise be refined to
    // cells a 10^4-th of it (NOTEBOOK 2026-10-19: the grouping of the example's 1500 collapsed seeds took 7.3 s that way)
    GRID_CK("mean_shift", "mean_shift", build_grid(reinterpret_cast<const float*>(cur), nullptr, (uint32_t)ns, s, &sgrid, mean, 2.0, 1.0, std::sqrt((double)tol_sq)));
    while (n_u > 0) {
      MS_CK(hipMemsetAsync(d_words + 2, 0, 2 * sizeof(unsigned int), s));
      hipLaunchKernelGGL(k_ms_lead, dim3(ms_launch(n_u, MS_THREADS)), block, 0, s, sgrid.grid, tol_sq, (const F3*)cur, (const uint32_t*)state, (const uint32_t*)list_a, (uint32_t)n_u,
                         new_leaders, d_words + 2);
      hipLaunchKernelGGL(k_ms_claim, dim3(std::min<unsigned>(ms_launch(n_u, MS_WAVES), 4096u)), block, 0, s, sgrid.grid, tol_sq, (const F3*)cur, state, lead_of,
                         (const uint32_t*)new_leaders, (const unsigned int*)(d_words + 2));
      hipLaunchKernelGGL(k_ms_compact, dim3(ms_launch(n_u, MS_THREADS)), block, 0, s, (const uint32_t*)state, (const uint32_t*)list_a, (uint32_t)n_u, list_b, d_words + 3);
      MS_CK(hipGetLastError());
      MS_CK(hipMemcpyAsync(&n_u, d_words + 3, sizeof(unsigned int), hipMemcpyDeviceToHost, s));
      MS_CK(hipStreamSynchronize(s));
      std::swap(list_a, list_b);
      if (++rounds > ns) return st_fail(CILHIP_ERR_HIP, "mean_shift", "the grouping did not finish");      // (every round decides the lowest undecided seed: never met)
    }
  }
  stats.rounds = rounds;
  if (const int rc = ms_finish<3>("mean_shift", a, pool, s, reinterpret_cast<const float*>(cur), state, lead_of, list_a, list_b, t_group0, &stats.group_ms)) return rc;
  *a.iterations = it;
  g_ms_stats = stats;
  return CILHIP_OK;
}

int ms_refuse(const char* why) { return st_fail(CILHIP_ERR_INVALID, "mean_shift", why); }
bool ms_tolerance(float v) { return std::isfinite(v) && v >= 0.0f; }

}  // namespace

}  // namespace cilhip

extern "C" void cilhip_ms_default_params(cilhip_ms_params* p) {
  if (!p) return;
  *p = cilhip_ms_params{};
  p->convergence_tol = FLT_EPSILON;
  p->kernel_sigma = 1.0f;
}

extern "C" int cilhip_ms_last_stats(cilhip_ms_stats* out) {
  if (!out) return CILHIP_ERR_INVALID;
  *out = cilhip::g_ms_stats;
  return CILHIP_OK;
}

extern "C" int cilhip_mean_shift3f(int device, const float* points, size_t n, const float* seeds_or_null, size_t n_seeds, int mem, const cilhip_ms_params* params,
                                   float* shifted_seeds_out, uint32_t* labels_out, float* modes_out_or_null, uint32_t* offsets_out_or_null, uint32_t* members_out_or_null,
                                   size_t* n_clusters_out, size_t* iterations_out) {
  using namespace cilhip;
  if (!params) return ms_refuse("params is null");
  if (!n_clusters_out) return ms_refuse("n_clusters_out is null");
  if (!iterations_out) return ms_refuse("iterations_out is null");
  if ((unsigned long long)n >= (1ull << 32)) return ms_refuse("n must be below 2^32");
  if ((unsigned long long)n_seeds >= (1ull << 32)) return ms_refuse("n_seeds must be below 2^32");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return ms_refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (n && !points) return ms_refuse("points is null");
  if (n_seeds && !seeds_or_null) return ms_refuse("n_seeds > 0 without a seed array");
  if (!ms_tolerance(params->kernel_radius)) return ms_refuse("kernel_radius must be finite and not negative");
  if (!ms_tolerance(params->cluster_tol)) return ms_refuse("cluster_tol must be finite and not negative");
  if (!ms_tolerance(params->convergence_tol)) return ms_refuse("convergence_tol must be finite and not negative");
  if (params->kernel_kind != CW_UNITY && params->kernel_kind != CW_IDENTITY && params->kernel_kind != CW_RBF) return ms_refuse("kernel_kind: 0 (Unity), 1 (Identity) or 2 (RBF)");
  if (params->kernel_kind == CW_RBF && !(std::isfinite(params->kernel_sigma) && params->kernel_sigma > 0.0f)) return ms_refuse("kernel_sigma must be finite and positive");
  if (params->form < 0 || params->form > 2) return ms_refuse("form: 0 (chosen by the code), 1 (a lane per seed) or 2 (a wave per seed)");
  const size_t ns = seeds_or_null ? n_seeds : n;
  if (ns && !shifted_seeds_out) return ms_refuse("shifted_seeds_out is null");
  if (ns && !labels_out) return ms_refuse("labels_out is null");
  st_clear();
  if (ns == 0) {      // (without touching a device)
    *n_clusters_out = 0;
    *iterations_out = 0;
    if (offsets_out_or_null && mem == CILHIP_MEM_HOST) offsets_out_or_null[0] = 0;
    return CILHIP_OK;
  }
  const MsArgs a{device, mem, points, n, 3, seeds_or_null ? seeds_or_null : points, ns, *params, shifted_seeds_out, modes_out_or_null, labels_out, offsets_out_or_null,
                 members_out_or_null, n_clusters_out, iterations_out};
  try {
    return ms_run(a);
  } catch (...) {      // (out of host memory: never across the C boundary)
    return st_fail(CILHIP_ERR_HIP, "mean_shift", "out of host memory");
  }
}

// components_nd.hip -- connected-component segmentation of n x dim float points, 1 <= dim <= 16: cilantro's
// ConnectedComponentExtraction<float, 2> / <float, Dynamic> with a RadiusNeighborhoodSpecification
// (clustering/connected_component_extraction.hpp:162-265, :394-457 over core/common_pair_evaluators.hpp:92-259).  DESIGN.md section 23
// has the contract in full; it is section 11's (components.hip) with the distance of section 21 and dim-component normals:
//   C1 graph      i ~ j (i != j) iff d2(i, j) < radius_sq (strict; d2 = rule N1, nd_device.hpp) and the selected clauses hold; a row with a
//                 non-finite coordinate has no neighbours (its d2 is NaN or +inf), nor have finite rows whose d2 overflows; radius_sq <= 0:
//                 every point is a singleton
//   C2 clauses    distance and colours as in components.hip; normals: dot = c_0 + (c_1 + (... + c_{dim-1})), c_a = n_ia * n_ja, every
//                 product and sum rounded, folded from the last axis (dim = 3: cc_dot bit for bit); angle = (float)acos((double)dot)
//   C3 output     cc_finish of components_device.hpp, word for word the 3-D entry's
//   C4 repeatable a component's root is its lowest original index whatever happened in between: two runs, and forms 1 and 2, agree
//   C5 refusals   components_nd_host.hpp ccn_check, before a device is opened
// No neighbour list is ever written and no grid is walked (a cell grid does not survive 9 or 16 dimensions):
//   k_ccn_hook    one block per tile pair (I, J), J <= I, of the lower triangle of pairs: a lane keeps one row point of tile I in registers
//                 (NdQuery<DIM>), the block stages column tile J in LDS and every lane streams it -- all lanes read the same column point,
//                 so the reads are broadcasts.  For every column before its row with d2 < radius_sq the lane does what k_cc_hook does:
//                 refresh its own root, skip a pair already under one root before any clause arithmetic or gather, evaluate the clauses,
//                 cc_unite.  Rows and columns are POSITIONS in the point stream; parent[] is over ORIGINAL indices (idx[position]).
//   form 1        the stream is the input: every tile pair of the triangle is tested.
//   form 2        sweep and prune, exact: rows with a non-finite coordinate are dropped (singletons), the others sorted by their coordinate
//                 on the axis of largest extent (k_ccn_extent: integer min / max over order-preserving keys; prim_sort_pairs carrying the
//                 original index; k_ccn_gather) and a column tile wholly R or more before a row tile on that axis is not tested
//                 (components_nd_host.hpp: ccn_prune_radius, ccn_skips and the proof that no skipped pair is an edge).
// The union-find result does not depend on the order the edges arrive in (components_device.hpp), so C4 holds across forms and launches.
// Roots are not cached in LDS next to the column tile: not built, not measured.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/cilantro_hip/c_api.h"
#include "components_device.hpp"
#include "components_nd_host.hpp"
#include "device_prims.hpp"
#include "internal.hpp"
#include "nd_device.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

constexpr int CCN_THREADS = (int)CCN_TILE;
static_assert(CCN_THREADS % 64 == 0 && CCN_THREADS == CC_THREADS, "a row tile is one block of whole waves");

thread_local cilhip_ccn_stats g_ccn_stats{};
thread_local unsigned long long g_ccn_pair_cap = 0;      // 0: CCN_MAX_PAIRS_PER_LAUNCH (cilhip_ccn_set_pair_cap)

// C2's dot product: c_0 + (c_1 + (... + c_{DIM-1})), every operation rounded
template <int DIM> __device__ __forceinline__ float ccn_dot(const float* __restrict__ a, const float* __restrict__ b) {
  float r = __fmul_rn(a[DIM - 1], b[DIM - 1]);
#pragma unroll
  for (int d = DIM - 2; d >= 0; --d) r = __fadd_rn(__fmul_rn(a[d], b[d]), r);
  return r;
}

// components.hip cc_similar with DIM-component normals
template <int DIM>
__device__ __forceinline__ bool ccn_similar(const CcClauses& c, const float* __restrict__ nrm, const F3* __restrict__ rgb, uint32_t i, uint32_t j, float d2) {
  if (c.use_distance && !(d2 < c.max_distance)) return false;
  if (c.use_colors) {
    const F3 a = rgb[i], b = rgb[j];
    const F3 d{__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z)};
    if (!(cc_dot(d, d) < c.color_thr2)) return false;
  }
  if (c.use_normals) {
    const float angle = (float)acos((double)ccn_dot<DIM>(nrm + (size_t)i * DIM, nrm + (size_t)j * DIM));      // NaN for a dot product above 1: every test below is then false
    float v = angle, lim = c.max_angle;
    if (!(c.max_angle >= 0.0f)) {
      const float other = __fsub_rn((float)M_PI, angle);
      v = other < angle ? other : angle;      // std::min
      lim = -c.max_angle;
    }
    return c.angle_inclusive ? v <= lim : v < lim;
  }
  return true;
}

// Block b of a launch: tile pair g = first_pair + b of the flat list.  Row tile I = the last one with begin[I] <= g (begin[]: tiles + 1
// ascending words, begin[tiles] > g), column tile J = first[I] + (g - begin[I]) <= I.  pts: m x DIM, the point stream; idx: the original
// index of every position (null: the position itself).
template <int DIM>
__global__ __launch_bounds__(CCN_THREADS) void k_ccn_hook(const float* __restrict__ pts, const uint32_t* __restrict__ idx, uint32_t m, const unsigned long long* __restrict__ begin,
                                                          const uint32_t* __restrict__ first, uint32_t tiles, unsigned long long first_pair, CcClauses c,
                                                          const float* __restrict__ nrm, const F3* __restrict__ rgb, uint32_t* parent) {
  __shared__ __attribute__((aligned(16))) float s_pts[CCN_THREADS * DIM];
  __shared__ uint32_t s_idx[CCN_THREADS];
  const unsigned long long g = first_pair + blockIdx.x;
  uint32_t lo = 0u, hi = tiles;      // (block-uniform)
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (begin[mid] <= g) lo = mid; else hi = mid;
  }
  const uint32_t I = lo, J = first[I] + (uint32_t)(g - begin[I]);
  const uint32_t col0 = J * (uint32_t)CCN_THREADS, ncol = min((uint32_t)CCN_THREADS, m - col0);      // (J <= I < tiles: col0 < m)
  for (uint32_t k = threadIdx.x; k < ncol * DIM; k += CCN_THREADS) s_pts[k] = pts[(size_t)col0 * DIM + k];
  if (threadIdx.x < ncol) s_idx[threadIdx.x] = idx ? idx[col0 + threadIdx.x] : col0 + threadIdx.x;
  __syncthreads();
  const uint32_t pos = I * (uint32_t)CCN_THREADS + threadIdx.x;
  if (pos >= m) return;      // (no barrier below)
  NdQuery<DIM> q;
  q.load(pts + (size_t)pos * DIM);
  const uint32_t i = idx ? idx[pos] : pos;
  const uint32_t lim = J == I ? threadIdx.x : ncol;      // the columns before this row: every undirected pair once (and never the point itself)
  uint32_t ri = i;      // an ancestor of i (its root when last looked at)
  for (uint32_t k = 0; k < lim; ++k) {
    const float d2 = q.d2(s_pts + k * DIM);
    if (!(d2 < c.radius_sq)) continue;      // (false for NaN and +inf)
    const uint32_t j = s_idx[k];
    ri = cc_find(parent, ri);
    if (cc_find(parent, j) == ri) continue;      // already one component: no clause arithmetic, no gathers
    if (!ccn_similar<DIM>(c, nrm, rgb, i, j, d2)) continue;
    ri = cc_unite(parent, ri, j);
  }
}

// ---- form 2's preparation -------------------------------------------------------------------------------------------------------
template <int DIM> __device__ __forceinline__ bool ccn_finite(const float* __restrict__ p) {
  bool ok = true;
#pragma unroll
  for (int a = 0; a < DIM; ++a) ok = ok && fabsf(p[a]) < INFINITY;      // (false for NaN too)
  return ok;
}

// words[a] = min key, words[DIM + a] = max key of coordinate a over the rows that are finite on every axis (preset: all ones / zero);
// words[2 DIM] = how many such rows.  Integer atomics only, one per wave and word.
template <int DIM> __global__ __launch_bounds__(CCN_THREADS) void k_ccn_extent(const float* __restrict__ pts, size_t n, unsigned int* words) {
  uint32_t kmin[DIM], kmax[DIM], cnt = 0u;
#pragma unroll
  for (int a = 0; a < DIM; ++a) { kmin[a] = 0xFFFFFFFFu; kmax[a] = 0u; }
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float* __restrict__ p = pts + i * DIM;
    if (!ccn_finite<DIM>(p)) continue;
    ++cnt;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      const uint32_t k = ccn_key_bits(__float_as_uint(p[a]));
      kmin[a] = min(kmin[a], k); kmax[a] = max(kmax[a], k);
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    cnt += __shfl_down(cnt, off, 64);
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
      kmin[a] = min(kmin[a], (uint32_t)__shfl_down((int)kmin[a], off, 64));
      kmax[a] = max(kmax[a], (uint32_t)__shfl_down((int)kmax[a], off, 64));
    }
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
#pragma unroll
    for (int a = 0; a < DIM; ++a) { atomicMin(words + a, kmin[a]); atomicMax(words + DIM + a, kmax[a]); }
    atomicAdd(words + 2 * DIM, cnt);
  }
}

// the sort keys: the order-preserving image of coordinate `axis`, CCN_KEY_DROPPED for a row with a non-finite coordinate
template <int DIM> __global__ __launch_bounds__(CCN_THREADS) void k_ccn_sort_keys(const float* __restrict__ pts, size_t n, uint32_t axis, uint32_t* __restrict__ keys) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float* __restrict__ p = pts + i * DIM;
    keys[i] = ccn_finite<DIM>(p) ? ccn_key_bits(__float_as_uint(p[axis])) : CCN_KEY_DROPPED;
  }
}

// sorted[pos] = pts[order[pos]] for the m kept rows; per tile the sweep coordinate of its first and of its last row
template <int DIM>
__global__ __launch_bounds__(CCN_THREADS) void k_ccn_gather(const float* __restrict__ pts, const uint32_t* __restrict__ order, uint32_t m, uint32_t axis, float* __restrict__ sorted,
                                                            float* __restrict__ tile_min, float* __restrict__ tile_max) {
  for (size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pos < m; pos += (size_t)gridDim.x * blockDim.x) {
    const float* __restrict__ p = pts + (size_t)order[pos] * DIM;
#pragma unroll
    for (int a = 0; a < DIM; ++a) sorted[pos * DIM + a] = p[a];
    if (pos % CCN_TILE == 0) tile_min[pos / CCN_TILE] = p[axis];
    if (pos % CCN_TILE == CCN_TILE - 1 || pos == (size_t)m - 1) tile_max[pos / CCN_TILE] = p[axis];
  }
}

#define CCN_CK(call) ST_CK("connected_components_nd", call)

struct CcnArgs {
  int device;
  const float *points, *normals, *rgb;
  size_t dim;
  int form;      // 1 or 2
  unsigned long long pair_cap;
  CcClauses cl;
  CcOut out;
};

template <int DIM> int ccn_run(const CcnArgs& a) {
  DevPool pool;
  StreamGuard st;      // (declared last: the stream is drained and destroyed before anything is freed)
  if (const int open = st_open("connected_components_nd", a.device)) return open;
  CCN_CK(st.create());
  hipStream_t s = st.s;
  const size_t n = a.out.n;
  const dim3 block(CCN_THREADS);
  cilhip_ccn_stats stats{};
  stats.form_used = a.form;

  const double t0 = st_now_ms();
  const float *d_pts = nullptr, *d_nrm = nullptr;
  const F3* d_rgb = nullptr;
  CCN_CK(st_stage(pool, s, a.out.mem, a.points, n * DIM, &d_pts));
  if (a.cl.use_normals) CCN_CK(st_stage(pool, s, a.out.mem, a.normals, n * DIM, &d_nrm));
  if (a.cl.use_colors) CCN_CK(st_stage(pool, s, a.out.mem, a.rgb, n, &d_rgb));
  uint32_t* parent = nullptr;
  CCN_CK(pool.get(&parent, n));
  hipLaunchKernelGGL(k_iota<uint32_t>, dim3(prim_blocks(n)), dim3(CC_THREADS), 0, s, parent, n);      // every point its own root
  CCN_CK(hipGetLastError());

  // ---- the point stream and its plan ----
  const float* stream = d_pts;      // form 1: the input itself
  const uint32_t* stream_idx = nullptr;
  size_t m = n;
  CcnPlan plan;
  std::vector<float> tile_lim;      // form 2: tile minima, then tile maxima (host copies)
  const bool edges = a.cl.radius_sq > 0.0f && n > 1;      // (otherwise nobody has a neighbour)
  if (edges && a.form == 2) {
    unsigned int *d_words = nullptr, words[2 * DIM + 1];
    CCN_CK(pool.get(&d_words, 2 * DIM + 1));
    CCN_CK(hipMemsetAsync(d_words, 0xFF, DIM * sizeof(unsigned int), s));
    CCN_CK(hipMemsetAsync(d_words + DIM, 0, (DIM + 1) * sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_ccn_extent<DIM>, dim3(prim_blocks(n)), block, 0, s, d_pts, n, d_words);
    CCN_CK(hipGetLastError());
    CCN_CK(hipMemcpyAsync(words, d_words, sizeof(words), hipMemcpyDeviceToHost, s));
    CCN_CK(hipStreamSynchronize(s));
    m = words[2 * DIM];
    if (m > 1) {
      const size_t axis = ccn_pick_axis(words, words + DIM, DIM);
      stats.axis = axis;
      uint32_t *keys = nullptr, *keys_sorted = nullptr, *iota = nullptr, *order = nullptr;
      float *sorted = nullptr, *d_lim = nullptr;
      const size_t tiles = ccn_tiles(m);
      CCN_CK(pool.get(&keys, n));
      CCN_CK(pool.get(&keys_sorted, n));
      CCN_CK(pool.get(&iota, n));
      CCN_CK(pool.get(&order, n));
      CCN_CK(pool.get(&sorted, m * DIM));
      CCN_CK(pool.get(&d_lim, 2 * tiles));
      hipLaunchKernelGGL(k_ccn_sort_keys<DIM>, dim3(prim_blocks(n)), block, 0, s, d_pts, n, (uint32_t)axis, keys);
      hipLaunchKernelGGL(k_iota<uint32_t>, dim3(prim_blocks(n)), dim3(CC_THREADS), 0, s, iota, n);
      CCN_CK(hipGetLastError());
      CCN_CK(prim_run(pool, prim_sort_pairs(keys, keys_sorted, iota, order, n, 0u, 32u, s)));      // stable: the dropped rows are the last n - m
      hipLaunchKernelGGL(k_ccn_gather<DIM>, dim3(prim_blocks(m)), block, 0, s, d_pts, (const uint32_t*)order, (uint32_t)m, (uint32_t)axis, sorted, d_lim, d_lim + tiles);
      CCN_CK(hipGetLastError());
      tile_lim.resize(2 * tiles);
      CCN_CK(hipMemcpyAsync(tile_lim.data(), d_lim, 2 * tiles * sizeof(float), hipMemcpyDeviceToHost, s));
      CCN_CK(hipStreamSynchronize(s));
      plan = ccn_plan_pruned(tile_lim.data(), tile_lim.data() + tiles, tiles, ccn_prune_radius(a.cl.radius_sq));
      stream = sorted;
      stream_idx = order;
    }
  } else if (edges) {
    plan = ccn_plan_full(ccn_tiles(m));
  }
  stats.tiles_total = (size_t)plan.total;
  stats.tiles_tested = (size_t)plan.tested;
  CCN_CK(hipStreamSynchronize(s));
  const double t1 = st_now_ms();
  stats.prep_ms = t1 - t0;

  // ---- the hook launches ----
  if (plan.tested) {
    const size_t tiles = plan.first.size();
    unsigned long long* d_begin = nullptr;
    uint32_t* d_first = nullptr;
    CCN_CK(pool.get(&d_begin, tiles + 1));
    CCN_CK(pool.get(&d_first, tiles));
    CCN_CK(hipMemcpyAsync(d_begin, plan.begin.data(), (tiles + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    CCN_CK(hipMemcpyAsync(d_first, plan.first.data(), tiles * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    const unsigned long long per = ccn_tile_pairs_per_launch(a.pair_cap), launches = ccn_launches(plan.tested, per);
    for (unsigned long long k = 0; k < launches; ++k) {
      const unsigned long long at = k * per, count = std::min(per, plan.tested - at);
      hipLaunchKernelGGL(k_ccn_hook<DIM>, dim3((unsigned)count), block, 0, s, stream, stream_idx, (uint32_t)m, (const unsigned long long*)d_begin, (const uint32_t*)d_first,
                         (uint32_t)tiles, at, a.cl, d_nrm, d_rgb, parent);
      CCN_CK(hipGetLastError());
    }
    stats.launches = (size_t)launches;
    CCN_CK(hipStreamSynchronize(s));
  }
  const double t2 = st_now_ms();
  stats.hook_ms = t2 - t1;

  if (const int rc = cc_finish(a.out, pool, s, parent)) return rc;
  stats.finish_ms = st_now_ms() - t2;
  g_ccn_stats = stats;
  return CILHIP_OK;
}

}  // namespace

}  // namespace cilhip

extern "C" int cilhip_ccn_last_stats(cilhip_ccn_stats* out) {
  if (!out) return CILHIP_ERR_INVALID;
  *out = cilhip::g_ccn_stats;
  return CILHIP_OK;
}

extern "C" void cilhip_ccn_set_pair_cap(size_t max_pairs_per_launch) { cilhip::g_ccn_pair_cap = max_pairs_per_launch; }

extern "C" int cilhip_connected_components_nd(int device, const float* points, const float* normals_or_null, const float* rgb_or_null, size_t n, size_t dim, int mem,
                                              const cilhip_cc_params* params, int form, const uint32_t* seeds_or_null, size_t n_seeds, uint32_t* labels_out,
                                              uint32_t* offsets_out_or_null, uint32_t* members_out_or_null, size_t* n_segments_out) {
  using namespace cilhip;
  const NdVerdict v = ccn_check(CcnCall{points, normals_or_null, rgb_or_null, n, dim, mem, params, form, seeds_or_null, n_seeds, labels_out, n_segments_out});
  if (v.status) return st_fail(v.status, "connected_components_nd", v.what);
  st_clear();
  if (n == 0) {      // (without touching a device)
    ccn_answer_empty(mem, offsets_out_or_null, n_segments_out);
    return CILHIP_OK;
  }
  CcnArgs a{};
  a.device = device; a.points = points; a.normals = normals_or_null; a.rgb = rgb_or_null; a.dim = dim;
  a.form = ccn_form(form, n);
  a.pair_cap = g_ccn_pair_cap;
  a.cl.radius_sq = params->radius_sq;
  a.cl.use_distance = params->use_distance != 0; a.cl.max_distance = params->max_distance;
  a.cl.use_normals = params->use_normals != 0; a.cl.max_angle = params->max_angle; a.cl.angle_inclusive = params->angle_inclusive != 0;
  a.cl.use_colors = params->use_colors != 0; a.cl.color_thr2 = params->color_thresh * params->color_thresh;
  a.out = CcOut{mem, n, (unsigned long long)params->min_segment_size, (unsigned long long)params->max_segment_size, seeds_or_null, n_seeds,
                labels_out, offsets_out_or_null, members_out_or_null, n_segments_out};
  try {
#define CCN_RUN(D) return ccn_run<D>(a)
    ND_DISPATCH(dim, CCN_RUN)
#undef CCN_RUN
  } catch (...) {      // (out of host memory: never across the C boundary)
    return st_fail(CILHIP_ERR_HIP, "connected_components_nd", "out of host memory");
  }
  return CILHIP_ERR_INVALID;      // (not reached)
}

// components.hip -- connected-component segmentation on the device: cilantro's ConnectedComponentExtraction3f
// (clustering/connected_component_extraction.hpp:162-265 over core/common_pair_evaluators.hpp:84-259 and
// clustering/clustering_base.hpp:7-18), the consumer of the radius search in the reference's
// examples/connected_component_extraction.cpp.
//
// The contract (DESIGN.md section 11 has it in full; every rule cites the reference lines it restates):
//   graph     i ~ j (i != j) iff d2(i, j) < radius_sq (strict; d2 = ((dx*dx)+(dy*dy))+(dz*dz), search_device.hpp's d2_pinned) and the
//             similarity clauses hold                                                   connected_component_extraction.hpp:201-204
//   clauses   distance: d2 < max_distance                                               common_pair_evaluators.hpp:100, :159, :185, :243
//             colours:  |c_i - c_j|^2 < fl(color_thresh * color_thresh); |v|^2 = x*x + (y*y + z*z)      :136-141
//             normals:  angle = (float)acos((double)dot), dot = x*x' + (y*y' + z*z'); max_angle >= 0: angle <| max_angle, otherwise
//                       min(angle, (float)M_PI - angle) <| -max_angle; <| is <= for NormalsProximityEvaluator alone (:119-121) and <
//                       in the combined classes (:162-164, :213-215, :247-249): angle_inclusive.  dot > 1 -> NaN -> not similar.
//   output    the connected components (only those holding a seed when a seed list is given), members in ascending index, kept iff
//             min <= size <= max (:246-261), ordered by size descending, equal sizes by lowest member ascending;
//             labels[i] = rank of i's segment, or the number of kept segments                clustering_base.hpp:10-11
//   a point is never its own neighbour and an exact duplicate always is one; a point with a non-finite coordinate has no neighbours;
//   a finite radius_sq <= 0 makes every point a singleton.
//
// The reference runs a serial stack flood fill per seed.  Here: a lock-free union-find over the uniform grid of grid_build.hip, no
// neighbour list is ever written.
//   k_points_clean (grid_ball.hpp) a point with a non-finite coordinate becomes (NaN, NaN, NaN): in no cell, nobody's neighbour
//   k_cc_hook      one lane per point in grid-cell order (neighbouring lanes of a wave scan the same cells); walks the cells the ball
//                  can touch (grid_ball.hpp: ball_cells, ball_rows) and, for every candidate with a SMALLER original index inside the
//                  radius that is not already under the same root and passes the clauses, unites the two.  parent[] is over ORIGINAL
//                  indices; a link is atomicCAS(&parent[hi], hi, lo) with hi > lo, made only on a true root.
//   k_cc_flatten   a launch of its own: root[i] = find(i).  The larger root always goes under the smaller one, so a component's root
//                  is its lowest original index whatever order the atomics landed in: the result is reproducible.
//   the rest       seed marks, sizes (integer atomics, one per distinct root of a wave), keep flags, rocPRIM radix sort of
//                  (~size, root) -> ranks, labels, and a stable rocPRIM sort of the point indices by label -> the member lists.
// The union-find (cc_load / cc_find / cc_unite) and everything from k_cc_flatten on (cc_finish) live in components_device.hpp, which
// components_nd.hip includes too.
// Memory model: inside k_cc_hook a load of parent[] may be stale; a stale value is the entry's former value,
// i.e. the point itself or a former parent, and either is an ancestor-or-self in the same component, with parent[x] <= x always: find
// may stop early but never leaves the component and always terminates; a link succeeds only through a device-scope CAS that sees the
// entry still naming itself.  Path halving only ever replaces a non-root's parent by one of its ancestors.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/cilantro_hip/c_api.h"
#include "components_device.hpp"      // the union-find and cc_finish, shared with components_nd.hip
#include "device_prims.hpp"
#include "grid_ball.hpp"      // ball_cells / ball_rows, the points-clean step; d2_pinned and query_is_finite (search_device.hpp)
#include "internal.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

// the evaluator classes' operator() (common_pair_evaluators.hpp:100, :116-123, :139-141, :158-166, :184-187, :209-217, :242-251)
__device__ __forceinline__ bool cc_similar(const CcClauses& c, const F3* __restrict__ nrm, const F3* __restrict__ rgb, uint32_t i, uint32_t j, float d2) {
  if (c.use_distance && !(d2 < c.max_distance)) return false;
  if (c.use_colors) {
    const F3 a = rgb[i], b = rgb[j];
    const F3 d{__fsub_rn(a.x, b.x), __fsub_rn(a.y, b.y), __fsub_rn(a.z, b.z)};
    if (!(cc_dot(d, d) < c.color_thr2)) return false;
  }
  if (c.use_normals) {
    const float angle = (float)acos((double)cc_dot(nrm[i], nrm[j]));      // NaN for a dot product above 1: every test below is then false
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

__global__ __launch_bounds__(CC_THREADS) void k_cc_hook(GridDev g, CcClauses c, const F3* __restrict__ nrm, const F3* __restrict__ rgb, uint32_t* parent) {
  const size_t pos = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (pos >= g.n) return;
  const float4 q = g.pts[pos];
  const uint32_t i = __float_as_uint(q.w);
  if (!query_is_finite(q.x, q.y, q.z)) return;
  uint32_t ri = i;      // an ancestor of i (its root when last looked at)
  ball_rows(g, ball_cells(g, q.x, q.y, q.z, c.radius_sq), 0u, 1u, [&](const float4& p) {
    const uint32_t j = __float_as_uint(p.w);
    if (j >= i) return;      // every undirected edge once, from its larger end (and never the point itself)
    const float d2 = d2_pinned(q.x, q.y, q.z, p.x, p.y, p.z);
    if (!(d2 < c.radius_sq)) return;
    ri = cc_find(parent, ri);
    if (cc_find(parent, j) == ri) return;      // already one component: no clause arithmetic, no gathers
    if (!cc_similar(c, nrm, rgb, i, j, d2)) return;
    ri = cc_unite(parent, ri, j);
  });
}

// the "given neighbours" overloads (connected_component_extraction.hpp:20-160): CSR lists instead of a search.  One lane per list.
__global__ __launch_bounds__(CC_THREADS) void k_cc_hook_lists(const unsigned long long* __restrict__ offsets, const uint32_t* __restrict__ idx, const unsigned char* __restrict__ keep,
                                                              unsigned long long n_entries, uint32_t n, unsigned int skip_first, uint32_t* parent) {
  const size_t i = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long end = min(offsets[i + 1], n_entries);      // (never past the arrays, whatever the offsets say)
  const unsigned long long beg = min(offsets[i] + skip_first, end);
  uint32_t ri = (uint32_t)i;
  for (unsigned long long e = beg; e < end; ++e) {
    if (keep && !keep[e]) continue;
    const uint32_t j = idx[e];
    if (j >= n || j == (uint32_t)i) continue;      // (the NONE padding of k-NN lists ends here)
    ri = cc_unite(parent, ri, j);
  }
}

int cc_run_fused(int device, const float* xyz, const float* nrm, const float* rgb, const CcClauses& cl, const CcOut& o) {
  DevPool pool;
  GridBuildResult grid{};      // the radius search's grid
  StreamGuard st;      // (declared last: the stream is drained and destroyed before anything is freed)
  if (const int open = st_open("connected_components", device)) return open;
  ST_CK("connected_components", st.create());
  hipStream_t s = st.s;
  const size_t n = o.n;
  const F3* d_in[3] = {nullptr, nullptr, nullptr};
  const float* src[3] = {xyz, cl.use_normals ? nrm : nullptr, cl.use_colors ? rgb : nullptr};
  for (int k = 0; k < 3; ++k)
    if (src[k]) ST_CK("connected_components", st_stage(pool, s, o.mem, src[k], n, &d_in[k]));
  uint32_t* parent = nullptr;
  ST_CK("connected_components", pool.bytes(&parent, n * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_iota<uint32_t>, dim3(prim_blocks(n)), dim3(PRIM_THREADS), 0, s, parent, n);      // every point its own root
  if (cl.radius_sq > 0.0f) {
    F3* clean = nullptr;
    unsigned int n_finite = 0;
    ST_CK("connected_components", clean_points(pool, s, d_in[0], n, &clean, &n_finite));
    if (n_finite > 1) {      // (otherwise nobody has a neighbour)
      double mean[3];
      ST_CK("connected_components", build_grid(reinterpret_cast<const float*>(clean), nullptr, (uint32_t)n, s, &grid, mean, 2.0));
      hipLaunchKernelGGL(k_cc_hook, dim3((unsigned)((n + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, s, grid.grid, cl, d_in[1], d_in[2], parent);
      ST_CK("connected_components", hipGetLastError());
    }
  }
  return cc_finish(o, pool, s, parent);
}

int cc_run_lists(int device, const uint64_t* offsets, const uint32_t* idx, const unsigned char* keep, size_t n_entries, int skip_first, const CcOut& o) {
  DevPool pool;
  StreamGuard st;
  if (const int open = st_open("connected_components", device)) return open;
  ST_CK("connected_components", st.create());
  hipStream_t s = st.s;
  const size_t n = o.n;
  const unsigned long long* d_off = reinterpret_cast<const unsigned long long*>(offsets);
  const uint32_t* d_idx = idx;
  const unsigned char* d_keep = keep;
  if (o.mem == CILHIP_MEM_HOST) {
    unsigned long long* a = nullptr; uint32_t* b = nullptr; unsigned char* c = nullptr;
    ST_CK("connected_components", pool.bytes(&a, (n + 1) * sizeof(unsigned long long)));
    ST_CK("connected_components", hipMemcpyAsync(a, offsets, (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    ST_CK("connected_components", pool.bytes(&b, n_entries * sizeof(uint32_t)));
    if (n_entries) ST_CK("connected_components", hipMemcpyAsync(b, idx, n_entries * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (keep) {
      ST_CK("connected_components", pool.bytes(&c, n_entries));
      if (n_entries) ST_CK("connected_components", hipMemcpyAsync(c, keep, n_entries, hipMemcpyHostToDevice, s));
    }
    d_off = a; d_idx = b; d_keep = c;
  }
  uint32_t* parent = nullptr;
  ST_CK("connected_components", pool.bytes(&parent, n * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_iota<uint32_t>, dim3(prim_blocks(n)), dim3(PRIM_THREADS), 0, s, parent, n);      // every point its own root
  hipLaunchKernelGGL(k_cc_hook_lists, dim3((unsigned)((n + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, s, d_off, d_idx, d_keep, (unsigned long long)n_entries, (uint32_t)n,
                     skip_first ? 1u : 0u, parent);
  ST_CK("connected_components", hipGetLastError());
  return cc_finish(o, pool, s, parent);
}

int cc_refuse(const char* why) { return st_fail(CILHIP_ERR_INVALID, "connected_components", why); }

// the argument rules both entries share; they hold on a machine without a device too.  0: go on, 1: answered (n == 0), < 0: refused
int cc_check_common(size_t n, int mem, const uint32_t* seeds, size_t n_seeds, uint32_t* labels, size_t* n_segments) {
  if (!n_segments) return cc_refuse("n_segments_out is null");
  if ((unsigned long long)n >= (1ull << 32)) return cc_refuse("n must be below 2^32");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return cc_refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (n && !labels) return cc_refuse("labels_out is null");
  if (n_seeds && !seeds) return cc_refuse("n_seeds > 0 without a seed array");
  for (size_t k = 0; k < n_seeds; ++k)
    if (seeds[k] >= n) return cc_refuse("a seed index is not below n");
  return 0;
}

}  // namespace

}  // namespace cilhip

extern "C" void cilhip_cc_default_params(cilhip_cc_params* p) {
  if (!p) return;
  *p = cilhip_cc_params{};
  p->min_segment_size = 1;
  p->max_segment_size = (size_t)-1;
}

extern "C" int cilhip_connected_components3f(int device, const float* xyz, const float* normals_or_null, const float* rgb_or_null, size_t n, int mem, const cilhip_cc_params* params,
                                             const uint32_t* seeds_or_null, size_t n_seeds, uint32_t* labels_out, uint32_t* offsets_out_or_null, uint32_t* members_out_or_null,
                                             size_t* n_segments_out) {
  using namespace cilhip;
  if (!params) return cc_refuse("params is null");
  if (int rc = cc_check_common(n, mem, seeds_or_null, n_seeds, labels_out, n_segments_out)) return rc;
  if (!std::isfinite(params->radius_sq)) return cc_refuse("radius_sq must be finite");
  if (params->use_normals && !normals_or_null) return cc_refuse("a normals clause without the normals array");
  if (params->use_colors && !rgb_or_null) return cc_refuse("a colours clause without the colours array");
  if (n && !xyz) return cc_refuse("points is null");
  st_clear();
  if (n == 0) {      // (without touching a device)
    *n_segments_out = 0;
    if (offsets_out_or_null && mem == CILHIP_MEM_HOST) offsets_out_or_null[0] = 0;
    return CILHIP_OK;
  }
  CcClauses cl{};
  cl.radius_sq = params->radius_sq;
  cl.use_distance = params->use_distance != 0; cl.max_distance = params->max_distance;
  cl.use_normals = params->use_normals != 0; cl.max_angle = params->max_angle; cl.angle_inclusive = params->angle_inclusive != 0;
  cl.use_colors = params->use_colors != 0; cl.color_thr2 = params->color_thresh * params->color_thresh;
  const CcOut o{mem, n, (unsigned long long)params->min_segment_size, (unsigned long long)params->max_segment_size, seeds_or_null, n_seeds,
                labels_out, offsets_out_or_null, members_out_or_null, n_segments_out};
  try {
    return cc_run_fused(device, xyz, normals_or_null, rgb_or_null, cl, o);
  } catch (...) {      // (out of host memory: never across the C boundary)
    return st_fail(CILHIP_ERR_HIP, "connected_components", "out of host memory");
  }
}

extern "C" int cilhip_connected_components_lists(int device, size_t n, const uint64_t* offsets, const uint32_t* idx, const unsigned char* keep_or_null, size_t n_entries,
                                                 int skip_first, int symmetric, int mem, size_t min_segment_size, size_t max_segment_size, const uint32_t* seeds_or_null,
                                                 size_t n_seeds, uint32_t* labels_out, uint32_t* offsets_out_or_null, uint32_t* members_out_or_null, size_t* n_segments_out) {
  using namespace cilhip;
  if (int rc = cc_check_common(n, mem, seeds_or_null, n_seeds, labels_out, n_segments_out)) return rc;
  if (n && !offsets) return cc_refuse("offsets is null");
  if (n_entries && !idx) return cc_refuse("idx is null");
  if (seeds_or_null && !symmetric) {
    return st_fail(CILHIP_ERR_UNSUPPORTED, "connected_components", "a seed list over directed lists (the reference's result then depends on its traversal order): pass symmetric lists or no seeds");
  }
  st_clear();
  if (n == 0) {
    *n_segments_out = 0;
    if (offsets_out_or_null && mem == CILHIP_MEM_HOST) offsets_out_or_null[0] = 0;
    return CILHIP_OK;
  }
  const CcOut o{mem, n, (unsigned long long)min_segment_size, (unsigned long long)max_segment_size, seeds_or_null, n_seeds, labels_out, offsets_out_or_null, members_out_or_null,
                n_segments_out};
  try {
    return cc_run_lists(device, offsets, idx, keep_or_null, n_entries, skip_first, o);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, "connected_components", "out of host memory");
  }
}

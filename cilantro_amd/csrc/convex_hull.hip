// convex_hull.hip -- ConvexHull2f / 3f: the part of a convex hull that scales with the cloud (the rules H1-H5 are
// stated in c_api.h).  Filter and refine: the host orders a candidate list (hull_host.hpp), the device tests every surviving point against
// the candidates' facets, drops what is inside for good and names the farthest point above every facet as a new candidate.
//   k_hull_seed<DIM>   arg-extremes of 14 (8 in 2-D) fixed directions -- the axes and the diagonals, both ways --, M and the non-finite count:
//                      order-independent 64-bit maxima of (value bits, ~index), so a tie goes to the lowest index whatever the schedule
//   k_hull_cull<DIM>   one lane per surviving point, the facets' f64 planes through LDS in tiles of HULL_TILE (every lane reads the same
//                      plane: a broadcast); the point bids for the facet of its largest d > tol with one 64-bit atomicMax
//   k_hull_compact     the survivors in input order: block_rank inside a block, the blocks' offsets from one exclusive scan
//   k_hull_gather<DIM> the candidates' coordinates for the host
// Everything runs in one stream.  No float is ever summed across lanes: two runs agree bit for bit.
#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "hull_host.hpp"
#include "stateless.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <new>
#include <vector>

struct cilhip_hull {
  cilhip_hull_info info;
  std::vector<uint32_t> vertex_point_indices, facet_offsets, facet_indices, facet_neighbors, vertex_facet_offsets, vertex_facets;
  std::vector<float> vertices, halfspaces;
  std::vector<uint64_t> survivors;
};

namespace {

constexpr int HT = 256;
constexpr int HULL_TILE = 1024;      // facets per LDS tile: 32 KB of f64 planes
constexpr int HULL_MAX_DIRS = 14;
constexpr size_t HULL_MAX_N = 0xFFFFFFF0ull;

struct SeedOut {
  unsigned long long best[HULL_MAX_DIRS];
  unsigned int maxabs_bits, nonfinite;
};

// the bits of a float as an unsigned that orders like the float
__device__ __forceinline__ uint32_t ord_bits(float f) {
  const uint32_t b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    v = o > v ? o : v;
  }
  return v;
}

template <int DIM> __global__ __launch_bounds__(HT) void k_hull_seed(const float* __restrict__ x, uint32_t n, SeedOut* __restrict__ out) {
  constexpr int K = DIM == 3 ? 14 : 8;
  unsigned long long best[K];
#pragma unroll
  for (int k = 0; k < K; ++k) best[k] = 0ull;
  uint32_t maxabs = 0u, bad = 0u;
  for (uint64_t i = (uint64_t)blockIdx.x * HT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * HT) {
    const float px = x[i * DIM], py = x[i * DIM + 1], pz = DIM == 3 ? x[i * DIM + 2] : 0.0f;
    if (!(isfinite(px) && isfinite(py) && isfinite(pz))) { ++bad; continue; }
    maxabs = max(maxabs, max(__float_as_uint(fabsf(px)), max(__float_as_uint(fabsf(py)), __float_as_uint(fabsf(pz)))));
    const unsigned long long low = (unsigned long long)(~(uint32_t)i);
    float v[K];
    v[0] = px; v[1] = -px; v[2] = py; v[3] = -py;
    if (DIM == 3) {
      v[4] = pz; v[5] = -pz;
#pragma unroll
      for (int c = 0; c < 8; ++c) v[6 + c] = __fadd_rn(__fadd_rn((c & 1) ? -px : px, (c & 2) ? -py : py), (c & 4) ? -pz : pz);
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[4 + c] = __fadd_rn((c & 1) ? -px : px, (c & 2) ? -py : py);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const unsigned long long key = ((unsigned long long)ord_bits(v[k]) << 32) | low;
      best[k] = key > best[k] ? key : best[k];
    }
  }
  const bool lane0 = (threadIdx.x & 63u) == 0u;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const unsigned long long w = wave_max64(best[k]);
    if (lane0 && w) atomicMax(&out->best[k], w);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    maxabs = max(maxabs, (uint32_t)__shfl_xor((int)maxabs, off, 64));
    bad += (uint32_t)__shfl_xor((int)bad, off, 64);
  }
  if (lane0) {
    if (maxabs) atomicMax(&out->maxabs_bits, maxabs);
    if (bad) atomicAdd(&out->nonfinite, bad);
  }
}

// planes: F x 4 doubles (nx, ny, nz, off).  idx_in == nullptr: the survivors are 0 .. m - 1.  keep[e] = 1 iff entry e goes on (it is outside
// some facet, or keep_all and it is finite); block_counts[b] = the block's number of those.  best[f]: the bid of section 20.
template <int DIM>
__global__ __launch_bounds__(HT) void k_hull_cull(const float* __restrict__ x, const uint32_t* __restrict__ idx_in, uint32_t m, const double* __restrict__ planes, uint32_t F, double tol,
                                                  int keep_all, unsigned long long* __restrict__ best, uint8_t* __restrict__ keep, uint32_t* __restrict__ block_counts) {
  __shared__ double sp[HULL_TILE * 4];
  const uint64_t e = (uint64_t)blockIdx.x * HT + threadIdx.x;
  const bool valid = e < m;
  const uint32_t i = valid ? (idx_in ? idx_in[e] : (uint32_t)e) : 0u;
  float fx = 0.0f, fy = 0.0f, fz = 0.0f;
  if (valid) { fx = x[(uint64_t)i * DIM]; fy = x[(uint64_t)i * DIM + 1]; fz = DIM == 3 ? x[(uint64_t)i * DIM + 2] : 0.0f; }
  const bool live = valid && isfinite(fx) && isfinite(fy) && isfinite(fz);
  const double px = (double)fx, py = (double)fy, pz = (double)fz;
  double dbest = tol;
  uint32_t fbest = 0xFFFFFFFFu;
  for (uint32_t t0 = 0; t0 < F; t0 += HULL_TILE) {
    const uint32_t cnt = min((uint32_t)HULL_TILE, F - t0);
    __syncthreads();      // (the tile before this one has been read)
    for (uint32_t u = threadIdx.x; u < cnt * 4u; u += HT) sp[u] = planes[(uint64_t)t0 * 4u + u];
    __syncthreads();
    if (live) {
      for (uint32_t j = 0; j < cnt; ++j) {
        const double d = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(sp[4 * j], px), __dmul_rn(sp[4 * j + 1], py)), __dmul_rn(sp[4 * j + 2], pz)), sp[4 * j + 3]);
        if (d > dbest) { dbest = d; fbest = t0 + j; }
      }
    }
  }
  const bool outside = live && fbest != 0xFFFFFFFFu;
  if (outside) atomicMax(&best[fbest], ((unsigned long long)ord_bits((float)dbest) << 32) | (unsigned long long)(~i));
  const bool go_on = outside || (keep_all && live);
  if (valid) keep[e] = go_on ? 1 : 0;
  uint32_t total = 0;
  block_rank<HT>(go_on, &total);
  if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(HT) void k_hull_compact(const uint32_t* __restrict__ idx_in, uint32_t m, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ block_offsets,
                                                     uint32_t* __restrict__ idx_out) {
  const uint64_t e = (uint64_t)blockIdx.x * HT + threadIdx.x;
  const bool flag = e < m && keep[e] != 0;
  uint32_t total = 0;
  const uint32_t rank = block_rank<HT>(flag, &total);
  if (flag) idx_out[block_offsets[blockIdx.x] + rank] = idx_in ? idx_in[e] : (uint32_t)e;
}

template <int DIM> __global__ __launch_bounds__(HT) void k_hull_gather(const float* __restrict__ x, const uint32_t* __restrict__ ids, uint32_t cnt, float* __restrict__ out) {
  const uint32_t e = blockIdx.x * HT + threadIdx.x;
  if (e >= cnt) return;
  for (int c = 0; c < DIM; ++c) out[(size_t)e * DIM + c] = x[(uint64_t)ids[e] * DIM + c];
}

void set_empty(cilhip_hull& h, int dim) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  h.info.dim = dim; h.info.is_empty = 1;
  h.info.n_vertices = h.info.n_facets = h.info.n_facet_indices = h.info.n_vertex_facets = 0;
  h.info.n_halfspaces = 2;
  h.info.area = h.info.volume = 0.0;
  for (int c = 0; c < 3; ++c) h.info.interior_point[c] = c < dim ? nan : 0.0f;
  h.halfspaces.assign((size_t)(dim + 1) * 2, 0.0f);      // (1, 0, .., 1) and (-1, 0, .., 1): convex_polytope.hpp:17-24
  h.halfspaces[0] = 1.0f; h.halfspaces[dim] = 1.0f; h.halfspaces[dim + 1] = -1.0f; h.halfspaces[2 * dim + 1] = 1.0f;
  h.facet_offsets.assign(1, 0u);
  h.vertex_facet_offsets.assign(1, 0u);
}

void set_result(cilhip_hull& h, const cilhip::HullResult& r, const std::vector<uint32_t>& cand, const std::vector<double>& P, int dim) {
  const size_t V = r.vertex_ids.size(), F = r.planes.size();
  h.info.dim = dim; h.info.is_empty = 0;
  h.info.n_vertices = V; h.info.n_facets = F; h.info.n_halfspaces = F;
  h.info.n_facet_indices = r.facet_indices.size(); h.info.n_vertex_facets = r.vertex_facets.size();
  h.info.area = r.area; h.info.volume = r.volume;
  for (int c = 0; c < 3; ++c) h.info.interior_point[c] = c < dim ? r.interior[c] : 0.0f;
  h.vertex_point_indices.resize(V);
  h.vertices.resize(V * dim);
  for (size_t k = 0; k < V; ++k) {
    h.vertex_point_indices[k] = cand[r.vertex_ids[k]];
    for (int c = 0; c < dim; ++c) h.vertices[k * dim + c] = (float)P[3 * (size_t)r.vertex_ids[k] + c];      // (exact: the f32 value widened and narrowed)
  }
  h.halfspaces.resize(F * (dim + 1));
  for (size_t k = 0; k < F; ++k) {
    for (int c = 0; c < dim; ++c) h.halfspaces[k * (dim + 1) + c] = (float)r.planes[k].n[c];
    h.halfspaces[k * (dim + 1) + dim] = (float)r.planes[k].off;
  }
  h.facet_offsets = r.facet_offsets; h.facet_indices = r.facet_indices; h.facet_neighbors = r.facet_neighbors;
  h.vertex_facet_offsets = r.vertex_facet_offsets; h.vertex_facets = r.vertex_facets;
}

template <int DIM> int hull_impl(const float* points, size_t n, int mem, bool simplicial, double merge_tol, cilhip_hull& h) {
  const char* F = "convex_hull";
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  cilhip::EventGuard ev0, ev1;
  ST_CK(F, s.create());
  const char* env = std::getenv("CILHIP_HULL_TIMING");
  const bool timing = env && env[0] == '1';
  if (timing) { ST_CK(F, ev0.create()); ST_CK(F, ev1.create()); }
  const float* d_x = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, mem, points, n * (size_t)DIM, &d_x));
  const uint32_t nblocks_all = (uint32_t)((n + HT - 1) / HT);

  // ---- seed
  SeedOut* d_seed = nullptr;
  SeedOut seed;
  ST_CK(F, pool.get(&d_seed, 1));
  ST_CK(F, hipMemsetAsync(d_seed, 0, sizeof(SeedOut), s));
  hipLaunchKernelGGL(k_hull_seed<DIM>, dim3(std::min<uint32_t>(nblocks_all, 1024u)), dim3(HT), 0, s, d_x, (uint32_t)n, d_seed);
  ST_CK(F, hipGetLastError());
  ST_CK(F, hipMemcpyAsync(&seed, d_seed, sizeof(SeedOut), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  h.info.n_nonfinite = seed.nonfinite;
  const size_t n_finite = n - seed.nonfinite;
  if (n_finite < (size_t)DIM + 1) { set_empty(h, DIM); return CILHIP_OK; }
  float maxabs;
  std::memcpy(&maxabs, &seed.maxabs_bits, sizeof(float));
  const double tol = cilhip::hull_tol(merge_tol, (double)maxabs);

  std::vector<uint32_t> cand;      // ascending input indices
  std::vector<double> P;           // their coordinates, 3 each
  std::vector<uint32_t> fresh;
  for (int k = 0; k < (DIM == 3 ? 14 : 8); ++k) if (seed.best[k]) fresh.push_back(~(uint32_t)(seed.best[k] & 0xFFFFFFFFull));

  uint32_t *d_ids = nullptr, *d_a = nullptr, *d_b = nullptr, *d_counts = nullptr, *d_offsets = nullptr;
  float* d_xyz = nullptr;
  uint8_t* d_keep = nullptr;
  double* d_planes = nullptr;
  unsigned long long* d_best = nullptr;
  size_t cap_ids = 0, cap_planes = 0;
  ST_CK(F, pool.get(&d_a, n)); ST_CK(F, pool.get(&d_b, n)); ST_CK(F, pool.get(&d_keep, n));
  ST_CK(F, pool.get(&d_counts, (size_t)nblocks_all + 1)); ST_CK(F, pool.get(&d_offsets, (size_t)nblocks_all + 1));
  std::vector<float> xyz;
  std::vector<unsigned long long> best;

  // adds `fresh` (input indices) to the candidates; false: nothing new
  auto absorb = [&](bool* added) -> int {
    std::sort(fresh.begin(), fresh.end());
    fresh.erase(std::unique(fresh.begin(), fresh.end()), fresh.end());
    std::vector<uint32_t> add;
    std::set_difference(fresh.begin(), fresh.end(), cand.begin(), cand.end(), std::back_inserter(add));
    *added = !add.empty();
    if (add.empty()) return CILHIP_OK;
    if (add.size() > cap_ids) {
      cap_ids = std::max<size_t>(add.size() * 2, 1024);
      ST_CK(F, pool.get(&d_ids, cap_ids)); ST_CK(F, pool.get(&d_xyz, cap_ids * DIM));
    }
    xyz.resize(add.size() * DIM);
    ST_CK(F, hipMemcpyAsync(d_ids, add.data(), add.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_hull_gather<DIM>, dim3((unsigned)((add.size() + HT - 1) / HT)), dim3(HT), 0, s, d_x, (const uint32_t*)d_ids, (uint32_t)add.size(), d_xyz);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(xyz.data(), d_xyz, xyz.size() * sizeof(float), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    // merge, keeping the index order
    std::vector<uint32_t> nc(cand.size() + add.size());
    std::vector<double> nP(3 * nc.size());
    size_t i = 0, j = 0, o = 0;
    while (i < cand.size() || j < add.size()) {
      const bool take_old = j == add.size() || (i < cand.size() && cand[i] < add[j]);
      if (take_old) { nc[o] = cand[i]; for (int c = 0; c < 3; ++c) nP[3 * o + c] = P[3 * i + c]; ++i; }
      else { nc[o] = add[j]; for (int c = 0; c < 3; ++c) nP[3 * o + c] = c < DIM ? (double)xyz[j * DIM + c] : 0.0; ++j; }
      ++o;
    }
    cand.swap(nc); P.swap(nP);
    return CILHIP_OK;
  };

  bool added = false;
  if (const int st = absorb(&added)) return st;
  const uint32_t* d_in = nullptr;      // the survivors (nullptr: all of 0 .. n - 1)
  uint32_t* d_out = d_a;
  size_t m = n;
  cilhip::HullResult r;
  h.info.rounds = 0; h.info.plane_tests = 0; h.info.survivors_first_round = 0; h.info.cull_ms = 0.0;
  for (;;) {
    r = cilhip::hull_build(P.data(), cand.size(), DIM, tol, simplicial);
    if (r.failed) return cilhip::st_fail(CILHIP_ERR_UNSUPPORTED, F, "the candidates' surface could not be ordered (a degenerate merge)");
    const std::vector<cilhip::HullPlane>& planes = r.empty ? r.bootstrap : r.planes;
    const uint32_t nF = (uint32_t)planes.size();
    if (nF == 0 || m == 0) break;
    if (nF > cap_planes) {
      cap_planes = std::max<size_t>((size_t)nF * 2, 1024);
      ST_CK(F, pool.get(&d_planes, cap_planes * 4)); ST_CK(F, pool.get(&d_best, cap_planes));
    }
    static_assert(sizeof(cilhip::HullPlane) == 4 * sizeof(double), "planes travel as 4 doubles");
    ST_CK(F, hipMemcpyAsync(d_planes, planes.data(), (size_t)nF * sizeof(cilhip::HullPlane), hipMemcpyHostToDevice, s));
    ST_CK(F, hipMemsetAsync(d_best, 0, (size_t)nF * sizeof(unsigned long long), s));
    const uint32_t nb = (uint32_t)((m + HT - 1) / HT);
    if (timing) ST_CK(F, hipEventRecord(ev0, s));
    hipLaunchKernelGGL(k_hull_cull<DIM>, dim3(nb), dim3(HT), 0, s, d_x, d_in, (uint32_t)m, (const double*)d_planes, nF, tol, r.empty ? 1 : 0, d_best, d_keep, d_counts);
    if (timing) ST_CK(F, hipEventRecord(ev1, s));
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemsetAsync(d_counts + nb, 0, sizeof(uint32_t), s));
    ST_CK(F, prim_run(pool, prim_exclusive_sum((const uint32_t*)d_counts, d_offsets, (size_t)nb + 1, s)));
    hipLaunchKernelGGL(k_hull_compact, dim3(nb), dim3(HT), 0, s, d_in, (uint32_t)m, (const uint8_t*)d_keep, (const uint32_t*)d_offsets, d_out);
    ST_CK(F, hipGetLastError());
    uint32_t m_next = 0;
    best.resize(nF);
    ST_CK(F, hipMemcpyAsync(&m_next, d_offsets + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipMemcpyAsync(best.data(), d_best, (size_t)nF * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    if (timing) { float ms = 0.0f; ST_CK(F, hipEventElapsedTime(&ms, ev0, ev1)); h.info.cull_ms += (double)ms; }
    h.info.plane_tests += (unsigned long long)m * nF;
    if (h.info.rounds++ == 0) h.info.survivors_first_round = m_next;
    h.survivors.push_back(m_next);
    d_in = d_out;
    d_out = d_out == d_a ? d_b : d_a;
    m = m_next;
    fresh.clear();
    for (uint32_t f = 0; f < nF; ++f) if (best[f]) fresh.push_back(~(uint32_t)(best[f] & 0xFFFFFFFFull));
    if (const int st = absorb(&added)) return st;
    if (!added) break;      // no survivor above any facet (or, never seen, only candidates the builder keeps out): r stands
  }
  if (r.empty) set_empty(h, DIM); else set_result(h, r, cand, P, DIM);
  return CILHIP_OK;
}

}  // namespace

extern "C" {

int cilhip_convex_hull_create(int device, const float* points, size_t n, size_t dim, int mem, int simplicial_facets, double merge_tol, cilhip_hull** out, cilhip_hull_info* info) {
  const char* F = "convex_hull";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (out) *out = nullptr;
  if (!out || !info) return refuse("out or info is NULL");
  if (!points && n != 0) return refuse("points is NULL");
  if (dim != 2 && dim != 3) return refuse("dim must be 2 or 3");
  if (n >= HULL_MAX_N) return refuse("n must lie below 2^32 - 16");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (!(merge_tol >= 0.0) || !std::isfinite(merge_tol)) return refuse("merge_tol must be finite and not negative");
  cilhip::st_clear();
  cilhip_hull* h = new (std::nothrow) cilhip_hull();
  if (!h) return cilhip::st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  std::memset(&h->info, 0, sizeof(h->info));
  h->info.facet_tile = HULL_TILE;
  int st = CILHIP_OK;
  try {
    if (n == 0) {
      set_empty(*h, (int)dim);
    } else {
      st = cilhip::st_open(F, device);
      if (st == CILHIP_OK) st = dim == 3 ? hull_impl<3>(points, n, mem, simplicial_facets != 0, merge_tol, *h) : hull_impl<2>(points, n, mem, simplicial_facets != 0, merge_tol, *h);
    }
  } catch (const std::bad_alloc&) {
    st = cilhip::st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  } catch (...) {
    st = cilhip::st_fail(CILHIP_ERR_HIP, F, "unexpected exception");
  }
  if (st != CILHIP_OK) { delete h; return st; }
  *info = h->info;
  *out = h;
  return CILHIP_OK;
}

int cilhip_convex_hull_get(const cilhip_hull* h, uint32_t* vertex_point_indices, float* vertices, float* halfspaces, uint32_t* facet_offsets, uint32_t* facet_indices,
                           uint32_t* facet_neighbors, uint32_t* vertex_facet_offsets, uint32_t* vertex_facets, uint64_t* survivors_per_round) {
  if (!h) return cilhip::st_fail(CILHIP_ERR_INVALID, "convex_hull_get", "hull is NULL");
  auto put = [](auto* dst, const auto& v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
  put(vertex_point_indices, h->vertex_point_indices); put(vertices, h->vertices); put(halfspaces, h->halfspaces); put(facet_offsets, h->facet_offsets);
  put(facet_indices, h->facet_indices); put(facet_neighbors, h->facet_neighbors); put(vertex_facet_offsets, h->vertex_facet_offsets); put(vertex_facets, h->vertex_facets);
  put(survivors_per_round, h->survivors);
  return CILHIP_OK;
}

void cilhip_convex_hull_destroy(cilhip_hull* h) { delete h; }

}  // extern "C"

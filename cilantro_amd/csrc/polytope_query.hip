// polytope_query.hip -- the point queries of ConvexPolytope and SpaceRegion (the rules Q1, Q2 are stated in c_api.h):
// n points against the facets of one or several polytopes.
//   k_poly_distances<DIM>  out[k * n + i] = v of halfspace k at point i; the halfspaces through LDS in tiles, one lane per point
//   k_poly_inside<DIM>     inside any polytope?  One lane per point, the current polytope's halfspaces through LDS in tiles (every lane reads
//                          the same one: a broadcast); a lane stops at its first failing halfspace, a block skips a polytope's remaining
//                          tiles once none of its lanes is still in, and the remaining polytopes once all of them are inside.
//                          Writes the mask, or (COUNT) the block's number of inside points
//   k_poly_indices         the inside points' indices in ascending order: block_rank and the scanned block counts
// v is ((h0 x + h1 y) + h2 z) + h3 in f32 with every rounding written out.
#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "stateless.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <new>

namespace {

constexpr int QT = 256;
constexpr int QTILE = 1024;      // halfspaces per LDS tile: 16 KB
constexpr size_t Q_MAX_N = 0xFFFFFFF0ull;

template <int DIM> __device__ __forceinline__ float q_value(const float* __restrict__ h, float x, float y, float z) {
  float v = __fadd_rn(__fmul_rn(h[0], x), __fmul_rn(h[1], y));
  if (DIM == 3) v = __fadd_rn(v, __fmul_rn(h[2], z));
  return __fadd_rn(v, h[DIM]);
}

template <int DIM>
__global__ __launch_bounds__(QT) void k_poly_distances(const float* __restrict__ hs, uint32_t F, const float* __restrict__ x, uint32_t n, float* __restrict__ out) {
  __shared__ float sh[QTILE * (DIM + 1)];
  const uint64_t i = (uint64_t)blockIdx.x * QT + threadIdx.x;
  const bool valid = i < n;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (valid) { px = x[i * DIM]; py = x[i * DIM + 1]; pz = DIM == 3 ? x[i * DIM + 2] : 0.0f; }
  for (uint32_t t0 = 0; t0 < F; t0 += QTILE) {
    const uint32_t cnt = min((uint32_t)QTILE, F - t0);
    __syncthreads();
    for (uint32_t u = threadIdx.x; u < cnt * (DIM + 1); u += QT) sh[u] = hs[(uint64_t)t0 * (DIM + 1) + u];
    __syncthreads();
    if (valid)
      for (uint32_t j = 0; j < cnt; ++j) out[(uint64_t)(t0 + j) * n + i] = q_value<DIM>(sh + j * (DIM + 1), px, py, pz);
  }
}

template <int DIM, bool COUNT>
__global__ __launch_bounds__(QT) void k_poly_inside(const float* __restrict__ hs, const uint32_t* __restrict__ poly_offsets, uint32_t n_polys, const float* __restrict__ x, uint32_t n,
                                                    float neg_offset, uint8_t* __restrict__ mask, uint32_t* __restrict__ block_counts) {
  __shared__ float sh[QTILE * (DIM + 1)];
  const uint64_t i = (uint64_t)blockIdx.x * QT + threadIdx.x;
  const bool valid = i < n;
  float px = 0.0f, py = 0.0f, pz = 0.0f;
  if (valid) { px = x[i * DIM]; py = x[i * DIM + 1]; pz = DIM == 3 ? x[i * DIM + 2] : 0.0f; }
  bool inside = false;
  for (uint32_t p = 0; p < n_polys; ++p) {
    if (!__syncthreads_or(valid && !inside)) break;      // every point of the block is inside already
    bool in = valid && !inside;
    const uint32_t f0 = poly_offsets[p], f1 = poly_offsets[p + 1];
    for (uint32_t t0 = f0; t0 < f1; t0 += QTILE) {
      if (!__syncthreads_or(in)) break;                  // nobody is still in this polytope (also: the tile before this one has been read)
      const uint32_t cnt = min((uint32_t)QTILE, f1 - t0);
      for (uint32_t u = threadIdx.x; u < cnt * (DIM + 1); u += QT) sh[u] = hs[(uint64_t)t0 * (DIM + 1) + u];
      __syncthreads();
      if (in)
        for (uint32_t j = 0; j < cnt; ++j)
          if (q_value<DIM>(sh + j * (DIM + 1), px, py, pz) > neg_offset) { in = false; break; }
    }
    inside = inside || in;
  }
  if (COUNT) {
    uint32_t total = 0;
    block_rank<QT>(inside, &total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
  }
  if (valid) mask[i] = inside ? 1 : 0;
}

__global__ __launch_bounds__(QT) void k_poly_indices(const uint8_t* __restrict__ mask, uint32_t n, const uint32_t* __restrict__ block_offsets, uint32_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * QT + threadIdx.x;
  const bool flag = i < n && mask[i] != 0;
  uint32_t total = 0;
  const uint32_t rank = block_rank<QT>(flag, &total);
  if (flag) out[block_offsets[blockIdx.x] + rank] = (uint32_t)i;
}

struct QArgs {
  const char* family;
  const float* hs;
  const uint32_t* poly_offsets;
  size_t n_polys;
  const float* points;
  size_t n, dim;
  int mem;
};

int q_check(const QArgs& a, bool need_offsets) {
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, a.family, what); };
  if (need_offsets && !a.poly_offsets) return refuse("poly_offsets is NULL");
  if (!a.points && a.n != 0) return refuse("points is NULL");
  if (a.dim != 2 && a.dim != 3) return refuse("dim must be 2 or 3");
  if (a.n >= Q_MAX_N) return refuse("n must lie below 2^32 - 16");
  if (a.mem != CILHIP_MEM_HOST && a.mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (need_offsets) {
    if (a.n_polys >= Q_MAX_N) return refuse("n_polytopes must lie below 2^32 - 16");
    if (a.poly_offsets[0] != 0) return refuse("poly_offsets must ascend from 0");
    for (size_t p = 0; p < a.n_polys; ++p) if (a.poly_offsets[p + 1] < a.poly_offsets[p]) return refuse("poly_offsets must ascend from 0");
    if (a.poly_offsets[a.n_polys] != 0 && !a.hs) return refuse("halfspaces is NULL");
  }
  return CILHIP_OK;
}

// the mask on the device (and, with counts, the blocks' numbers of inside points)
int q_inside(const QArgs& a, cilhip::DevPool& pool, hipStream_t s, float offset, uint8_t* d_mask, uint32_t* d_counts) {
  const char* F = a.family;
  const size_t total_cols = a.poly_offsets[a.n_polys];
  const float* d_x = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, a.mem, a.points, a.n * a.dim, &d_x));
  float* d_hs = nullptr;
  uint32_t* d_po = nullptr;
  ST_CK(F, pool.get(&d_hs, total_cols * (a.dim + 1))); ST_CK(F, pool.get(&d_po, a.n_polys + 1));
  if (total_cols) ST_CK(F, hipMemcpyAsync(d_hs, a.hs, total_cols * (a.dim + 1) * sizeof(float), hipMemcpyHostToDevice, s));
  ST_CK(F, hipMemcpyAsync(d_po, a.poly_offsets, (a.n_polys + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  const unsigned nb = (unsigned)((a.n + QT - 1) / QT);
  const float neg = -offset;
#define Q_LAUNCH(DIM, COUNT) hipLaunchKernelGGL((k_poly_inside<DIM, COUNT>), dim3(nb), dim3(QT), 0, s, (const float*)d_hs, (const uint32_t*)d_po, (uint32_t)a.n_polys, d_x, (uint32_t)a.n, neg, d_mask, d_counts)
  if (a.dim == 3) { if (d_counts) Q_LAUNCH(3, true); else Q_LAUNCH(3, false); }
  else { if (d_counts) Q_LAUNCH(2, true); else Q_LAUNCH(2, false); }
#undef Q_LAUNCH
  ST_CK(F, hipGetLastError());
  return CILHIP_OK;
}

template <class Fn> int q_guard(const char* family, Fn&& fn) {
  try { return fn(); } catch (const std::bad_alloc&) { return cilhip::st_fail(CILHIP_ERR_HIP, family, "out of host memory"); } catch (...) { return cilhip::st_fail(CILHIP_ERR_HIP, family, "unexpected exception"); }
}

}  // namespace

extern "C" {

int cilhip_polytope_signed_distances(int device, const float* halfspaces, size_t n_facets, const float* points, size_t n, size_t dim, int mem, float* out) {
  const char* F = "polytope_signed_distances";
  const QArgs a{F, halfspaces, nullptr, 0, points, n, dim, mem};
  if (const int st = q_check(a, false)) return st;
  if (n_facets >= Q_MAX_N) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "n_facets must lie below 2^32 - 16");
  if (n_facets != 0 && !halfspaces) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "halfspaces is NULL");
  if (n_facets != 0 && n != 0 && !out) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "out is NULL");
  cilhip::st_clear();
  if (n == 0 || n_facets == 0) return CILHIP_OK;
  if (const int open = cilhip::st_open(F, device)) return open;
  return q_guard(F, [&]() -> int {
    cilhip::DevPool pool;
    cilhip::StreamGuard s;
    ST_CK(F, s.create());
    const float* d_x = nullptr;
    ST_CK(F, cilhip::st_stage(pool, s, mem, points, n * dim, &d_x));
    float *d_hs = nullptr, *d_out = out;
    ST_CK(F, pool.get(&d_hs, n_facets * (dim + 1)));
    ST_CK(F, hipMemcpyAsync(d_hs, halfspaces, n_facets * (dim + 1) * sizeof(float), hipMemcpyHostToDevice, s));
    if (mem != CILHIP_MEM_DEVICE) ST_CK(F, pool.get(&d_out, n_facets * n));
    const unsigned nb = (unsigned)((n + QT - 1) / QT);
    if (dim == 3) hipLaunchKernelGGL(k_poly_distances<3>, dim3(nb), dim3(QT), 0, s, (const float*)d_hs, (uint32_t)n_facets, d_x, (uint32_t)n, d_out);
    else hipLaunchKernelGGL(k_poly_distances<2>, dim3(nb), dim3(QT), 0, s, (const float*)d_hs, (uint32_t)n_facets, d_x, (uint32_t)n, d_out);
    ST_CK(F, hipGetLastError());
    if (mem != CILHIP_MEM_DEVICE) ST_CK(F, hipMemcpyAsync(out, d_out, n_facets * n * sizeof(float), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    return CILHIP_OK;
  });
}

int cilhip_polytopes_interior_mask(int device, const float* halfspaces, const uint32_t* poly_offsets, size_t n_polytopes, const float* points, size_t n, size_t dim, int mem,
                                   float offset, uint8_t* mask_out) {
  const char* F = "polytopes_interior_mask";
  const QArgs a{F, halfspaces, poly_offsets, n_polytopes, points, n, dim, mem};
  if (const int st = q_check(a, true)) return st;
  if (std::isnan(offset)) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "offset is NaN");
  if (n != 0 && !mask_out) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "mask_out is NULL");
  cilhip::st_clear();
  if (n == 0) return CILHIP_OK;
  if (const int open = cilhip::st_open(F, device)) return open;
  return q_guard(F, [&]() -> int {
    cilhip::DevPool pool;
    cilhip::StreamGuard s;
    ST_CK(F, s.create());
    uint8_t* d_mask = mask_out;
    if (mem != CILHIP_MEM_DEVICE) ST_CK(F, pool.get(&d_mask, n));
    if (const int st = q_inside(a, pool, s, offset, d_mask, nullptr)) return st;
    if (mem != CILHIP_MEM_DEVICE) ST_CK(F, hipMemcpyAsync(mask_out, d_mask, n, hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    return CILHIP_OK;
  });
}

int cilhip_polytopes_interior_indices(int device, const float* halfspaces, const uint32_t* poly_offsets, size_t n_polytopes, const float* points, size_t n, size_t dim, int mem,
                                      float offset, uint32_t* indices_out, size_t capacity, size_t* n_out) {
  const char* F = "polytopes_interior_indices";
  const QArgs a{F, halfspaces, poly_offsets, n_polytopes, points, n, dim, mem};
  if (!n_out) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "n_out is NULL");
  if (const int st = q_check(a, true)) return st;
  if (std::isnan(offset)) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "offset is NaN");
  if (capacity != 0 && !indices_out) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "indices_out is NULL");
  cilhip::st_clear();
  if (n == 0) { *n_out = 0; return CILHIP_OK; }
  if (const int open = cilhip::st_open(F, device)) return open;
  return q_guard(F, [&]() -> int {
    cilhip::DevPool pool;
    cilhip::StreamGuard s;
    ST_CK(F, s.create());
    const unsigned nb = (unsigned)((n + QT - 1) / QT);
    uint8_t* d_mask = nullptr;
    uint32_t *d_counts = nullptr, *d_offsets = nullptr;
    ST_CK(F, pool.get(&d_mask, n)); ST_CK(F, pool.get(&d_counts, (size_t)nb + 1)); ST_CK(F, pool.get(&d_offsets, (size_t)nb + 1));
    if (const int st = q_inside(a, pool, s, offset, d_mask, d_counts)) return st;
    ST_CK(F, hipMemsetAsync(d_counts + nb, 0, sizeof(uint32_t), s));
    ST_CK(F, prim_run(pool, prim_exclusive_sum((const uint32_t*)d_counts, d_offsets, (size_t)nb + 1, s)));
    uint32_t rows = 0;
    ST_CK(F, hipMemcpyAsync(&rows, d_offsets + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    *n_out = rows;
    if (capacity == 0) return CILHIP_OK;      // the counting call
    if (rows > capacity) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "capacity is smaller than the number of inside points (*n_out has it; capacity = n always suffices)");
    uint32_t* d_idx = indices_out;
    if (mem != CILHIP_MEM_DEVICE) ST_CK(F, pool.get(&d_idx, rows));
    hipLaunchKernelGGL(k_poly_indices, dim3(nb), dim3(QT), 0, s, (const uint8_t*)d_mask, (uint32_t)n, (const uint32_t*)d_offsets, d_idx);
    ST_CK(F, hipGetLastError());
    if (mem != CILHIP_MEM_DEVICE && rows) ST_CK(F, hipMemcpyAsync(indices_out, d_idx, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    return CILHIP_OK;
  });
}

}  // extern "C"

// grid_ball.hpp -- how a ball meets the uniform grid of grid_build.hip, in one place.  Every feature that visits
// "the points within a fixed radius of a query" goes through it: radius search and radius normals (knn.hip), connected components
// (components.hip), 3-D mean shift (mean_shift.hip).
//   device  ball_cells          the block of cells a ball can touch, never fewer: what makes each of those features exact
//           ball_rows           the walk over that block's records, in a stated order (sums taken in it are reproducible bit for bit)
//           k_points_clean      a cloud's non-finite rows -> (NaN, NaN, NaN), and the number of finite rows
//   host    clean_points        that kernel with its one readback
//           GRID_CK             build_grid under a stateless entry: its refusal of the coordinate range is not a HIP failure
// The distance and the finiteness test are search_device.hpp's d2_pinned and query_is_finite.  The expanding-shell searches (k-NN, the
// 1-NN of the ICP path) are a different algorithm and do not come here; warm.hip's k_self_nn walks a fixed 3 x 3 x 3 block.
// Included by .hip files only; everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

#include "device_prims.hpp"
#include "internal.hpp"
#include "search_device.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

// ---- device side --------------------------------------------------------------------------------------------------------------------
struct BallCells { int x0, x1, y0, y1, z0, z1; };      // inclusive cell ranges, clamped into the grid; empty when some lo > hi

// The cells the ball d2_pinned(q, .) < radius_sq can touch -- never fewer.  The radius is rounded UP (sqrtf and the products below err by
// a few 2^-24, the factor is 2^-20) and widened by g.margin, the grid's own safety margin for bounds formed from cell boxes; the +-1e9
// clamp keeps the float -> int conversion defined for a query far outside the grid.  The caller has tested that q is finite.
__device__ __forceinline__ BallCells ball_cells(const GridDev& g, float qx, float qy, float qz, float radius_sq) {
  const float r = sqrtf(radius_sq) * 1.000001f + g.margin;
  const float BIG = 1.0e9f;
  BallCells b;
  b.x0 = max((int)floorf(fminf(fmaxf((qx - r - g.ox) * g.inv_cell, -BIG), BIG)), 0); b.x1 = min((int)floorf(fminf(fmaxf((qx + r - g.ox) * g.inv_cell, -BIG), BIG)), g.nx - 1);
  b.y0 = max((int)floorf(fminf(fmaxf((qy - r - g.oy) * g.inv_cell, -BIG), BIG)), 0); b.y1 = min((int)floorf(fminf(fmaxf((qy + r - g.oy) * g.inv_cell, -BIG), BIG)), g.ny - 1);
  b.z0 = max((int)floorf(fminf(fmaxf((qz - r - g.oz) * g.inv_cell, -BIG), BIG)), 0); b.z1 = min((int)floorf(fminf(fmaxf((qz + r - g.oz) * g.inv_cell, -BIG), BIG)), g.nz - 1);
  return b;
}

// visit(p) for the records p = {x, y, z, bitcast(original index)} of the block's cells.  The cells x0 .. x1 of one (z, y) row are one
// contiguous run of g.pts[] (the records are sorted by cell, x fastest).  THE ORDER IS PART OF THE CONTRACT: z ascending, within z y
// ascending, within a row the positions beg + first, beg + first + step, ... below the run's end.  first = 0, step = 1: one lane sees
// every record; first = lane, step = 64: a wave shares the rows.  An empty block (x0 > x1, or y, or z) visits nothing.
template <class Visit>
__device__ __forceinline__ void ball_rows(const GridDev& g, const BallCells& b, uint32_t first, uint32_t step, Visit&& visit) {
  if (b.x0 > b.x1) return;
  for (int z = b.z0; z <= b.z1; ++z)
    for (int y = b.y0; y <= b.y1; ++y) {
      const uint32_t row = ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx;
      const uint32_t beg = g.cell_start[row + b.x0], end = g.cell_start[row + b.x1 + 1];
      for (uint32_t k = beg + first; k < end; k += step) visit(g.pts[k]);
    }
}

// Points with a non-finite coordinate become (NaN, NaN, NaN): such a record sits in the grid's first (empty) cell, is inside nobody's
// ball (its d2 is NaN) and searches nothing itself; an infinite coordinate never reaches the grid's bounding box.  *n_finite (zeroed by
// the caller) += the rows left as they were.  A template so that only the units that launch it carry it.
template <class P> __global__ __launch_bounds__(PRIM_THREADS) void k_points_clean(const P* __restrict__ xyz, size_t n, P* __restrict__ out, unsigned int* n_finite) {
  unsigned int cnt = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    P p = xyz[i];
    if (query_is_finite(p.x, p.y, p.z)) ++cnt;
    else p = P{NAN, NAN, NAN};
    out[i] = p;
  }
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
  if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(n_finite, cnt);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
// *clean = a copy of d_pts[0 .. n) the pool owns, non-finite rows as k_points_clean leaves them; *n_finite = the number of finite rows,
// on the host (one readback, one synchronisation of s).  Whether that is enough points to build a grid is the caller's rule.  P: F3 (a template for the kernel's reason).
template <class P> hipError_t clean_points(DevPool& pool, hipStream_t s, const P* d_pts, size_t n, P** clean, unsigned int* n_finite) {
  unsigned int* d_count = nullptr;
  hipError_t e = pool.get(clean, n);
  if (e == hipSuccess) e = pool.get(&d_count, 1);
  if (e == hipSuccess) e = hipMemsetAsync(d_count, 0, sizeof(unsigned int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_points_clean<P>, dim3(prim_blocks(n)), dim3(PRIM_THREADS), 0, s, d_pts, n, *clean, d_count);
  e = hipMemcpyAsync(n_finite, d_count, sizeof(unsigned int), hipMemcpyDeviceToHost, s);
  return e != hipSuccess ? e : hipStreamSynchronize(s);
}

// `call` is build_grid(...) or its result.  GRID_RANGE_ERROR -> CILHIP_ERR_UNSUPPORTED, "<range_family>: " kGridRangeMessage; any other
// failure -> what ST_CK(family, call) records.
#define GRID_CK(range_family, family, call) do { const hipError_t grid_e_ = (call); \
    if (grid_e_ == cilhip::GRID_RANGE_ERROR) return cilhip::st_fail(CILHIP_ERR_UNSUPPORTED, range_family, cilhip::kGridRangeMessage); \
    if (grid_e_ != hipSuccess) return cilhip::st_fail(CILHIP_ERR_HIP, family, #call, hipGetErrorString(grid_e_)); } while (0)

}  // namespace

}  // namespace cilhip

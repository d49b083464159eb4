// grid_build.hip -- one-off construction of the target index (replaces the single-threaded nanoflann
// kd-tree build: core/kd_tree.hpp:162-170 -> 3rd_party/nanoflann/nanoflann.hpp:1661-1687,1150-1212,
// 5.7 s for 10M points on the reference's CPU path) and the spatial pre-sort of the source cloud.
//
//   bbox + f64 mean (one pass)  ->  cell size from density (adaptive: shrink until the expected
//   own-cell population is small)  ->  cell key per point  ->  stable LSD radix sort of (key, index)
//   (rocPRIM; stable => within a cell points stay in ascending original index)  ->  cell_start table
//   ->  gather into 16-byte {x,y,z,idx} records (+ normals in the same order).
//
// The search radius is NOT baked into the grid (the kd-tree it replaces is radius-agnostic too):
// the query kernel expands shells until its pruning bound proves exactness.
#include <hip/hip_runtime.h>

#include <cstring>

#include <algorithm>
#include <cmath>
#include <vector>

#include "device_prims.hpp"
#include "grid_policy.hpp"
#include "internal.hpp"

namespace cilhip {

#define HIP_TRY(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)

constexpr int RB = 1024;  // reduction blocks

// per-block min/max (f32) over the FINITE coordinates and sum (f64) of all of them: the box is what the grid is laid over (a depth
// sensor's NaN / +-inf points have no cell), the mean stays the IEEE one (NaN or inf for such a cloud, as the reference's dst_mean_)
__global__ __launch_bounds__(256) void k_bbox_sum(const float* __restrict__ xyz, uint32_t n, float* bmin, float* bmax, double* bsum) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  double sm[3] = {0, 0, 0};
  const uint32_t per = (n + gridDim.x - 1) / gridDim.x;
  const uint32_t beg = blockIdx.x * per, end = min(beg + per, n);
  for (uint32_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float v = xyz[3 * (size_t)i + c];
      if (fabsf(v) < INFINITY) { mn[c] = fminf(mn[c], v); mx[c] = fmaxf(mx[c], v); }
      sm[c] += (double)v;
    }
  }
  __shared__ float smn[4][3], smx[4][3];
  __shared__ double ssm[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = mn[c], b = mx[c]; double s = sm[c];
    for (int off = 32; off > 0; off >>= 1) {
      a = fminf(a, __shfl_down(a, off, 64)); b = fmaxf(b, __shfl_down(b, off, 64)); s += __shfl_down(s, off, 64);
    }
    if (lane == 0) { smn[wave][c] = a; smx[wave][c] = b; ssm[wave][c] = s; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int c = threadIdx.x;
    bmin[blockIdx.x * 3 + c] = fminf(fminf(smn[0][c], smn[1][c]), fminf(smn[2][c], smn[3][c]));
    bmax[blockIdx.x * 3 + c] = fmaxf(fmaxf(smx[0][c], smx[1][c]), fmaxf(smx[2][c], smx[3][c]));
    bsum[blockIdx.x * 3 + c] = (ssm[0][c] + ssm[1][c]) + (ssm[2][c] + ssm[3][c]);
  }
}

static hipError_t bbox_mean(const float* d_xyz, uint32_t n, hipStream_t s, float lo[3], float hi[3], double mean[3]) {
  DevBuf<float> d_min, d_max; DevBuf<double> d_sum;
  HIP_TRY(d_min.alloc(RB * 3));
  HIP_TRY(d_max.alloc(RB * 3));
  HIP_TRY(d_sum.alloc(RB * 3));
  hipLaunchKernelGGL(k_bbox_sum, dim3(RB), dim3(256), 0, s, d_xyz, n, d_min.get(), d_max.get(), d_sum.get());
  std::vector<float> hmin(RB * 3), hmax(RB * 3); std::vector<double> hsum(RB * 3);
  HIP_TRY(hipMemcpyAsync(hmin.data(), d_min, RB * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hmax.data(), d_max, RB * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(hsum.data(), d_sum, RB * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  for (int c = 0; c < 3; ++c) { lo[c] = INFINITY; hi[c] = -INFINITY; mean[c] = 0.0; }
  for (int b = 0; b < RB; ++b)
    for (int c = 0; c < 3; ++c) {
      lo[c] = std::min(lo[c], hmin[b * 3 + c]); hi[c] = std::max(hi[c], hmax[b * 3 + c]); mean[c] += hsum[b * 3 + c];
    }
  for (int c = 0; c < 3; ++c) mean[c] = n ? mean[c] / (double)n : 0.0;
  return hipSuccess;
}

hipError_t mean3_device(const float* d_xyz, uint32_t n, hipStream_t s, double mean_out[3], float* lo_out, float* hi_out) {
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  hipError_t e = hipSuccess;
  if (n == 0) mean_out[0] = mean_out[1] = mean_out[2] = 0.0;
  else e = bbox_mean(d_xyz, n, s, lo, hi, mean_out);
  for (int c = 0; c < 3; ++c) { if (lo_out) lo_out[c] = lo[c]; if (hi_out) hi_out[c] = hi[c]; }
  return e;
}

// A point with a non-finite coordinate has no cell: key g.nx * g.ny * g.nz, one past the last cell.  It sorts behind every cell's points
// (its record keeps its index at the tail of GridDev::pts) and no cell range holds it, so no search ever meets it as a candidate.
__device__ __forceinline__ uint32_t cell_of(const GridDev& g, float x, float y, float z) {
  if (!(fabsf(x) < INFINITY && fabsf(y) < INFINITY && fabsf(z) < INFINITY)) return (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz;
  int cx = grid_cell_coord(x, g.ox, g.inv_cell), cy = grid_cell_coord(y, g.oy, g.inv_cell), cz = grid_cell_coord(z, g.oz, g.inv_cell);
  cx = min(max(cx, 0), g.nx - 1); cy = min(max(cy, 0), g.ny - 1); cz = min(max(cz, 0), g.nz - 1);
  return ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
}

__global__ void k_cell_keys(const float* __restrict__ xyz, uint32_t n, GridDev g, uint32_t* keys, uint32_t* vals) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    keys[i] = cell_of(g, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    vals[i] = i;
  }
}

struct Tf { float m[16]; };

__global__ void k_cell_keys_tf(const float* __restrict__ xyz, uint32_t n, GridDev g, Tf T, uint32_t* keys, uint32_t* vals) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float qx, qy, qz;
    transform_point(T.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], qx, qy, qz);
    keys[i] = cell_of(g, qx, qy, qz);
    vals[i] = i;
  }
}

// cell_start[k] = first sorted position whose key >= k, for k in [0, ncells]
__global__ void k_cell_start(const uint32_t* __restrict__ keys_sorted, uint32_t n, uint32_t ncells, uint32_t* cell_start) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += gridDim.x * blockDim.x) {
    const uint32_t prev = (i == 0) ? 0u : keys_sorted[i - 1] + 1u;           // first key not yet closed
    const uint32_t cur = (i == n) ? ncells + 1u : keys_sorted[i] + 1u;      // exclusive end to fill
    for (uint32_t k = prev; k < cur; ++k) cell_start[k] = i;
  }
}

// The same table for MANY cells with long empty stretches (the target grid: two layers of empty cells around the data make
// the first and the last key's gap ~10^5 cells, which one lane of k_cell_start fills alone: 1.4 ms at 10M): mark the first
// sorted position of every non-empty cell, then a reverse running minimum hands every empty cell the start of the next
// non-empty one (0.1 ms).
__global__ void k_run_starts(const uint32_t* __restrict__ keys_sorted, uint32_t n, uint32_t ncells, uint32_t* cell_start) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t k = keys_sorted[i];
    if (i == 0 || keys_sorted[i - 1] != k) cell_start[k] = i;      // (key ncells: the points without a cell -- the table ends where they begin)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && (n == 0 || keys_sorted[n - 1] != ncells)) cell_start[ncells] = n;
}
static inline int grid_blocks(uint32_t n);
// a rocPRIM call (device_prims.hpp) in a temporary block of its own, freed once the stream has run it
template <class Op> static hipError_t run_and_wait(Op op, hipStream_t s) {
  size_t tmp_bytes = 0;
  HIP_TRY(op(nullptr, tmp_bytes));
  DevBuf<unsigned char> tmp;
  HIP_TRY(tmp.alloc(tmp_bytes));
  hipError_t e = op(tmp.get(), tmp_bytes);
  hipError_t e2 = hipStreamSynchronize(s);
  return e != hipSuccess ? e : e2;
}
static hipError_t cell_start_table(const uint32_t* keys_sorted, uint32_t n, uint32_t ncells, uint32_t* cell_start, hipStream_t s) {
  HIP_TRY(hipMemsetAsync(cell_start, 0xFF, ((size_t)ncells + 1) * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_run_starts, dim3(grid_blocks(n)), dim3(256), 0, s, keys_sorted, n, ncells, cell_start);
  auto rit = rocprim::make_reverse_iterator(cell_start + (size_t)ncells + 1);
  return run_and_wait(prim_inclusive_scan(rit, rit, (size_t)ncells + 1, rocprim::minimum<uint32_t>(), s), s);
}

__global__ void k_gather(const float* __restrict__ xyz, const float* __restrict__ nrm, const uint32_t* __restrict__ perm,
                         uint32_t n, float4* pts_out, float4* nrm_out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const uint32_t j = perm[i];
    pts_out[i] = make_float4(xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], __uint_as_float(j));
    if (nrm_out) nrm_out[i] = make_float4(nrm[3 * (size_t)j], nrm[3 * (size_t)j + 1], nrm[3 * (size_t)j + 2], 0.0f);
  }
}

// sum over cells of count^2 (f64): expected own-cell population seen by a random target point is this / n
__global__ void k_occupancy(const uint32_t* __restrict__ cell_start, uint32_t ncells, double* out) {
  double s = 0.0;
  for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < ncells; k += gridDim.x * blockDim.x) {
    const double c = (double)(cell_start[k + 1] - cell_start[k]);
    s += c * c;
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0 && s != 0.0) atomicAdd(out, s);
}

static inline int grid_blocks(uint32_t n) { return (int)std::min<uint32_t>((n + 255) / 256, 8192u) + (n == 0); }

static unsigned bits_for(uint32_t ncells) {
  unsigned b = 1;
  while (b < 32 && (1ull << b) < (unsigned long long)ncells) ++b;
  return b;
}

// grid_policy.hpp decides the shape; false: the cloud's coordinates leave the range an f32 grid can index (GRID_POLICY_RANGE)
static bool set_dims(GridDev& g, const float lo[3], const float hi[3], double cell) {
  GridShape sh{};
  if (grid_set_dims(sh, lo, hi, cell) != GRID_POLICY_OK) return false;
  g.nx = sh.nx; g.ny = sh.ny; g.nz = sh.nz;
  g.cell = sh.cell; g.inv_cell = sh.inv_cell; g.margin = sh.margin;
  g.ox = sh.ox; g.oy = sh.oy; g.oz = sh.oz;
  return true;
}

hipError_t build_grid(const float* d_xyz, const float* d_nrm, uint32_t n, hipStream_t s, GridBuildResult* out, double mean_out[3],
                      double target_occupancy, double refined_factor, double min_cell) {
  GridDev g{};
  g.n = n; g.pts = nullptr; g.nrm = nullptr; g.pn = nullptr; g.cell_start = nullptr;
  GridStore st;      // (handed to *out on success only)
  out->avg_occupancy = 0.0;
  if (n == 0) {
    // empty target: a minimal grid of empty cells; every search returns "none" (kd_tree_utilities.hpp:16-19)
    const float z3[3] = {0, 0, 0};
    (void)set_dims(g, z3, z3, 1.0);
    const size_t nc = (size_t)g.nx * g.ny * g.nz;
    HIP_TRY(st.cell_start.alloc(nc + 1));
    HIP_TRY(hipMemsetAsync(st.cell_start, 0, (nc + 1) * sizeof(uint32_t), s));
    HIP_TRY(st.pts.alloc(1));
    g.cell_start = st.cell_start; g.pts = st.pts;
    out->grid = g; out->store = std::move(st); out->n_cells = nc;
    mean_out[0] = mean_out[1] = mean_out[2] = 0.0;
    return hipSuccess;
  }
  float lo[3], hi[3];
  {
    float lo_raw[3], hi_raw[3];
    HIP_TRY(bbox_mean(d_xyz, n, s, lo_raw, hi_raw, mean_out));
    grid_clean_box(lo_raw, hi_raw, lo, hi);      // an axis without a finite coordinate: extent 0 at origin 0
  }
  const double TARGET = target_occupancy > 0.0 ? target_occupancy : 1.0;  // points per cell for a volumetric cloud
  double cell = grid_first_cell(lo, hi, n, TARGET);
  const bool floor_cell = min_cell > 0.0 && std::isfinite(min_cell);
  if (floor_cell && !(cell >= min_cell)) cell = min_cell;
  if (!set_dims(g, lo, hi, cell)) return GRID_RANGE_ERROR;      // (before anything is allocated)

  DevBuf<uint32_t> k_in, k_out, v_in, v_out;
  DevBuf<double> d_occ;
  HIP_TRY(k_in.alloc(n)); HIP_TRY(k_out.alloc(n));
  HIP_TRY(v_in.alloc(n)); HIP_TRY(v_out.alloc(n));
  HIP_TRY(d_occ.alloc(1));
  double occ = 0.0;
  size_t ncells = 0;
  for (int attempt = 0; attempt < 8; ++attempt) {
    (void)set_dims(g, lo, hi, cell);      // (cannot fail where the first guess did not: the range test does not depend on a smaller cell)
    ncells = (size_t)g.nx * g.ny * g.nz;
    HIP_TRY(st.cell_start.alloc(ncells + 1));
    uint32_t* const cs = st.cell_start;
    hipLaunchKernelGGL(k_cell_keys, dim3(grid_blocks(n)), dim3(256), 0, s, d_xyz, n, g, k_in.get(), v_in.get());
    HIP_TRY(run_and_wait(prim_sort_pairs(k_in.get(), k_out.get(), v_in.get(), v_out.get(), (size_t)n, 0u, bits_for((uint32_t)ncells + 1u), s), s));      // (+ 1: the key of the points without a cell)
    HIP_TRY(cell_start_table(k_out, n, (uint32_t)ncells, cs, s));
    HIP_TRY(hipMemsetAsync(d_occ, 0, sizeof(double), s));
    hipLaunchKernelGGL(k_occupancy, dim3(grid_blocks((uint32_t)ncells)), dim3(256), 0, s, cs, (uint32_t)ncells, d_occ.get());
    HIP_TRY(hipMemcpyAsync(&occ, d_occ, sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    occ /= (double)n;
    // adaptive refinement for surface-like / clustered clouds: too many candidates per cell -> shrink.  Such a cloud fills a small
    // part of its cells; a search that has to go beyond the first block of cells (a source far from alignment, residuals of several
    // cells: two frames of a depth sensor) walks shells of mostly EMPTY cells, and what that costs goes with the number of cells, not
    // of points: refined grids stop at a population RF times that of a volumetric cloud's grid (measured on the reference's frames:
    // frame_1 vs frame_2 0.67 -> 0.27 ms per iteration at 3x the cell edge's third power, the near-aligned pair 0.032 -> 0.038).
    const double RF = refined_factor >= 1.0 ? refined_factor : 1.0;
    if (occ <= 3.0 * TARGET * (attempt == 0 ? 1.0 : RF)) break;
    const double shrink = std::min(0.85, std::max(0.3, std::pow(2.0 * TARGET * RF / occ, 1.0 / 2.5)));
    double new_cell = (double)g.cell * shrink;
    if (floor_cell && new_cell < min_cell) new_cell = min_cell;
    GridDev probe = g;
    if (!set_dims(probe, lo, hi, new_cell)) break;
    if (probe.cell >= g.cell * 0.97f) break;  // dims / cell-count caps reached: keep the current grid
    cell = new_cell;
  }
  HIP_TRY(st.pts.alloc(n));
  if (d_nrm) HIP_TRY(st.nrm.alloc(n));
  hipLaunchKernelGGL(k_gather, dim3(grid_blocks(n)), dim3(256), 0, s, d_xyz, d_nrm, (const uint32_t*)v_out.get(), n, st.pts.get(), st.nrm.get());
  HIP_TRY(hipStreamSynchronize(s));
  g.pts = st.pts; g.nrm = st.nrm; g.cell_start = st.cell_start;
  out->grid = g; out->store = std::move(st); out->avg_occupancy = occ; out->n_cells = ncells;
  return hipSuccess;
}

// ---- source ordering + tiles ------------------------------------------------------------------------
// The source is sorted CUBE-major: cube = CUBE_EDGE^3 block of target-grid cells, key = cube_id * CUBE_EDGE^3 +
// cell within the cube.  Queries of one cube become one (or, above TILE_QUERIES queries, several) TILE(s) of
// the LDS-tiled search kernel: the octant blocks of a cube's queries fit a (CUBE_EDGE+2..3)^3-cell region that
// one workgroup stages in LDS once.
__device__ __forceinline__ uint32_t cube_key_of(const GridDev& g, float x, float y, float z) {
  int cx = grid_cell_coord(x, g.ox, g.inv_cell), cy = grid_cell_coord(y, g.oy, g.inv_cell), cz = grid_cell_coord(z, g.oz, g.inv_cell);
  // cubes tile the DATA cells GRID_PAD..n-1-GRID_PAD (the outer layers hold no target points): shift by the padding,
  // so a cloud registered onto itself fills whole cubes; queries in the low outer layers join cube 0
  cx = min(max(cx - GRID_PAD, 0), g.nx - 1 - GRID_PAD); cy = min(max(cy - GRID_PAD, 0), g.ny - 1 - GRID_PAD); cz = min(max(cz - GRID_PAD, 0), g.nz - 1 - GRID_PAD);
  constexpr uint32_t C = CUBE_EDGE;
  const uint32_t cnx = (uint32_t)(g.nx - 1 - GRID_PAD) / C + 1, cny = (uint32_t)(g.ny - 1 - GRID_PAD) / C + 1;
  const uint32_t bx = (uint32_t)cx / C, by = (uint32_t)cy / C, bz = (uint32_t)cz / C;
  const uint32_t cube = (bz * cny + by) * cnx + bx;
  const uint32_t local = (((uint32_t)cz - bz * C) * C + ((uint32_t)cy - by * C)) * C + ((uint32_t)cx - bx * C);
  return cube * (C * C * C) + local;
}

__global__ void k_cube_keys_tf(const float* __restrict__ xyz, uint32_t n, GridDev g, Tf T, uint32_t* keys, uint32_t* vals) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float qx, qy, qz;
    transform_point(T.m, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], qx, qy, qz);
    keys[i] = cube_key_of(g, qx, qy, qz);
    vals[i] = i;
  }
}

__global__ void k_shift_keys(const uint32_t* __restrict__ in, uint32_t n, uint32_t* out) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = in[i] / (uint32_t)(CUBE_EDGE * CUBE_EDGE * CUBE_EDGE);
}

// tiles of one cube: ceil(count / TILE_QUERIES)
__global__ void k_tile_counts(const uint32_t* __restrict__ cube_start, uint32_t ncubes, uint32_t* counts) {
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < ncubes; c += gridDim.x * blockDim.x)
    counts[c] = (cube_start[c + 1] - cube_start[c] + (TILE_QUERIES - 1)) / TILE_QUERIES;
}

// tile_center[t] = centre of the tile's cube mapped back to SOURCE space (Tinv = inverse of the sort transform):
// with the common half-axes (tile_axes) that is the oriented box k_search_tiled pushes through the current transform
__global__ void k_emit_tiles(const uint32_t* __restrict__ cube_start, const uint32_t* __restrict__ tile_off, uint32_t ncubes, GridDev g, Tf Tinv,
                             uint2* tiles, float4* tile_center) {
  constexpr uint32_t C = CUBE_EDGE;
  const uint32_t cnx = (uint32_t)(g.nx - 1 - GRID_PAD) / C + 1, cny = (uint32_t)(g.ny - 1 - GRID_PAD) / C + 1;
  for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < ncubes; c += gridDim.x * blockDim.x) {
    const uint32_t b = cube_start[c], e = cube_start[c + 1];
    if (b == e) continue;
    const uint32_t bx = c % cnx, by = (c / cnx) % cny, bz = c / (cnx * cny);
    // cube b spans the cells [GRID_PAD + b C, GRID_PAD + (b + 1) C)
    const float hx = g.ox + ((float)(bx * C) + (float)GRID_PAD + 0.5f * (float)C) * g.cell, hy = g.oy + ((float)(by * C) + (float)GRID_PAD + 0.5f * (float)C) * g.cell,
                hz = g.oz + ((float)(bz * C) + (float)GRID_PAD + 0.5f * (float)C) * g.cell;
    const float* m = Tinv.m;
    const float4 ctr = make_float4(m[0] * hx + m[4] * hy + m[8] * hz + m[12], m[1] * hx + m[5] * hy + m[9] * hz + m[13],
                                   m[2] * hx + m[6] * hy + m[10] * hz + m[14], 0.0f);
    uint32_t t = tile_off[c];
    for (uint32_t q = b; q < e; q += TILE_QUERIES) { tiles[t] = make_uint2(q, min(q + TILE_QUERIES, e)); tile_center[t] = ctr; ++t; }
  }
}

// ws (optional): scratch and tile-table storage kept between calls -- a registration loop re-sorts the same source for every new
// initial transform, and the dozen hipMalloc / hipFree of a stand-alone call cost more than its kernels (1.7 -> 0.8 ms at 10M).
// The tile table lives in ws (valid until the next call with it); everything stays on the stream.
hipError_t sort_source(const float* d_xyz, uint32_t n, const GridDev& g, const float T[16], float4* d_out, hipStream_t s,
                       uint2** d_tiles_out, float4** d_tile_center_out, float tile_axes_out[9], uint32_t* ntiles_out, SortWorkspace& ws) {
  *d_tiles_out = nullptr; *d_tile_center_out = nullptr; *ntiles_out = 0;
  // inverse of the (affine) sort transform, in double; a singular linear part leaves a zero box (every query
  // then takes the clean-up pass: slow, still exact)
  Tf tinv;
  {
    const double a00 = T[0], a01 = T[4], a02 = T[8], a10 = T[1], a11 = T[5], a12 = T[9], a20 = T[2], a21 = T[6], a22 = T[10];
    const double det = a00 * (a11 * a22 - a12 * a21) - a01 * (a10 * a22 - a12 * a20) + a02 * (a10 * a21 - a11 * a20);
    const double id = (det != 0.0 && std::isfinite(det)) ? 1.0 / det : 0.0;
    const double i00 = (a11 * a22 - a12 * a21) * id, i01 = (a02 * a21 - a01 * a22) * id, i02 = (a01 * a12 - a02 * a11) * id;
    const double i10 = (a12 * a20 - a10 * a22) * id, i11 = (a00 * a22 - a02 * a20) * id, i12 = (a02 * a10 - a00 * a12) * id;
    const double i20 = (a10 * a21 - a11 * a20) * id, i21 = (a01 * a20 - a00 * a21) * id, i22 = (a00 * a11 - a01 * a10) * id;
    const double t0 = T[12], t1 = T[13], t2 = T[14];
    const double inv[16] = {i00, i10, i20, 0, i01, i11, i21, 0, i02, i12, i22, 0,
                            -(i00 * t0 + i01 * t1 + i02 * t2), -(i10 * t0 + i11 * t1 + i12 * t2), -(i20 * t0 + i21 * t1 + i22 * t2), 1};
    for (int i = 0; i < 16; ++i) tinv.m[i] = (float)inv[i];
    const double h = 0.5 * (double)CUBE_EDGE * (double)g.cell;
    const double li[9] = {i00, i01, i02, i10, i11, i12, i20, i21, i22};
    for (int i = 0; i < 9; ++i) tile_axes_out[i] = (float)(h * li[i]);
  }
  if (n == 0) return hipSuccess;
  constexpr uint32_t CE = CUBE_EDGE;
  const uint32_t cnx = (uint32_t)(g.nx - 1 - GRID_PAD) / CE + 1, cny = (uint32_t)(g.ny - 1 - GRID_PAD) / CE + 1, cnz = (uint32_t)(g.nz - 1 - GRID_PAD) / CE + 1;
  const uint32_t ncubes = cnx * cny * cnz;
  const unsigned bits = std::min(32u, bits_for(ncubes * CE * CE * CE));
  // one slab of scratch: 4 key / value arrays, 3 per-cube arrays, the temporaries of the sort and of the scan
  uint32_t* nul = nullptr;
  size_t sort_tmp = 0, scan_tmp = 0;
  HIP_TRY(prim_sort_pairs(nul, nul, nul, nul, (size_t)n, 0u, bits, s)(nullptr, sort_tmp));
  HIP_TRY(prim_exclusive_sum(nul, nul, (size_t)ncubes + 1, s)(nullptr, scan_tmp));
  auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t arr = up((size_t)n * 4), carr = up(((size_t)ncubes + 1) * 4);
  const size_t need = 4 * arr + 3 * carr + up(sort_tmp ? sort_tmp : 16) + up(scan_tmp ? scan_tmp : 16);
  hipError_t e = hipSuccess;
  if ((e = ws.scratch.ensure(need)) != hipSuccess) return e;
  char* base = reinterpret_cast<char*>(ws.scratch.get());
  uint32_t *k_in = reinterpret_cast<uint32_t*>(base), *k_out = reinterpret_cast<uint32_t*>(base + arr), *v_in = reinterpret_cast<uint32_t*>(base + 2 * arr),
           *v_out = reinterpret_cast<uint32_t*>(base + 3 * arr);
  uint32_t *cube_start = reinterpret_cast<uint32_t*>(base + 4 * arr), *tcount = reinterpret_cast<uint32_t*>(base + 4 * arr + carr),
           *toff = reinterpret_cast<uint32_t*>(base + 4 * arr + 2 * carr);
  void* tmp_sort = base + 4 * arr + 3 * carr;
  void* tmp_scan = base + 4 * arr + 3 * carr + up(sort_tmp ? sort_tmp : 16);
  Tf tf;
  for (int i = 0; i < 16; ++i) tf.m[i] = T[i];
  do {
    hipLaunchKernelGGL(k_cube_keys_tf, dim3(grid_blocks(n)), dim3(256), 0, s, d_xyz, n, g, tf, k_in, v_in);
    if ((e = prim_sort_pairs(k_in, k_out, v_in, v_out, (size_t)n, 0u, bits, s)(tmp_sort, sort_tmp)) != hipSuccess) break;
    hipLaunchKernelGGL(k_gather, dim3(grid_blocks(n)), dim3(256), 0, s, d_xyz, (const float*)nullptr, v_out, n, d_out, (float4*)nullptr);
    // cube_start[] over the sorted cube ids, then the tile table
    hipLaunchKernelGGL(k_shift_keys, dim3(grid_blocks(n)), dim3(256), 0, s, k_out, n, k_in);
    hipLaunchKernelGGL(k_cell_start, dim3(grid_blocks(n + 1)), dim3(256), 0, s, k_in, n, ncubes, cube_start);
    if ((e = hipMemsetAsync(tcount, 0, ((size_t)ncubes + 1) * 4, s)) != hipSuccess) break;
    hipLaunchKernelGGL(k_tile_counts, dim3(grid_blocks(ncubes)), dim3(256), 0, s, cube_start, ncubes, tcount);
    if ((e = prim_exclusive_sum(tcount, toff, (size_t)ncubes + 1, s)(tmp_scan, scan_tmp)) != hipSuccess) break;
    uint32_t ntiles = 0;
    if ((e = hipMemcpyAsync(&ntiles, toff + ncubes, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if (ws.tiles.capacity() < (size_t)ntiles + 1 || ws.centers.capacity() < (size_t)ntiles + 1) {
      ws.tiles.reset(); ws.centers.reset();
      const size_t cap = (size_t)ntiles + 1 + ntiles / 8;
      if ((e = ws.tiles.alloc(cap)) != hipSuccess) break;
      if ((e = ws.centers.alloc(cap)) != hipSuccess) break;
    }
    hipLaunchKernelGGL(k_emit_tiles, dim3(grid_blocks(ncubes)), dim3(256), 0, s, cube_start, toff, ncubes, g, tinv, ws.tiles.get(), ws.centers.get());
    e = hipGetLastError();
    *d_tiles_out = ws.tiles; *d_tile_center_out = ws.centers; *ntiles_out = ntiles;
  } while (0);
  if (e != hipSuccess) { *d_tiles_out = nullptr; *d_tile_center_out = nullptr; *ntiles_out = 0; }
  return e;
}

}  // namespace cilhip

// grid_downsample.hip -- voxel-grid downsampling on the device: cilantro's PointsGridDownsampler3f and its three siblings with
// normals / colours (core/grid_downsampler.hpp over core/grid_accumulator.hpp and core/common_accumulators.hpp), the first line of the
// reference's registration / normal-estimation / clustering examples (`cloud.gridDownsample(0.005f)`).
//
// The contract (DESIGN.md has it in full; every rule cites the reference lines it restates):
//   cell     = floor(fl(p * fl(1 / bin_size))) per axis                                        grid_accumulator.hpp:79, :114-123
//   sums     = the bin's members in ascending input index, one f32 add at a time, the running sum starting AS the first
//              member (common_accumulators.hpp:45-46, :68-72): the reference with parallel = false, or on one thread
//   normals  = if (dot(sum, n_i) < 0) sum -= n_i; else sum += n_i;   dot = x x' + (y y' + z z')            :122-131
//   outputs  = scale * sum with scale = 1.0f / (float)count; normals normalized() afterwards   grid_downsampler.hpp:118-126
//   order    = lexicographic in (cell_x, cell_y, cell_z) (parallel = true, :180-184) or first appearance (:186-197)
// Points with a non-finite coordinate belong to no bin; a finite point whose cell lies outside +-2^20 refuses the call.
//
// The chain:
//   k_gd_range       cells of every point: per-axis minimum / maximum, number of finite points, the error word (atomics, one set per block)
//   k_gd_keys        key = the three cell indices relative to the minimum, packed x | y | z in as few bits as the ranges need
//                    (32-bit keys when they fit); non-finite points get the one key above all others
//   rocPRIM          stable LSD radix sort of (key, index) over exactly those bits: members of a bin stay in index order
//   k_gd_heads + inclusive scan + k_gd_starts      bin of every sorted position, first position of every bin
//   k_gd_keep / k_gd_mark + exclusive scan         output slot of every bin that has min_points_in_bin members, in either order
//   k_gd_gather      points / normals / colours into sorted order (coalesced writes)
//   k_gd_fold_lane   one lane per bin of up to GD_WAVE_MIN members: the serial chain, members read from consecutive addresses
//   k_gd_fold_wave   one wave per longer bin: 64 consecutive members loaded one per lane, the next 64 already in flight, the
//                    chain fed from lane broadcasts (v_readlane) -- it waits on add latency, not on memory
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "internal.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

constexpr int GD_CELL_LIMIT = 1 << 20;       // accepted cells: [-2^20, 2^20) per axis
constexpr uint32_t GD_WAVE_MIN = 64;         // bins with MORE members than this are folded by a whole wave

struct GdRange {
  int mn[3], mx[3];
  unsigned int err;
  unsigned int pad;
  unsigned long long n_valid;
};

struct GdPack {                              // how k_gd_keys packs the three cells
  int mn[3];
  unsigned int shift_x, shift_y;             // bits of (y, z) and of z
  unsigned int skip_bit;                     // the key of a point without a bin: 1 << skip_bit
  float inv;
};

// 0: a cell, 1: no bin (non-finite coordinate), 2: a finite point outside the accepted cells
__device__ __forceinline__ int gd_cell(float inv, float x, float y, float z, int c[3]) {
  if (!(isfinite(x) && isfinite(y) && isfinite(z))) return 1;
  const float fx = floorf(__fmul_rn(x, inv)), fy = floorf(__fmul_rn(y, inv)), fz = floorf(__fmul_rn(z, inv));
  const float lo = -(float)GD_CELL_LIMIT, hi = (float)GD_CELL_LIMIT;
  if (!(fx >= lo && fx < hi && fy >= lo && fy < hi && fz >= lo && fz < hi)) return 2;      // (a product that overflowed ends here too)
  c[0] = (int)fx; c[1] = (int)fy; c[2] = (int)fz;
  return 0;
}

__global__ __launch_bounds__(256) void k_gd_range(const F3* __restrict__ xyz, size_t n, float inv, GdRange* out) {
  int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
  unsigned int err = 0, cnt = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const F3 p = xyz[i];
    int c[3];
    const int st = gd_cell(inv, p.x, p.y, p.z, c);
    if (st == 2) err = 1u;
    if (st == 0) {
      ++cnt;
#pragma unroll
      for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], c[a]); mx[a] = max(mx[a], c[a]); }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], __shfl_down(mn[a], off, 64)); mx[a] = max(mx[a], __shfl_down(mx[a], off, 64)); }
    err |= __shfl_down(err, off, 64);
    cnt += __shfl_down(cnt, off, 64);
  }
  // one set of atomics per block (a few thousand per call: all of them land on the same eight words)
  __shared__ int s_mn[4][3], s_mx[4][3];
  __shared__ unsigned int s_err[4], s_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) { s_mn[wave][a] = mn[a]; s_mx[wave][a] = mx[a]; }
    s_err[wave] = err; s_cnt[wave] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { mn[a] = min(mn[a], s_mn[w][a]); mx[a] = max(mx[a], s_mx[w][a]); }
      err |= s_err[w]; cnt += s_cnt[w];
    }
    if (cnt) {
#pragma unroll
      for (int a = 0; a < 3; ++a) { atomicMin(&out->mn[a], mn[a]); atomicMax(&out->mx[a], mx[a]); }
      atomicAdd(&out->n_valid, (unsigned long long)cnt);
    }
    if (err) atomicOr(&out->err, 1u);
  }
}

template <typename KeyT>
__global__ __launch_bounds__(256) void k_gd_keys(const F3* __restrict__ xyz, size_t n, GdPack pk, KeyT* __restrict__ keys, uint32_t* __restrict__ vals) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const F3 p = xyz[i];
    int c[3];
    KeyT k = (KeyT)1 << pk.skip_bit;
    if (gd_cell(pk.inv, p.x, p.y, p.z, c) == 0)
      k = ((KeyT)(uint32_t)(c[0] - pk.mn[0]) << pk.shift_x) | ((KeyT)(uint32_t)(c[1] - pk.mn[1]) << pk.shift_y) | (KeyT)(uint32_t)(c[2] - pk.mn[2]);
    keys[i] = k;
    vals[i] = (uint32_t)i;
  }
}

template <typename KeyT>
__global__ __launch_bounds__(256) void k_gd_heads(const KeyT* __restrict__ keys, size_t m, uint32_t* __restrict__ flags) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    flags[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// bin_of: inclusive scan of the head flags (bin of position i = bin_of[i] - 1); start[b] = first position of bin b, start[nbins] = m
__global__ __launch_bounds__(256) void k_gd_starts(const uint32_t* __restrict__ bin_of, size_t m, uint32_t nbins, uint32_t* __restrict__ start) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t b = bin_of[i];
    if (i == 0 || bin_of[i - 1] != b) start[b - 1] = (uint32_t)i;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) start[nbins] = (uint32_t)m;
}

// lexicographic order: slot[b] = 1 for a bin that is kept (exclusive scan in place -> its output row; slot[nbins] -> the number of rows)
__global__ __launch_bounds__(256) void k_gd_keep(const uint32_t* __restrict__ start, uint32_t nbins, uint32_t min_pts, uint32_t* __restrict__ slot) {
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b <= nbins; b += (size_t)gridDim.x * blockDim.x)
    slot[b] = (b < nbins && start[b + 1] - start[b] >= min_pts) ? 1u : 0u;
}
// first-appearance order: the stable sort left every bin's lowest input index at its head; mark[] (zeroed, n + 1 entries) gets a 1
// there for every kept bin, its exclusive scan numbers the bins by that index
__global__ __launch_bounds__(256) void k_gd_mark(const uint32_t* __restrict__ start, const uint32_t* __restrict__ perm, uint32_t nbins, uint32_t min_pts,
                                                 uint32_t* __restrict__ mark) {
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbins; b += (size_t)gridDim.x * blockDim.x)
    if (start[b + 1] - start[b] >= min_pts) mark[perm[start[b]]] = 1u;
}
__global__ __launch_bounds__(256) void k_gd_slots(const uint32_t* __restrict__ start, const uint32_t* __restrict__ perm, uint32_t nbins,
                                                  const uint32_t* __restrict__ mark_scanned, uint32_t* __restrict__ slot) {
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < nbins; b += (size_t)gridDim.x * blockDim.x) slot[b] = mark_scanned[perm[start[b]]];
}

__global__ __launch_bounds__(256) void k_gd_gather(const F3* __restrict__ xyz, const F3* __restrict__ nrm, const F3* __restrict__ rgb,
                                                   const uint32_t* __restrict__ perm, size_t m, F3* __restrict__ gp, F3* __restrict__ gn, F3* __restrict__ gc) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t j = perm[i];
    gp[i] = xyz[j];
    if (gn) gn[i] = nrm[j];
    if (gc) gc[i] = rgb[j];
  }
}

struct GdFold {
  const uint32_t* start;     // [nbins + 1]
  const uint32_t* slot;      // [nbins]: output row of a kept bin
  const F3 *gp, *gn, *gc;    // members in sorted order (gn / gc null: no such attribute)
  uint32_t nbins, min_pts;
  uint32_t* long_list;       // bins left to k_gd_fold_wave, and how many
  uint32_t* n_long;
  F3 *out_p, *out_n, *out_c; // (null: not wanted)
  uint32_t* out_cnt;
};

// the pinned 3-term dot product: x x' + (y y' + z z'), every operation rounded to f32
__device__ __forceinline__ float gd_dot(float ax, float ay, float az, float bx, float by, float bz) {
  return __fadd_rn(__fmul_rn(ax, bx), __fadd_rn(__fmul_rn(ay, by), __fmul_rn(az, bz)));
}
// common_accumulators.hpp:124-128
__device__ __forceinline__ void gd_add_normal(float& sx, float& sy, float& sz, float x, float y, float z) {
  if (gd_dot(sx, sy, sz, x, y, z) < 0.0f) { sx = __fsub_rn(sx, x); sy = __fsub_rn(sy, y); sz = __fsub_rn(sz, z); }
  else { sx = __fadd_rn(sx, x); sy = __fadd_rn(sy, y); sz = __fadd_rn(sz, z); }
}
// grid_downsampler.hpp:118-126.  1 / count, the square root and the quotients are the correctly rounded f32 ones, formed in f64.
__device__ __forceinline__ void gd_write(const GdFold& a, uint32_t row, uint32_t cnt, const float* sp, const float* sn, const float* sc) {
  const float scale = (float)(1.0 / (double)(float)cnt);
  if (a.out_p) a.out_p[row] = F3{__fmul_rn(scale, sp[0]), __fmul_rn(scale, sp[1]), __fmul_rn(scale, sp[2])};
  if (a.out_c) a.out_c[row] = F3{__fmul_rn(scale, sc[0]), __fmul_rn(scale, sc[1]), __fmul_rn(scale, sc[2])};
  if (a.out_n) {
    float vx = __fmul_rn(scale, sn[0]), vy = __fmul_rn(scale, sn[1]), vz = __fmul_rn(scale, sn[2]);
    const float z = gd_dot(vx, vy, vz, vx, vy, vz);
    if (z > 0.0f) {
      const double r = (double)(float)sqrt((double)z);
      vx = (float)((double)vx / r); vy = (float)((double)vy / r); vz = (float)((double)vz / r);
    }
    a.out_n[row] = F3{vx, vy, vz};
  }
  if (a.out_cnt) a.out_cnt[row] = cnt;
}

template <bool HAS_N, bool HAS_C>
__global__ __launch_bounds__(256) void k_gd_fold_lane(GdFold a) {
  for (size_t b = (size_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.nbins; b += (size_t)gridDim.x * blockDim.x) {
    const uint32_t beg = a.start[b], cnt = a.start[b + 1] - beg;
    if (cnt < a.min_pts) continue;
    if (cnt > GD_WAVE_MIN) { a.long_list[atomicAdd(a.n_long, 1u)] = (uint32_t)b; continue; }
    float sp[3], sn[3] = {0.f, 0.f, 0.f}, sc[3] = {0.f, 0.f, 0.f};
    { const F3 p = a.gp[beg]; sp[0] = p.x; sp[1] = p.y; sp[2] = p.z; }
    if (HAS_N) { const F3 v = a.gn[beg]; sn[0] = v.x; sn[1] = v.y; sn[2] = v.z; }
    if (HAS_C) { const F3 v = a.gc[beg]; sc[0] = v.x; sc[1] = v.y; sc[2] = v.z; }
    for (uint32_t j = 1; j < cnt; ++j) {
      const F3 p = a.gp[beg + j];
      sp[0] = __fadd_rn(sp[0], p.x); sp[1] = __fadd_rn(sp[1], p.y); sp[2] = __fadd_rn(sp[2], p.z);
      if (HAS_N) { const F3 v = a.gn[beg + j]; gd_add_normal(sn[0], sn[1], sn[2], v.x, v.y, v.z); }
      if (HAS_C) { const F3 v = a.gc[beg + j]; sc[0] = __fadd_rn(sc[0], v.x); sc[1] = __fadd_rn(sc[1], v.y); sc[2] = __fadd_rn(sc[2], v.z); }
    }
    gd_write(a, a.slot[b], cnt, sp, sn, sc);
  }
}

__device__ __forceinline__ float gd_lane(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// One wave per long bin.  Every lane holds one of 64 consecutive members; the chain runs on broadcasts of lane 0, 1, 2, ... (every
// lane computes the same sums: the sign test of the normal rule is wave-uniform), while the next 64 members are already being loaded.
template <bool HAS_N, bool HAS_C>
__global__ __launch_bounds__(256) void k_gd_fold_wave(GdFold a) {
  const uint32_t lane = threadIdx.x & 63u;
  // (wave-uniform, and said so: the bin, its bounds and the loop conditions below then live in scalar registers)
  const uint32_t wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (gridDim.x * blockDim.x) >> 6;
  const uint32_t n_long = *a.n_long;
  const F3 zero{0.f, 0.f, 0.f};
  for (uint32_t w = wave; w < n_long; w += nwaves) {
    const uint32_t b = a.long_list[w];
    const uint32_t beg = a.start[b], cnt = a.start[b + 1] - beg;
    float sp[3] = {0.f, 0.f, 0.f}, sn[3] = {0.f, 0.f, 0.f}, sc[3] = {0.f, 0.f, 0.f};
    F3 cp = lane < cnt ? a.gp[beg + lane] : zero, cn = zero, cc = zero;
    if (HAS_N) cn = lane < cnt ? a.gn[beg + lane] : zero;
    if (HAS_C) cc = lane < cnt ? a.gc[beg + lane] : zero;
    for (uint32_t base = 0; base < cnt; base += 64u) {
      const uint32_t m = min(64u, cnt - base);
      const size_t nx = (size_t)beg + base + 64u + lane;
      const bool more = base + 64u + lane < cnt;
      F3 np = more ? a.gp[nx] : zero, nn = zero, nc = zero;
      if (HAS_N) nn = more ? a.gn[nx] : zero;
      if (HAS_C) nc = more ? a.gc[nx] : zero;
      if (base == 0) {      // the sums start AS the first member
        sp[0] = gd_lane(cp.x, 0); sp[1] = gd_lane(cp.y, 0); sp[2] = gd_lane(cp.z, 0);
        if (HAS_N) { sn[0] = gd_lane(cn.x, 0); sn[1] = gd_lane(cn.y, 0); sn[2] = gd_lane(cn.z, 0); }
        if (HAS_C) { sc[0] = gd_lane(cc.x, 0); sc[1] = gd_lane(cc.y, 0); sc[2] = gd_lane(cc.z, 0); }
      }
      auto add_member = [&](int l) {
        sp[0] = __fadd_rn(sp[0], gd_lane(cp.x, l)); sp[1] = __fadd_rn(sp[1], gd_lane(cp.y, l)); sp[2] = __fadd_rn(sp[2], gd_lane(cp.z, l));
        if (HAS_N) gd_add_normal(sn[0], sn[1], sn[2], gd_lane(cn.x, l), gd_lane(cn.y, l), gd_lane(cn.z, l));
        if (HAS_C) { sc[0] = __fadd_rn(sc[0], gd_lane(cc.x, l)); sc[1] = __fadd_rn(sc[1], gd_lane(cc.y, l)); sc[2] = __fadd_rn(sc[2], gd_lane(cc.z, l)); }
      };
      if (base != 0 && m == 64u) {      // a whole chunk: 64 broadcasts and adds in a straight line
#pragma unroll
        for (int l = 0; l < 64; ++l) add_member(l);
      } else {                          // the first chunk (member 0 is the seed) and the last one: a loop over a scalar lane index
#pragma unroll 1
        for (uint32_t l = base == 0 ? 1u : 0u; l < m; ++l) add_member((int)l);
      }
      cp = np; cn = nn; cc = nc;
    }
    if (lane == 0) gd_write(a, a.slot[b], cnt, sp, sn, sc);
  }
}

inline int gd_blocks(size_t n) { return (int)std::min<size_t>((n + 255) / 256, 8192) + (n == 0); }
unsigned gd_bits(int range) {      // bits that hold 0 .. range
  unsigned b = 0;
  while (((long long)1 << b) <= (long long)range) ++b;
  return b;
}

struct GdCall {
  const float *xyz, *nrm, *rgb;
  size_t n;
  int mem;
  float bin_size;
  size_t min_pts;
  int bin_order;
  float *xyz_out, *nrm_out, *rgb_out;
  uint32_t* cnt_out;
  size_t capacity;
  size_t* n_out;
};

template <typename KeyT>
int gd_sort_and_fold(const GdCall& c, DevPool& pool, hipStream_t s, const F3* d_xyz, const F3* d_nrm, const F3* d_rgb, const GdPack& pk, unsigned end_bit, size_t m) {
  const size_t n = c.n;
  KeyT *k_in = nullptr, *k_out = nullptr;
  uint32_t *v_in = nullptr, *v_out = nullptr;
  ST_CK("grid_downsample", pool.bytes(&k_in, n * sizeof(KeyT))); ST_CK("grid_downsample", pool.bytes(&k_out, n * sizeof(KeyT)));
  ST_CK("grid_downsample", pool.bytes(&v_in, (n + 1) * sizeof(uint32_t))); ST_CK("grid_downsample", pool.bytes(&v_out, n * sizeof(uint32_t)));
  hipLaunchKernelGGL((k_gd_keys<KeyT>), dim3(gd_blocks(n)), dim3(256), 0, s, d_xyz, n, pk, k_in, v_in);
  ST_CK("grid_downsample", prim_run(pool, prim_sort_pairs(k_in, k_out, v_in, v_out, n, 0u, end_bit, s)));
  // the first m sorted positions are the points that have a bin
  uint32_t* bin_of = reinterpret_cast<uint32_t*>(k_in);      // (the unsorted keys are done with)
  hipLaunchKernelGGL((k_gd_heads<KeyT>), dim3(gd_blocks(m)), dim3(256), 0, s, (const KeyT*)k_out, m, bin_of);
  void* scan_tmp = nullptr;      // one block for every scan below: the larger of the two requests
  size_t scan_bytes = 0;
  const auto bin_scan = prim_inclusive_sum(bin_of, bin_of, m, s);
  {
    size_t b1 = 0, b2 = 0;
    ST_CK("grid_downsample", bin_scan(nullptr, b1));
    ST_CK("grid_downsample", prim_exclusive_sum(bin_of, bin_of, n + 1, s)(nullptr, b2));
    scan_bytes = std::max(b1, b2);
    ST_CK("grid_downsample", pool.bytes(&scan_tmp, scan_bytes));
  }
  ST_CK("grid_downsample", bin_scan(scan_tmp, scan_bytes));
  uint32_t nbins = 0;
  ST_CK("grid_downsample", hipMemcpyAsync(&nbins, bin_of + (m - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ST_CK("grid_downsample", hipStreamSynchronize(s));
  uint32_t *start = nullptr, *slot = nullptr;
  ST_CK("grid_downsample", pool.bytes(&start, ((size_t)nbins + 1) * sizeof(uint32_t)));
  ST_CK("grid_downsample", pool.bytes(&slot, ((size_t)nbins + 1) * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_gd_starts, dim3(gd_blocks(m)), dim3(256), 0, s, (const uint32_t*)bin_of, m, nbins, start);
  const uint32_t min_pts = (uint32_t)std::min<size_t>(c.min_pts, 0xFFFFFFFFull);      // (no bin has 2^32 members: anything above refuses them all)
  uint32_t rows = 0;
  if (c.bin_order == 1) {
    hipLaunchKernelGGL(k_gd_keep, dim3(gd_blocks((size_t)nbins + 1)), dim3(256), 0, s, (const uint32_t*)start, nbins, min_pts, slot);
    ST_CK("grid_downsample", prim_exclusive_sum(slot, slot, (size_t)nbins + 1, s)(scan_tmp, scan_bytes));
    ST_CK("grid_downsample", hipMemcpyAsync(&rows, slot + nbins, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  } else {
    uint32_t* mark = v_in;      // (the unsorted indices are done with; n + 1 entries)
    ST_CK("grid_downsample", hipMemsetAsync(mark, 0, (n + 1) * sizeof(uint32_t), s));
    hipLaunchKernelGGL(k_gd_mark, dim3(gd_blocks(nbins)), dim3(256), 0, s, (const uint32_t*)start, (const uint32_t*)v_out, nbins, min_pts, mark);
    ST_CK("grid_downsample", prim_exclusive_sum(mark, mark, n + 1, s)(scan_tmp, scan_bytes));
    hipLaunchKernelGGL(k_gd_slots, dim3(gd_blocks(nbins)), dim3(256), 0, s, (const uint32_t*)start, (const uint32_t*)v_out, nbins, (const uint32_t*)mark, slot);
    ST_CK("grid_downsample", hipMemcpyAsync(&rows, mark + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  ST_CK("grid_downsample", hipStreamSynchronize(s));
  *c.n_out = rows;
  const bool want = c.xyz_out || c.nrm_out || c.rgb_out || c.cnt_out;
  if (!want && c.capacity == 0) return CILHIP_OK;      // the counting call
  if (rows > c.capacity) return st_fail(CILHIP_ERR_INVALID, "grid_downsample", "capacity is smaller than the number of bins (*n_out has it; capacity = n always suffices)");
  if (rows == 0 || !want) return CILHIP_OK;

  const bool has_n = d_nrm && c.nrm_out, has_c = d_rgb && c.rgb_out;
  F3 *gp = nullptr, *gn = nullptr, *gc = nullptr;
  ST_CK("grid_downsample", pool.bytes(&gp, m * sizeof(F3)));
  if (has_n) ST_CK("grid_downsample", pool.bytes(&gn, m * sizeof(F3)));
  if (has_c) ST_CK("grid_downsample", pool.bytes(&gc, m * sizeof(F3)));
  hipLaunchKernelGGL(k_gd_gather, dim3(gd_blocks(m)), dim3(256), 0, s, d_xyz, has_n ? d_nrm : (const F3*)nullptr, has_c ? d_rgb : (const F3*)nullptr,
                     (const uint32_t*)v_out, m, gp, gn, gc);
  GdFold a{};
  a.start = start; a.slot = slot; a.gp = gp; a.gn = gn; a.gc = gc; a.nbins = nbins; a.min_pts = min_pts;
  uint32_t* n_long = nullptr;
  // a bin that goes to the wave form has more than GD_WAVE_MIN members: there are fewer than m / GD_WAVE_MIN of them
  ST_CK("grid_downsample", pool.bytes(&a.long_list, (m / GD_WAVE_MIN + 1) * sizeof(uint32_t)));
  ST_CK("grid_downsample", pool.bytes(&n_long, sizeof(uint32_t)));
  ST_CK("grid_downsample", hipMemsetAsync(n_long, 0, sizeof(uint32_t), s));
  a.n_long = n_long;
  const bool host = c.mem == CILHIP_MEM_HOST;
  if (host) {
    if (c.xyz_out) ST_CK("grid_downsample", pool.bytes(&a.out_p, (size_t)rows * sizeof(F3)));
    if (has_n) ST_CK("grid_downsample", pool.bytes(&a.out_n, (size_t)rows * sizeof(F3)));
    if (has_c) ST_CK("grid_downsample", pool.bytes(&a.out_c, (size_t)rows * sizeof(F3)));
    if (c.cnt_out) ST_CK("grid_downsample", pool.bytes(&a.out_cnt, (size_t)rows * sizeof(uint32_t)));
  } else {
    a.out_p = reinterpret_cast<F3*>(c.xyz_out);
    a.out_n = has_n ? reinterpret_cast<F3*>(c.nrm_out) : nullptr;
    a.out_c = has_c ? reinterpret_cast<F3*>(c.rgb_out) : nullptr;
    a.out_cnt = c.cnt_out;
  }
  const dim3 lane_grid(gd_blocks(nbins)), wave_grid((unsigned)std::min<size_t>(m / GD_WAVE_MIN / 4 + 1, 2048));
  if (has_n && has_c) {
    hipLaunchKernelGGL((k_gd_fold_lane<true, true>), lane_grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_gd_fold_wave<true, true>), wave_grid, dim3(256), 0, s, a);
  } else if (has_n) {
    hipLaunchKernelGGL((k_gd_fold_lane<true, false>), lane_grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_gd_fold_wave<true, false>), wave_grid, dim3(256), 0, s, a);
  } else if (has_c) {
    hipLaunchKernelGGL((k_gd_fold_lane<false, true>), lane_grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_gd_fold_wave<false, true>), wave_grid, dim3(256), 0, s, a);
  } else {
    hipLaunchKernelGGL((k_gd_fold_lane<false, false>), lane_grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_gd_fold_wave<false, false>), wave_grid, dim3(256), 0, s, a);
  }
  ST_CK("grid_downsample", hipGetLastError());
  if (host) {
    if (a.out_p) ST_CK("grid_downsample", hipMemcpyAsync(c.xyz_out, a.out_p, (size_t)rows * sizeof(F3), hipMemcpyDeviceToHost, s));
    if (a.out_n) ST_CK("grid_downsample", hipMemcpyAsync(c.nrm_out, a.out_n, (size_t)rows * sizeof(F3), hipMemcpyDeviceToHost, s));
    if (a.out_c) ST_CK("grid_downsample", hipMemcpyAsync(c.rgb_out, a.out_c, (size_t)rows * sizeof(F3), hipMemcpyDeviceToHost, s));
    if (a.out_cnt) ST_CK("grid_downsample", hipMemcpyAsync(c.cnt_out, a.out_cnt, (size_t)rows * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  }
  ST_CK("grid_downsample", hipStreamSynchronize(s));
  return CILHIP_OK;
}

int gd_run(const GdCall& c, int device) {
  if (const int open = st_open("grid_downsample", device)) return open;
  DevPool pool;
  StreamGuard st;      // (declared after the pool: the stream is drained and destroyed before anything is freed)
  ST_CK("grid_downsample", st.create());
  hipStream_t s = st.s;
  const size_t n = c.n;
  const F3 *d_xyz = nullptr, *d_nrm = nullptr, *d_rgb = nullptr;
  ST_CK("grid_downsample", st_stage(pool, s, c.mem, c.xyz, n, &d_xyz));
  if (c.nrm) ST_CK("grid_downsample", st_stage(pool, s, c.mem, c.nrm, n, &d_nrm));
  if (c.rgb) ST_CK("grid_downsample", st_stage(pool, s, c.mem, c.rgb, n, &d_rgb));
  const float inv = 1.0f / c.bin_size;      // grid_accumulator.hpp:79 (cwiseInverse, f32)
  GdRange h{};
  for (int a = 0; a < 3; ++a) { h.mn[a] = INT_MAX; h.mx[a] = INT_MIN; }
  GdRange* d_range = nullptr;
  ST_CK("grid_downsample", pool.bytes(&d_range, sizeof(GdRange)));
  ST_CK("grid_downsample", hipMemcpyAsync(d_range, &h, sizeof(GdRange), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_gd_range, dim3(std::min(gd_blocks(n), 2048)), dim3(256), 0, s, d_xyz, n, inv, d_range);
  ST_CK("grid_downsample", hipMemcpyAsync(&h, d_range, sizeof(GdRange), hipMemcpyDeviceToHost, s));
  ST_CK("grid_downsample", hipStreamSynchronize(s));
  if (h.err)
    return st_fail(CILHIP_ERR_UNSUPPORTED, "grid_downsample", "a finite point lies in a cell outside [-2^20, 2^20) on some axis (three cell indices must fit one 64-bit sort key): use a larger bin_size or move the cloud towards the origin");
  const size_t m = (size_t)h.n_valid;
  if (m == 0) { *c.n_out = 0; return CILHIP_OK; }      // nothing but non-finite points
  const unsigned bx = gd_bits(h.mx[0] - h.mn[0]), by = gd_bits(h.mx[1] - h.mn[1]), bz = gd_bits(h.mx[2] - h.mn[2]);
  GdPack pk{};
  for (int a = 0; a < 3; ++a) pk.mn[a] = h.mn[a];
  pk.shift_y = bz; pk.shift_x = by + bz; pk.skip_bit = bx + by + bz; pk.inv = inv;
  const unsigned end_bit = std::max(1u, pk.skip_bit + (m < n ? 1u : 0u));      // (<= 64: three ranges of at most 21 bits, and the skip bit)
  if (pk.skip_bit + 1 <= 32) return gd_sort_and_fold<uint32_t>(c, pool, s, d_xyz, d_nrm, d_rgb, pk, end_bit, m);
  return gd_sort_and_fold<unsigned long long>(c, pool, s, d_xyz, d_nrm, d_rgb, pk, end_bit, m);
}

}  // namespace

}  // namespace cilhip

extern "C" int cilhip_grid_downsample3f(int device, const float* xyz, const float* normals_or_null, const float* rgb_or_null, size_t n, int mem, float bin_size,
                                        size_t min_points_in_bin, int bin_order, float* xyz_out, float* normals_out, float* rgb_out, uint32_t* counts_out_or_null,
                                        size_t capacity, size_t* n_out) {
  using namespace cilhip;
  // argument rules first: they hold on a machine without a device too
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, "grid_downsample", why); };
  if (!n_out) return refuse("n_out is null");
  if (!(bin_size > 0.0f) || !std::isfinite(bin_size)) return refuse("bin_size must be a finite positive number");
  if ((unsigned long long)n >= (1ull << 32)) return refuse("n must be below 2^32");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (bin_order != 0 && bin_order != 1) return refuse("bin_order: 0 = first appearance, 1 = lexicographic");
  if (n && !xyz) return refuse("points is null");
  st_clear();
  if (n == 0) { *n_out = 0; return CILHIP_OK; }      // (without touching a device)
  GdCall c{xyz, normals_or_null, rgb_or_null, n, mem, bin_size, min_points_in_bin, bin_order, xyz_out, normals_out, rgb_out, counts_out_or_null, capacity, n_out};
  try {
    return gd_run(c, device);
  } catch (...) {      // (out of host memory: never across the C boundary)
    return st_fail(CILHIP_ERR_HIP, "grid_downsample", "out of host memory");
  }
}

// image_device.hpp -- the device code and host helpers that image_conversions.hip (depth images <-> points) and fusion.hip (the map
// update over two index maps) share: the pinned arithmetic of DESIGN.md section 14.1 and the splat kernel behind rule P4 / P5.
//   ic_dot3        a0 b0 + (a1 b1 + a2 b2), every product and sum rounded to f32
//   ic_apply       the engine's pinned point transform (L_r0 x + (L_r1 y + L_r2 z)) + t_r;  ic_linear: its linear part
//   ic_normalized  DESIGN section 10 rule 4: v / sqrt(|v|^2) if |v|^2 > 0, else v (correctly rounded f32 square root and quotients)
//   ic_pixel       P3: llround of a projected coordinate as a pixel coordinate, or -1
//   k_ic_splat     one lane per point: one 64-bit atomicMin on (bits(c_z) << 32) | index or (raw << 32) | index
//   ic_rigid / ic_to_cam   a column-major 4x4 as rows of L and t / its inverse (R^T, -R^T t) formed in f64 and rounded once (P1)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/cilantro_hip/c_api.h"
#include "internal.hpp"

namespace cilhip {

constexpr unsigned long long IC_LIMIT = 0xFFFFFFF0ull;      // w * h and n stay below 2^32 - 16
constexpr unsigned long long IC_EMPTY = ~0ull;
constexpr int IC_BLOCK = 256;

struct IcConv { float scale, inv_scale, max_depth; int truncated, raw_type; };

__device__ __forceinline__ float ic_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return __fadd_rn(__fmul_rn(a0, b0), __fadd_rn(__fmul_rn(a1, b1), __fmul_rn(a2, b2)));
}
// the engine's pinned point transform: (L_r0 x + (L_r1 y + L_r2 z)) + t_r; M = rows of L, then t
struct IcRigid { float L[9]; float t[3]; };
__device__ __forceinline__ F3 ic_linear(const IcRigid& m, F3 p) {
  return F3{ic_dot3(m.L[0], m.L[1], m.L[2], p.x, p.y, p.z), ic_dot3(m.L[3], m.L[4], m.L[5], p.x, p.y, p.z), ic_dot3(m.L[6], m.L[7], m.L[8], p.x, p.y, p.z)};
}
__device__ __forceinline__ F3 ic_apply(const IcRigid& m, F3 p) {
  const F3 l = ic_linear(m, p);
  return F3{__fadd_rn(l.x, m.t[0]), __fadd_rn(l.y, m.t[1]), __fadd_rn(l.z, m.t[2])};
}
__device__ __forceinline__ F3 ic_normalized(F3 v) {
  const float z = ic_dot3(v.x, v.y, v.z, v.x, v.y, v.z);
  if (z > 0.0f) {      // (the correctly rounded f32 square root and quotients, formed in f64 as everywhere in the engine)
    const double s = (double)(float)sqrt((double)z);
    v.x = (float)((double)v.x / s); v.y = (float)((double)v.y / s); v.z = (float)((double)v.z / s);
  }
  return v;
}

struct IcSplat {
  const F3* xyz;
  uint32_t n;
  int has_cam;
  IcRigid to_cam;
  float k0[3], k1[3];      // rows 0 and 1 of K
  uint32_t w, h;
  IcConv conv;
  unsigned long long* keys;      // [w * h], IC_EMPTY where nothing landed
};

// P3: llround of a finite u as a pixel coordinate below `limit`; -1: outside
__device__ __forceinline__ long long ic_pixel(float u, uint32_t limit) {
  const float r = roundf(u);      // ties away from zero
  if (!(r >= 0.0f && r < 4294967296.0f)) return -1;      // (-0.4 rounds to -0: pixel 0)
  const long long x = (long long)r;
  return x < (long long)limit ? x : -1;
}

enum { IC_INDEX = 0, IC_DEPTH = 1 };

template <int MODE>
__global__ __launch_bounds__(IC_BLOCK) void k_ic_splat(IcSplat a) {
  const size_t i = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  if (i >= a.n) return;
  F3 c = a.xyz[i];
  if (a.has_cam) c = ic_apply(a.to_cam, c);      // P1
  if (!(c.z > 0.0f)) return;                     // P2 (NaN ends here)
  const float inv_z = (float)(1.0 / (double)c.z);
  const float u = __fmul_rn(inv_z, ic_dot3(a.k0[0], a.k0[1], a.k0[2], c.x, c.y, c.z)), v = __fmul_rn(inv_z, ic_dot3(a.k1[0], a.k1[1], a.k1[2], c.x, c.y, c.z));
  if (!(isfinite(u) && isfinite(v))) return;
  const long long x = ic_pixel(u, a.w), y = ic_pixel(v, a.h);
  if (x < 0 || y < 0) return;
  uint32_t hi;
  if (MODE == IC_INDEX) {
    hi = (uint32_t)__float_as_int(c.z);
  } else {       // P5
    if (a.conv.truncated && !(c.z < a.conv.max_depth)) return;
    const float prod = __fmul_rn(a.conv.scale, c.z);
    if (a.conv.raw_type == CILHIP_DEPTH_U16) {
      if (!(prod < 65536.0f)) return;      // (NaN too: no defined conversion)
      hi = (uint32_t)prod;                 // truncation toward zero
      if (hi == 0u) return;
    } else {
      if (!(prod > 0.0f)) return;
      hi = (uint32_t)__float_as_int(prod);
    }
  }
  // y < h, x < w and w * h < 2^32 - 16: the pixel is inside keys[]
  atomicMin(&a.keys[(size_t)y * a.w + (size_t)x], ((unsigned long long)hi << 32) | (unsigned long long)(uint32_t)i);
}

inline unsigned ic_blocks(size_t n) { return (unsigned)((n + IC_BLOCK - 1) / IC_BLOCK); }      // (n < 2^32: below the grid limit)

// ---- host side of the rules ------------------------------------------------------------------------------------------
inline bool ic_all_finite(const float* a, int n) {
  for (int i = 0; i < n; ++i) if (!std::isfinite(a[i])) return false;
  return true;
}
inline IcRigid ic_rigid(const float* E) {      // column-major 4x4 -> rows of the linear part, translation
  IcRigid m{};
  for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) m.L[3 * r + c] = E[r + 4 * c]; m.t[r] = E[r + 12]; }
  return m;
}
// P1: to_cam = (R^T, -R^T t), formed in f64 from the f32 entries, rounded once
inline IcRigid ic_to_cam(const float* E) {
  IcRigid m{};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) m.L[3 * r + c] = E[c + 4 * r];
    m.t[r] = (float)-((double)E[0 + 4 * r] * (double)E[12] + ((double)E[1 + 4 * r] * (double)E[13] + (double)E[2 + 4 * r] * (double)E[14]));
  }
  return m;
}

}  // namespace cilhip

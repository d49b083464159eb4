// projective.hip -- projective association inside a context: cilantro's correspondence_search/correspondence_search_projective.hpp
// (:156-209) over the target's index map.  DESIGN.md section 14.4 has the rules (S1-S3); the projection is rules P1-P3 of the image
// conversions (image_conversions.hip), the same expressions, so a point lands on the pixel cilhip_points_to_index_map3f gives it.
//   k_proj_keys    one lane per SORTED target position: one 64-bit atomicMin on (bits(c_z) << 32) | original index -- ties in c_z go to
//                  the lowest ORIGINAL index (rule P4), whatever the grid's order
//   k_proj_claim   the same lanes again: the one whose key won writes its sorted position -- what the accumulation kernels index
//   k_proj_search  one lane per sorted source point: q = T s, project, one 4-byte gather from the map, one point gather,
//                  value = dx^2 + (dy^2 + dz^2), kept iff value < max_sq (strict)
#include <hip/hip_runtime.h>

#include "internal.hpp"
#include "solve.hpp"

namespace cilhip {

namespace {

__device__ __forceinline__ float pj_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
  return __fadd_rn(__fmul_rn(a0, b0), __fadd_rn(__fmul_rn(a1, b1), __fmul_rn(a2, b2)));
}
__device__ __forceinline__ long long pj_round(float u, uint32_t limit) {      // llround: ties away from zero; -1: outside [0, limit)
  const float r = roundf(u);
  if (!(r >= 0.0f && r < 4294967296.0f)) return -1;
  const long long x = (long long)r;
  return x < (long long)limit ? x : -1;
}
// P1-P3: the pixel of a world point, or -1; *cz = its camera-frame depth
__device__ __forceinline__ long long pj_pixel(const ProjDev& p, float x, float y, float z, float* cz) {
  float cx = x, cy = y, c_z = z;
  if (p.has_cam) {
    cx = __fadd_rn(pj_dot3(p.L[0], p.L[1], p.L[2], x, y, z), p.t[0]);
    cy = __fadd_rn(pj_dot3(p.L[3], p.L[4], p.L[5], x, y, z), p.t[1]);
    c_z = __fadd_rn(pj_dot3(p.L[6], p.L[7], p.L[8], x, y, z), p.t[2]);
  }
  *cz = c_z;
  if (!(c_z > 0.0f)) return -1;
  const float inv_z = (float)(1.0 / (double)c_z);
  const float u = __fmul_rn(inv_z, pj_dot3(p.k0[0], p.k0[1], p.k0[2], cx, cy, c_z)), v = __fmul_rn(inv_z, pj_dot3(p.k1[0], p.k1[1], p.k1[2], cx, cy, c_z));
  if (!(isfinite(u) && isfinite(v))) return -1;
  const long long px = pj_round(u, p.w), py = pj_round(v, p.h);
  if (px < 0 || py < 0) return -1;
  return py * (long long)p.w + px;      // < w * h
}

template <bool CLAIM>
__global__ __launch_bounds__(256) void k_proj_map(const float4* __restrict__ pts, uint32_t n, ProjDev p, unsigned long long* __restrict__ keys, uint32_t* __restrict__ map) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float4 t = pts[j];
  float cz;
  const long long pix = pj_pixel(p, t.x, t.y, t.z, &cz);
  if (pix < 0) return;
  const unsigned long long key = ((unsigned long long)(uint32_t)__float_as_int(cz) << 32) | (unsigned long long)__float_as_uint(t.w);
  if (CLAIM) { if (keys[pix] == key) map[pix] = (uint32_t)j; }
  else atomicMin(&keys[pix], key);
}

__global__ __launch_bounds__(256) void k_proj_search(const float4* __restrict__ src, uint32_t ns, const IcpState* __restrict__ state, const float4* __restrict__ pts, ProjDev p,
                                                     const uint32_t* __restrict__ map, float max_sq, uint32_t* __restrict__ nn_pos, float* __restrict__ nn_d2) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ns) return;
  float T[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) T[k] = state->T[k];
  const float4 s4 = src[i];
  float qx, qy, qz, cz;
  transform_point(T, s4.x, s4.y, s4.z, qx, qy, qz);
  uint32_t pos = NONE_U32;
  float val = 0.0f;
  const long long pix = pj_pixel(p, qx, qy, qz, &cz);
  if (pix >= 0) {
    const uint32_t j = map[pix];
    if (j != NONE_U32) {
      const float4 t = pts[j];
      const float dx = __fsub_rn(qx, t.x), dy = __fsub_rn(qy, t.y), dz = __fsub_rn(qz, t.z);
      const float d = __fadd_rn(__fmul_rn(dx, dx), __fadd_rn(__fmul_rn(dy, dy), __fmul_rn(dz, dz)));
      if (d < max_sq) { pos = j; val = d; }
    }
  }
  nn_pos[i] = pos;
  if (nn_d2) nn_d2[i] = val;
}

}  // namespace

hipError_t launch_proj_map(const float4* pts, uint32_t n, const ProjDev& p, unsigned long long* keys, uint32_t* map, hipStream_t s) {
  const size_t npix = (size_t)p.w * p.h;
  hipError_t e = hipMemsetAsync(keys, 0xFF, npix * sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(map, 0xFF, npix * sizeof(uint32_t), s);
  if (e != hipSuccess || n == 0) return e;
  const unsigned nb = (unsigned)(((size_t)n + 255) / 256);
  hipLaunchKernelGGL((k_proj_map<false>), dim3(nb), dim3(256), 0, s, pts, n, p, keys, map);
  hipLaunchKernelGGL((k_proj_map<true>), dim3(nb), dim3(256), 0, s, pts, n, p, keys, map);
  return hipGetLastError();
}

void launch_proj_search(const float4* src, uint32_t ns, const IcpState* state, const float4* pts, const ProjDev& p, const uint32_t* map, float max_sq, uint32_t* nn_pos,
                        float* nn_d2, hipStream_t s) {
  if (ns == 0) return;
  hipLaunchKernelGGL(k_proj_search, dim3((unsigned)(((size_t)ns + 255) / 256)), dim3(256), 0, s, src, ns, state, pts, p, map, max_sq, nn_pos, nn_d2);
}

}  // namespace cilhip

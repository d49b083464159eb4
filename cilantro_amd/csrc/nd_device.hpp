// nd_device.hpp -- what the kernels over n x dim float points (1 <= dim <= 16) share: rule N1 of DESIGN.md section 21 written once, and
// the switch that instantiates a kernel template for every dimension.  Included by .hip files only; everything has internal linkage.
#pragma once

#include <hip/hip_runtime.h>

namespace cilhip {
namespace {

// A point whose DIM coordinates live in registers, and its squared distance to a point in memory.
template <int DIM> struct NdQuery {
  float c[DIM];
  __device__ __forceinline__ void load(const float* __restrict__ q) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) c[d] = q[d];
  }
  // N1: nanoflann's L2_Adaptor::evalMetric in f32, every operation rounded, nothing contracted: r = 0; per full group of four coordinates
  // r = r + (((s0 + s1) + s2) + s3); then r = r + s for each coordinate left over (s_i = (q_i - p_i)^2).  dim = 3: d2_pinned.
  __device__ __forceinline__ float d2(const float* __restrict__ p) const {
    float r = 0.0f;
#pragma unroll
    for (int g = 0; g + 4 <= DIM; g += 4) {
      const float t0 = __fsub_rn(c[g], p[g]), t1 = __fsub_rn(c[g + 1], p[g + 1]), t2 = __fsub_rn(c[g + 2], p[g + 2]), t3 = __fsub_rn(c[g + 3], p[g + 3]);
      r = __fadd_rn(r, __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(t0, t0), __fmul_rn(t1, t1)), __fmul_rn(t2, t2)), __fmul_rn(t3, t3)));
    }
#pragma unroll
    for (int d = DIM & ~3; d < DIM; ++d) {
      const float t = __fsub_rn(c[d], p[d]);
      r = __fadd_rn(r, __fmul_rn(t, t));
    }
    return r;
  }
};

}  // namespace
}  // namespace cilhip

// CALL(D) for the D that equals dim (1 .. 16; the entries have refused everything else)
#define ND_DISPATCH(dim, CALL)                                                                                                                  \
  switch (dim) {                                                                                                                                \
    case 1: CALL(1); break; case 2: CALL(2); break; case 3: CALL(3); break; case 4: CALL(4); break; case 5: CALL(5); break; case 6: CALL(6); break;      \
    case 7: CALL(7); break; case 8: CALL(8); break; case 9: CALL(9); break; case 10: CALL(10); break; case 11: CALL(11); break; case 12: CALL(12); break; \
    case 13: CALL(13); break; case 14: CALL(14); break; case 15: CALL(15); break; default: CALL(16); break;                                          \
  }

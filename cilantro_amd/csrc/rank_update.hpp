// rank_update.hpp -- the matrix-core accumulation of the rigid classes' normal-equation sums: THE one copy of the LDS layouts, the
// v_mfma_f64_16x16x4_f64 loops and the map from the 16x16 tile to a row of SUMS_MAX sums (FusedZ<ACC>::slot_terms).  Z += z z^T per
// correspondence, two groups of correspondences per tile when the term vector has at most eight components (DUAL).  The parts
// (stage / mfma_round / store_tile / fold_row) are what k_search_tiled (step 5) and k_warm call, each with its own barriers and its own
// work between the halves; update() / write_row() compose them for the kernels that run a round in one go (k_reverse_warm, k_feat_warm).
//
// How the terms z are formed is NOT shared.  k_search_tiled and k_warm call fused_z<ACC>(has, ...): zeros under the branch on `has`.
// update() forms every lane's terms and selects zeros afterwards: under a divergent branch around fused_z in its callers' loops the
// gfx950 back end was seen to drop the PLANE vector's n_z component on one path (profiles/r06 notebook entry).  Either way a lane
// without a correspondence stages zeros; the hot kernels keep the code they were tuned with.
#pragma once
#include "search_device.hpp"

namespace cilhip {

template <int ACC>
struct WaveRank {
  typedef double double4_t __attribute__((ext_vector_type(4)));
  static constexpr int NC = FusedZ<ACC>::NC;
  static constexpr bool DUAL = NC <= 8;        // two groups of 4 correspondences per instruction: rows/cols 0-7 and 8-15
  double4_t acc = {0.0, 0.0, 0.0, 0.0};

  // the lane's terms -> the wave's scratch zb (FUSED_WAVE_BYTES).  DUAL: [64 correspondences][8 floats], the second half of the wave
  // 16 floats further (so that the two groups an instruction reads sit on different banks); else [64][NC].
  static __device__ __forceinline__ void stage(float* zb, int lane, const float (&z)[16]) {
    if (DUAL) {
      float4* w4 = reinterpret_cast<float4*>(zb + lane * 8 + (lane >= 32 ? 16 : 0));
      w4[0] = make_float4(z[0], z[1], z[2], z[3]);
      w4[1] = make_float4(z[4], z[5], z[6], z[7]);
    } else {
      float2* w2 = reinterpret_cast<float2*>(zb + lane * NC);
#pragma unroll
      for (int c = 0; c < NC / 2; ++c) w2[c] = make_float2(z[2 * c], z[2 * c + 1]);
    }
  }
  // the wave's 64 staged correspondences -> f64 operands -> the tile.  The caller's wave barriers around it: one after stage() (DS
  // operations of one wave execute in order: the reads see the writes), one before the scratch is staged again.
  static __device__ __forceinline__ void mfma_round(const float* zb, int lane, double4_t& acc) {
    if (DUAL) {
      const int comp = lane & 7, hf = (lane >> 3) & 1, k4 = lane >> 4;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int qi = hf * 32 + 4 * jj + k4;
        const double x = (double)zb[qi * 8 + hf * 16 + comp];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
      }
    } else {
      const int comp = lane & 15, k4 = lane >> 4;
#pragma unroll
      for (int jj = 0; jj < 16; ++jj) {
        const float f = zb[(4 * jj + k4) * NC + (comp < NC ? comp : 0)];
        const double x = comp < NC ? (double)f : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
      }
    }
  }
  // D[(lane >> 4) + 4 r][lane & 15] = acc[r]  ->  the wave's 16x16 tile in its own scratch (whose last readers are the wave's own
  // in-order DS reads: no barrier before it); a __syncthreads() of the caller between this and fold_row
  static __device__ __forceinline__ void store_tile(unsigned char* raw, int wave, int lane, const double4_t& acc) {
    double* const db = reinterpret_cast<double*>(raw + wave * FUSED_WAVE_BYTES);
#pragma unroll
    for (int r = 0; r < 4; ++r) db[r * 64 + lane] = acc[r];
  }
  // the block's row of SUMS_MAX sums: the NW waves' tiles added in wave order (fixed order: bitwise reproducible); raw: NW x
  // FUSED_WAVE_BYTES of LDS; every thread of the block calls this
  template <int NW>
  static __device__ __forceinline__ void fold_row(const unsigned char* raw, double* row) {
    if (threadIdx.x < SUMS_MAX) {
      int i1, j1, i2, j2;
      const bool used = FusedZ<ACC>::slot_terms((int)threadIdx.x, i1, j1, i2, j2);
      double v1 = 0.0, v2 = 0.0;
      if (used) {
        const int e1 = (i1 >> 2) * 64 + 16 * (i1 & 3) + j1, e1b = ((i1 + 8) >> 2) * 64 + 16 * ((i1 + 8) & 3) + j1 + 8;
        const int e2 = i2 >= 0 ? (i2 >> 2) * 64 + 16 * (i2 & 3) + j2 : 0, e2b = i2 >= 0 ? ((i2 + 8) >> 2) * 64 + 16 * ((i2 + 8) & 3) + j2 + 8 : 0;
        for (int w = 0; w < NW; ++w) {
          const double* dw = reinterpret_cast<const double*>(raw + w * FUSED_WAVE_BYTES);
          v1 += dw[e1];
          if (DUAL) v1 += dw[e1b];
          if (i2 >= 0) { v2 += dw[e2]; if (DUAL) v2 += dw[e2b]; }
        }
      }
      row[threadIdx.x] = v1 - v2;
    }
  }

  // one round in one go: the lane's correspondence (has: it has one) -> LDS -> the wave's tile (terms formed branch-free: above)
  __device__ __forceinline__ void update(float* zb, int lane, bool has, float qx, float qy, float qz, const float4 p, const float4 nv, const float* dmean, const float* smt) {
    float z[16];
    fused_z<ACC>(true, qx, qy, qz, p, nv, dmean, smt, z);
#pragma unroll
    for (int k = 0; k < 16; ++k) z[k] = has ? z[k] : 0.0f;
    stage(zb, lane, z);
    __builtin_amdgcn_wave_barrier();
    mfma_round(zb, lane, acc);
    __builtin_amdgcn_wave_barrier();
  }
  template <int NW>
  __device__ __forceinline__ void write_row(unsigned char* raw, int wave, int lane, double* row) {
    store_tile(raw, wave, lane, acc);
    __syncthreads();
    fold_row<NW>(raw, row);
  }
};

}  // namespace cilhip

// warp_field.hip -- non-rigid registration on a sparse warp field: cilantro's estimateSparseWarpFieldCombinedMetric for rigid 3-D
// transforms (registration/warp_field_estimation.hpp:1388-1846), resampleTransforms (registration/warp_field_utilities.hpp:14-48) and
// transformPoints with one transform per point.  DESIGN.md section 17 has the contract in full.
//
// The reference assembles a CSC Jacobian At per Gauss-Newton step, forms At * At^T as a sparse product and runs Eigen's
// Jacobi-preconditioned CG on it.  Here no matrix exists.  A data row touches at most k_ctrl control nodes x 6 unknowns and is kept as
// one 24-float record per source point (the rotation derivatives applied to s, the normal's dot products, the normalised weight, the
// residuals); a regularisation row touches 2 unknowns and is kept as one derivative and one residual per arc and component.
//   (A^T A) p  =  pass 1: u = A p   (one lane per source point, one lane per arc)
//                 pass 2: A^T u     (one wave per control node over its transposed lists: the (point, slot) pairs and the arcs naming it)
// Every sum is a gather in list order or a tree of fixed shape, accumulated in f64 and stored in f32; no floating-point atomics: two
// runs give the same bits.  CG follows Eigen's conjugate_gradient() with x0 = 0 (IterativeSolvers/ConjugateGradient.h); its scalars
// live in one device record, the vector updates and the convergence decision run in one 1024-thread block, and the host reads that
// record back once per WF_CG_BATCH iterations.
//
// The same with AFFINE node transforms (:1859-2234): 12 unknowns per node (the 3 x 3 row-major, then t), one
// 12-float record per source point (s_t, the normalised weights, the residuals, the normal), no polish on the way out or in the resample.
// The kernels whose only difference is the unknown count are templates on it (NU = 6 or 12); WfRec<NU> says where a record keeps what
// the gathers read.  The handle's scratch is sized for 6 at creation and grown on the first affine estimate.
//
// Set-up (cilhip_warp_field_create): the weights w_ij = eval(d2_ij), their totals in list order (:1456-1465) and the arc weights
// sqrt(eval(d2)) on the device; the two transposes by a counting sort on the host, once per (source, control graph) pair.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <new>
#include <vector>

#include "../../include/cilantro_hip/c_api.h"
#include "internal.hpp"
#include "search_device.hpp"
#include "solve.hpp"
#include "stateless.hpp"
#include "warp_field.hpp"

namespace cilhip {

namespace {

constexpr int WF_THREADS = 256;
constexpr int WF_MAX_BLOCKS = 256;      // lane-per-item kernels stride over the rest (one block per CU)
constexpr int WF_NODE_BLOCKS = 1024;    // wave-per-node kernels: 4 nodes per block and trip
constexpr int WF_CG_THREADS = 1024;
constexpr int WF_CG_BATCH = 8;          // CG iterations enqueued between two read-backs of the scalar record
constexpr int WF_ROW = 24;              // floats per source point's record
// record layout: [0..2] dRda^T s  [3..5] dRdb^T s  [6..8] dRdc^T s  [9] point weight / total  [10..12] point residuals
//                [13..15] n . (the three above)  [16..18] n  [19] plane weight / total  [20] plane residual  [21..23] unused
// the affine record (section 17.4, A3), 12 floats in the same buffer: [0..2] s_t  [3] point weight / total  [4] plane weight / total
//                [5..7] point residuals  [8..10] n  [11] plane residual
constexpr unsigned long long WF_LIMIT = 0xFFFFFFF0ull;

// where a record of NU unknowns per node keeps what the gathers read: its stride, the two normalised weights, the four residuals
template <int NU> struct WfRec;
template <> struct WfRec<6> { static constexpr int ROW = WF_ROW, WPT = 9, WPL = 19, BPT = 10, BPL = 20; };
template <> struct WfRec<12> { static constexpr int ROW = 12, WPT = 3, WPL = 4, BPT = 5, BPL = 11; };

struct WfScal {
  float abs_new, thr, rhs2, resid2, max_delta_sq;
  uint32_t iters, done, n_match;
};

struct WfGraph {
  uint32_t n_src, n_ctrl, k_ctrl, n_arcs;
  const uint32_t* ctrl_idx; const float* ctrl_w; const float* total_w;
  const uint32_t* node_ptr; const uint32_t* node_items;
  const uint32_t* arc_s; const uint32_t* arc_n; const float* arc_w;
  const uint32_t* anode_ptr; const uint32_t* anode_items;
};

inline unsigned wf_blocks(size_t n) { return (unsigned)std::min<size_t>((n + WF_THREADS - 1) / WF_THREADS, WF_MAX_BLOCKS); }
inline unsigned wf_node_blocks(size_t n) { return (unsigned)std::min<size_t>((n + 3) / 4, WF_NODE_BLOCKS); }

__device__ __forceinline__ double wf_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// the sum of v over a WF_CG_THREADS block, the same value in every thread; lds: 16 doubles
__device__ __forceinline__ double wf_block_sum(double v, double* lds) {
  v = wf_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int i = 0; i < WF_CG_THREADS / 64; ++i) t += lds[i];
  return t;
}

__device__ __forceinline__ float wf_sqrt_huber(float x, float delta) {
  const float xa = fabsf(x);
  return xa > delta ? __fsqrt_rn(delta * (xa - 0.5f * delta)) : __fsqrt_rn(0.5f) * xa;
}
__device__ __forceinline__ float wf_sqrt_huber_derivative(float x, float delta) {
  const float xa = fabsf(x);
  const float m = xa > delta ? delta / (2.0f * __fsqrt_rn(delta * (xa - 0.5f * delta))) : __fsqrt_rn(0.5f);
  return x < 0.0f ? -m : m;
}

// ---- set-up --------------------------------------------------------------------------------------------------------------------
__global__ void k_wf_ctrl_weights(uint32_t n, uint32_t k, const uint32_t* __restrict__ idx, const float* __restrict__ d2, int kind, float coeff, float* __restrict__ w_out,
                                  float* __restrict__ total) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float tot = 0.0f;
    for (uint32_t j = 0; j < k; ++j) {
      const size_t e = (size_t)i * k + j;
      float w = 0.0f;
      if (idx[e] != NONE_U32) { w = corr_weight(kind, coeff, d2[e]); tot = __fadd_rn(tot, w); }
      w_out[e] = w;
    }
    total[i] = tot;
  }
}

__global__ void k_wf_arc_weights(uint32_t n_arcs, const uint32_t* __restrict__ arc_pos, const float* __restrict__ d2, int kind, float coeff, float* __restrict__ w_out) {
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < n_arcs; a += gridDim.x * blockDim.x) w_out[a] = __fsqrt_rn(corr_weight(kind, coeff, d2[arc_pos[a]]));
}

// ---- one Gauss-Newton step: linearise ----------------------------------------------------------------------------------------------
__global__ void k_wf_count_matches(uint32_t n, uint32_t n_dst, const uint32_t* __restrict__ nn, WfScal* sc) {
  uint32_t mine = 0;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) mine += nn[i] < n_dst ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&sc->n_match, mine);
}

__global__ void k_wf_lin_points(WfGraph g, const float* __restrict__ tf, const float* __restrict__ dst, const float* __restrict__ nrm, uint32_t n_dst,
                                const float* __restrict__ src, const uint32_t* __restrict__ nn, float w_pt_sqrt, float w_pl_sqrt, float* __restrict__ rows) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n_src; i += gridDim.x * blockDim.x) {
    float* row = rows + (size_t)i * WF_ROW;
    const uint32_t m = nn[i];
    const float tot = g.total_w[i];
    if (m >= n_dst || tot == 0.0f) {      // no correspondence, or no control node in reach (:1687-1690): a row of zeros
#pragma unroll
      for (int q = 0; q < WF_ROW; ++q) row[q] = 0.0f;
      continue;
    }
    float ang[3] = {0.0f, 0.0f, 0.0f}, tr[3] = {0.0f, 0.0f, 0.0f};
    for (uint32_t j = 0; j < g.k_ctrl; ++j) {
      const size_t e = (size_t)i * g.k_ctrl + j;
      const uint32_t id = g.ctrl_idx[e];
      if (id == NONE_U32) continue;
      const float w = g.ctrl_w[e];
      const float* t6 = tf + 6 * (size_t)id;
#pragma unroll
      for (int c = 0; c < 3; ++c) { ang[c] += w * t6[c]; tr[c] += w * t6[3 + c]; }
    }
    const float inv = 1.0f / tot;
#pragma unroll
    for (int c = 0; c < 3; ++c) { ang[c] *= inv; tr[c] *= inv; }
    float sina, cosa, sinb, cosb, sinc, cosc;
    sincosf(ang[0], &sina, &cosa); sincosf(ang[1], &sinb, &cosb); sincosf(ang[2], &sinc, &cosc);
    // computeRotationTerms (:38-89): the matrices are stored transposed there, M(r, c) below is their (c, r)
    const float r00 = cosc * cosb, r01 = -sinc * cosa + cosc * sinb * sina, r02 = sinc * sina + cosc * sinb * cosa;
    const float r10 = sinc * cosb, r11 = cosc * cosa + sinc * sinb * sina, r12 = -cosc * sina + sinc * sinb * cosa;
    const float r20 = -sinb, r21 = cosb * sina, r22 = cosb * cosa;
    const float a01 = sinc * sina + cosc * sinb * cosa, a02 = sinc * cosa - cosc * sinb * sina;
    const float a11 = -cosc * sina + sinc * sinb * cosa, a12 = -cosc * cosa - sinc * sinb * sina;
    const float a21 = cosb * cosa, a22 = -cosb * sina;
    const float b00 = -cosc * sinb, b01 = cosc * cosb * sina, b02 = cosc * cosb * cosa;
    const float b10 = -sinc * sinb, b11 = sinc * cosb * sina, b12 = sinc * cosb * cosa;
    const float b20 = -cosb, b21 = -sinb * sina, b22 = -sinb * cosa;
    const float c00 = -sinc * cosb, c01 = -cosc * cosa - sinc * sinb * sina, c02 = cosc * sina - sinc * sinb * cosa;
    const float c10 = cosc * cosb, c11 = -sinc * cosa + cosc * sinb * sina, c12 = sinc * sina + cosc * sinb * cosa;
    const float sx = src[3 * (size_t)i], sy = src[3 * (size_t)i + 1], sz = src[3 * (size_t)i + 2];
    const float dx = dst[3 * (size_t)m], dy = dst[3 * (size_t)m + 1], dz = dst[3 * (size_t)m + 2];
    const float e0 = dx - ((r00 * sx + r01 * sy + r02 * sz) + tr[0]);
    const float e1 = dy - ((r10 * sx + r11 * sy + r12 * sz) + tr[1]);
    const float e2 = dz - ((r20 * sx + r21 * sy + r22 * sz) + tr[2]);
    const float da0 = 0.0f * sx + a01 * sy + a02 * sz, da1 = 0.0f * sx + a11 * sy + a12 * sz, da2 = 0.0f * sx + a21 * sy + a22 * sz;
    const float db0 = b00 * sx + b01 * sy + b02 * sz, db1 = b10 * sx + b11 * sy + b12 * sz, db2 = b20 * sx + b21 * sy + b22 * sz;
    const float dc0 = c00 * sx + c01 * sy + c02 * sz, dc1 = c10 * sx + c11 * sy + c12 * sz, dc2 = 0.0f;
    row[0] = da0; row[1] = da1; row[2] = da2; row[3] = db0; row[4] = db1; row[5] = db2; row[6] = dc0; row[7] = dc1; row[8] = dc2;
    row[9] = w_pt_sqrt / tot;
    row[10] = e0 * w_pt_sqrt; row[11] = e1 * w_pt_sqrt; row[12] = e2 * w_pt_sqrt;
    float n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (w_pl_sqrt != 0.0f) { n0 = nrm[3 * (size_t)m]; n1 = nrm[3 * (size_t)m + 1]; n2 = nrm[3 * (size_t)m + 2]; }
    row[13] = n0 * da0 + n1 * da1 + n2 * da2; row[14] = n0 * db0 + n1 * db1 + n2 * db2; row[15] = n0 * dc0 + n1 * dc1 + n2 * dc2;
    row[16] = n0; row[17] = n1; row[18] = n2;
    row[19] = w_pl_sqrt / tot;
    row[20] = (n0 * e0 + n1 * e1 + n2 * e2) * w_pl_sqrt;
    row[21] = row[22] = row[23] = 0.0f;
  }
}

// the affine unknowns start at the identity and a zero translation (:2004-2008): 12 per node, the 3 x 3 row-major, then t
__global__ void k_wf_affine_start(uint32_t n_ctrl, float* __restrict__ tf) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 12 * (size_t)n_ctrl; i += (size_t)gridDim.x * blockDim.x) {
    const uint32_t c = (uint32_t)(i % 12);
    tf[i] = (c == 0 || c == 4 || c == 8) ? 1.0f : 0.0f;
  }
}

// the affine record (A2, A3; :2050-2099, :2110-2163): blend in list order, scale by the reciprocal, s_t, the residuals
__global__ void k_wf_lin_points_affine(WfGraph g, const float* __restrict__ tf, const float* __restrict__ dst, const float* __restrict__ nrm, uint32_t n_dst,
                                       const float* __restrict__ src, const uint32_t* __restrict__ nn, float w_pt_sqrt, float w_pl_sqrt, float* __restrict__ rows) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n_src; i += gridDim.x * blockDim.x) {
    float* row = rows + (size_t)i * WfRec<12>::ROW;
    const uint32_t m = nn[i];
    const float tot = g.total_w[i];
    if (m >= n_dst || tot == 0.0f) {      // no correspondence, or both correspondence weights 0 (:2068-2071): a row of zeros
#pragma unroll
      for (int q = 0; q < WfRec<12>::ROW; ++q) row[q] = 0.0f;
      continue;
    }
    float lin[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, tr[3] = {0, 0, 0};
    for (uint32_t j = 0; j < g.k_ctrl; ++j) {
      const size_t e = (size_t)i * g.k_ctrl + j;
      const uint32_t id = g.ctrl_idx[e];
      if (id == NONE_U32) continue;
      const float w = g.ctrl_w[e];
      const float* t12 = tf + 12 * (size_t)id;
#pragma unroll
      for (int c = 0; c < 9; ++c) lin[c] += w * t12[c];
#pragma unroll
      for (int c = 0; c < 3; ++c) tr[c] += w * t12[9 + c];
    }
    const float inv = 1.0f / tot;
#pragma unroll
    for (int c = 0; c < 9; ++c) lin[c] *= inv;
#pragma unroll
    for (int c = 0; c < 3; ++c) tr[c] *= inv;
    const float sx = src[3 * (size_t)i], sy = src[3 * (size_t)i + 1], sz = src[3 * (size_t)i + 2];
    float st[3], e[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      st[r] = ((lin[3 * r] * sx + lin[3 * r + 1] * sy) + lin[3 * r + 2] * sz) + tr[r];
      e[r] = dst[3 * (size_t)m + r] - st[r];
    }
    float n[3] = {0.0f, 0.0f, 0.0f};
    if (w_pl_sqrt != 0.0f) { n[0] = nrm[3 * (size_t)m]; n[1] = nrm[3 * (size_t)m + 1]; n[2] = nrm[3 * (size_t)m + 2]; }
    row[0] = st[0]; row[1] = st[1]; row[2] = st[2];
    row[3] = w_pt_sqrt / tot; row[4] = w_pl_sqrt / tot;
    row[5] = w_pt_sqrt * e[0]; row[6] = w_pt_sqrt * e[1]; row[7] = w_pt_sqrt * e[2];
    row[8] = n[0]; row[9] = n[1]; row[10] = n[2];
    row[11] = ((n[0] * e[0] + n[1] * e[1]) + n[2] * e[2]) * w_pl_sqrt;
  }
}

template <int NU>
__global__ void k_wf_lin_arcs(WfGraph g, const float* __restrict__ tf, float w_reg_sqrt, float huber, float* __restrict__ arc_d, float* __restrict__ arc_b) {
  for (uint32_t a = blockIdx.x * blockDim.x + threadIdx.x; a < g.n_arcs; a += gridDim.x * blockDim.x) {
    const float w = w_reg_sqrt * g.arc_w[a];
    const float* ts = tf + NU * (size_t)g.arc_s[a];
    const float* tn = tf + NU * (size_t)g.arc_n[a];
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      const float diff = ts[c] - tn[c];
      arc_d[NU * (size_t)a + c] = w * wf_sqrt_huber_derivative(diff, huber);
      arc_b[NU * (size_t)a + c] = -w * wf_sqrt_huber(diff, huber);
    }
  }
}

// the coefficients of one (point, slot) pair: co[e][c] = row e (three point equations, one plane equation) x unknown c of the node
__device__ __forceinline__ void wf_coefficients(const float* __restrict__ row, float w, float co[4][6]) {
  const float wpt = row[9] * w, wpl = row[19] * w;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    co[e][0] = row[e] * wpt; co[e][1] = row[3 + e] * wpt; co[e][2] = row[6 + e] * wpt;
    co[e][3] = e == 0 ? wpt : 0.0f; co[e][4] = e == 1 ? wpt : 0.0f; co[e][5] = e == 2 ? wpt : 0.0f;
  }
  co[3][0] = row[13] * wpl; co[3][1] = row[14] * wpl; co[3][2] = row[15] * wpl;
  co[3][3] = row[16] * wpl; co[3][4] = row[17] * wpl; co[3][5] = row[18] * wpl;
}

// the affine rows (A3): the linear part's coefficients carry the TRANSFORMED point s_t, as the reference writes them (:2091, :2153)
__device__ __forceinline__ void wf_coefficients(const float* __restrict__ row, float w, float co[4][12]) {
  const float wpt = row[3] * w, wpl = row[4] * w;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
#pragma unroll
    for (int c = 0; c < 12; ++c) co[e][c] = 0.0f;
#pragma unroll
    for (int nz = 0; nz < 3; ++nz) co[e][3 * e + nz] = wpt * row[nz];
    co[e][9 + e] = wpt;
  }
#pragma unroll
  for (int blk = 0; blk < 3; ++blk) {
    const float wn = wpl * row[8 + blk];
#pragma unroll
    for (int cur = 0; cur < 3; ++cur) co[3][3 * blk + cur] = wn * row[cur];
    co[3][9 + blk] = wn;
  }
}

// A^T b and diag(A^T A), one wave per control node
template <int NU>
__global__ void k_wf_gather_rhs(WfGraph g, const float* __restrict__ rows, const float* __restrict__ arc_d, const float* __restrict__ arc_b, float* __restrict__ atb,
                                float* __restrict__ invdiag) {
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t node = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); node < g.n_ctrl; node += gridDim.x * (blockDim.x >> 6)) {
    using R = WfRec<NU>;
    double rb[NU], dg[NU];
#pragma unroll
    for (int c = 0; c < NU; ++c) rb[c] = dg[c] = 0.0;
    for (uint32_t q = g.node_ptr[node] + lane; q < g.node_ptr[node + 1]; q += 64) {
      const uint32_t item = g.node_items[q];
      const float* row = rows + (size_t)(item / g.k_ctrl) * R::ROW;
      float co[4][NU];
      wf_coefficients(row, g.ctrl_w[item], co);
      const float b[4] = {row[R::BPT], row[R::BPT + 1], row[R::BPT + 2], row[R::BPL]};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < NU; ++c) { rb[c] = fma((double)co[e][c], (double)b[e], rb[c]); dg[c] = fma((double)co[e][c], (double)co[e][c], dg[c]); }
    }
    for (uint32_t q = g.anode_ptr[node] + lane; q < g.anode_ptr[node + 1]; q += 64) {
      const uint32_t item = g.anode_items[q];
      const size_t a = item >> 1;
      const double sign = (item & 1u) ? -1.0 : 1.0;
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        const double d = (double)arc_d[NU * a + c];
        rb[c] = fma(sign * d, (double)arc_b[NU * a + c], rb[c]);
        dg[c] = fma(d, d, dg[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < NU; ++c) { rb[c] = wf_wave_sum(rb[c]); dg[c] = wf_wave_sum(dg[c]); }
    if (lane < NU) {
      double r = rb[0], d = dg[0];
#pragma unroll
      for (int c = 1; c < NU; ++c) if (lane == (uint32_t)c) { r = rb[c]; d = dg[c]; }
      const float df = (float)d;
      atb[NU * (size_t)node + lane] = (float)r;
      invdiag[NU * (size_t)node + lane] = df != 0.0f ? 1.0f / df : 1.0f;      // Eigen's DiagonalPreconditioner
    }
  }
}

// ---- the operator ------------------------------------------------------------------------------------------------------------------
// pass 1: u = A p.  Lanes [0, n_src) take a source point each, lanes [n_src, n_src + n_arcs) an arc each.
template <int NU>
__global__ void k_wf_apply_rows(WfGraph g, const float* __restrict__ rows, const float* __restrict__ arc_d, const float* __restrict__ p, const WfScal* __restrict__ sc,
                                float* __restrict__ u_pt, float* __restrict__ u_arc) {
  if (sc->done) return;
  const size_t total = (size_t)g.n_src + g.n_arcs;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (size_t)gridDim.x * blockDim.x) {
    if (t < g.n_src) {
      using R = WfRec<NU>;
      const float* row = rows + t * R::ROW;
      double u[4] = {0, 0, 0, 0};
      if (row[R::WPT] != 0.0f || row[R::WPL] != 0.0f) {
        for (uint32_t j = 0; j < g.k_ctrl; ++j) {
          const size_t e = t * g.k_ctrl + j;
          const uint32_t id = g.ctrl_idx[e];
          if (id == NONE_U32) continue;
          float co[4][NU];
          wf_coefficients(row, g.ctrl_w[e], co);
          const float* p6 = p + NU * (size_t)id;
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int c = 0; c < NU; ++c) u[q] = fma((double)co[q][c], (double)p6[c], u[q]);
        }
      }
      *reinterpret_cast<float4*>(u_pt + 4 * t) = make_float4((float)u[0], (float)u[1], (float)u[2], (float)u[3]);
    } else {
      const size_t a = t - g.n_src;
      const float* ps = p + NU * (size_t)g.arc_s[a];
      const float* pn = p + NU * (size_t)g.arc_n[a];
#pragma unroll
      for (int c = 0; c < NU; ++c) {
        const double d = (double)arc_d[NU * a + c];
        u_arc[NU * a + c] = (float)fma(d, (double)ps[c], -(d * (double)pn[c]));
      }
    }
  }
}

// pass 2: tmp = A^T u, one wave per control node; node_dot[node] = the node's NU terms of p . tmp
template <int NU>
__global__ void k_wf_apply_nodes(WfGraph g, const float* __restrict__ rows, const float* __restrict__ arc_d, const float* __restrict__ u_pt, const float* __restrict__ u_arc,
                                 const float* __restrict__ p, const WfScal* __restrict__ sc, float* __restrict__ tmp, double* __restrict__ node_dot) {
  if (sc->done) return;
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t node = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); node < g.n_ctrl; node += gridDim.x * (blockDim.x >> 6)) {
    double acc[NU];
#pragma unroll
    for (int c = 0; c < NU; ++c) acc[c] = 0.0;
    for (uint32_t q = g.node_ptr[node] + lane; q < g.node_ptr[node + 1]; q += 64) {
      const uint32_t item = g.node_items[q];
      const size_t i = item / g.k_ctrl;
      float co[4][NU];
      wf_coefficients(rows + i * WfRec<NU>::ROW, g.ctrl_w[item], co);
      const float4 u = *reinterpret_cast<const float4*>(u_pt + 4 * i);
      const float uu[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int c = 0; c < NU; ++c) acc[c] = fma((double)co[e][c], (double)uu[e], acc[c]);
    }
    for (uint32_t q = g.anode_ptr[node] + lane; q < g.anode_ptr[node + 1]; q += 64) {
      const uint32_t item = g.anode_items[q];
      const size_t a = item >> 1;
      const double sign = (item & 1u) ? -1.0 : 1.0;
#pragma unroll
      for (int c = 0; c < NU; ++c) acc[c] = fma(sign * (double)arc_d[NU * a + c], (double)u_arc[NU * a + c], acc[c]);
    }
    double dot = 0.0;
#pragma unroll
    for (int c = 0; c < NU; ++c) {
      const float v = (float)wf_wave_sum(acc[c]);
      if (lane == 0) tmp[NU * (size_t)node + c] = v;
      dot = fma((double)p[NU * (size_t)node + c], (double)v, dot);
    }
    if (lane == 0) node_dot[node] = dot;
  }
}

// ---- CG: Eigen's conjugate_gradient(), one block ---------------------------------------------------------------------------------
__global__ __launch_bounds__(WF_CG_THREADS) void k_wf_cg_init(uint32_t n6, const float* __restrict__ atb, const float* __restrict__ invdiag, float* __restrict__ x,
                                                              float* __restrict__ r, float* __restrict__ p, WfScal* sc, float tol, uint32_t max_cg) {
  __shared__ double lds[16];
  double rhs2 = 0.0;
  for (uint32_t i = threadIdx.x; i < n6; i += WF_CG_THREADS) {
    const float b = atb[i];
    x[i] = 0.0f; r[i] = b;
    rhs2 = fma((double)b, (double)b, rhs2);
  }
  rhs2 = wf_block_sum(rhs2, lds);
  const float rhs2f = (float)rhs2;
  const float thr = fmaxf(tol * tol * rhs2f, FLT_MIN);
  const bool stop = rhs2f == 0.0f || rhs2f < thr || max_cg == 0;      // (x = 0 in all three; the residual test precedes the first iteration)
  double rz = 0.0;
  if (!stop)
    for (uint32_t i = threadIdx.x; i < n6; i += WF_CG_THREADS) {
      const float z = invdiag[i] * r[i];
      p[i] = z;
      rz = fma((double)r[i], (double)z, rz);
    }
  rz = wf_block_sum(rz, lds);
  if (threadIdx.x == 0) { sc->abs_new = (float)rz; sc->thr = thr; sc->rhs2 = rhs2f; sc->resid2 = rhs2f; sc->iters = 0; sc->done = stop ? 1u : 0u; }
}

__global__ __launch_bounds__(WF_CG_THREADS) void k_wf_cg_update(uint32_t n6, uint32_t n_ctrl, const double* __restrict__ node_dot, const float* __restrict__ tmp,
                                                                const float* __restrict__ invdiag, float* __restrict__ x, float* __restrict__ r, float* __restrict__ p,
                                                                WfScal* sc, uint32_t max_cg) {
  __shared__ double lds[16];
  __shared__ WfScal s0;
  if (threadIdx.x == 0) s0 = *sc;
  __syncthreads();
  if (s0.done) return;
  const float abs_old = s0.abs_new, thr = s0.thr;
  double pap = 0.0;
  for (uint32_t i = threadIdx.x; i < n_ctrl; i += WF_CG_THREADS) pap += node_dot[i];
  pap = wf_block_sum(pap, lds);
  const float alpha = abs_old / (float)pap;
  double r2 = 0.0;
  for (uint32_t i = threadIdx.x; i < n6; i += WF_CG_THREADS) {
    x[i] = x[i] + alpha * p[i];
    const float ri = r[i] - alpha * tmp[i];
    r[i] = ri;
    r2 = fma((double)ri, (double)ri, r2);
  }
  r2 = wf_block_sum(r2, lds);
  const float resid2 = (float)r2;
  if (resid2 < thr) {      // (the iteration that meets the threshold is not counted: Eigen leaves the loop before i++)
    if (threadIdx.x == 0) { sc->resid2 = resid2; sc->done = 1u; }
    return;
  }
  double rz = 0.0;
  for (uint32_t i = threadIdx.x; i < n6; i += WF_CG_THREADS) rz = fma((double)r[i], (double)(invdiag[i] * r[i]), rz);
  rz = wf_block_sum(rz, lds);
  const float abs_new = (float)rz;
  const float beta = abs_new / abs_old;
  for (uint32_t i = threadIdx.x; i < n6; i += WF_CG_THREADS) p[i] = invdiag[i] * r[i] + beta * p[i];
  if (threadIdx.x == 0) {
    sc->abs_new = abs_new; sc->resid2 = resid2; sc->iters = s0.iters + 1u;
    sc->done = s0.iters + 1u >= max_cg ? 1u : 0u;
  }
}

// ---- epilogue --------------------------------------------------------------------------------------------------------------------
// tforms_vec += delta; max_delta_sq = max over the nodes of |delta_node|^2 (:1814-1824)
template <int NU>
__global__ __launch_bounds__(WF_CG_THREADS) void k_wf_gn_update(uint32_t n_ctrl, const float* __restrict__ x, float* __restrict__ tf, WfScal* sc) {
  __shared__ float lds[16];
  float mx = 0.0f;
  for (uint32_t node = threadIdx.x; node < n_ctrl; node += WF_CG_THREADS) {
    float d2 = 0.0f;
#pragma unroll
    for (int c = 0; c < NU; ++c) { const float v = x[NU * (size_t)node + c]; d2 += v * v; tf[NU * (size_t)node + c] += v; }
    if (d2 > mx) mx = d2;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < WF_CG_THREADS / 64; ++i) mx = fmaxf(mx, lds[i]);
    sc->max_delta_sq = mx;
  }
}

// the rotation() polish of space_transformations.hpp:43-51 on a row-major 3 x 3
__device__ __forceinline__ void wf_polish(const float L[9], float R[9]) {
  double Lin[9], Rd[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Lin[i] = (double)L[i];
  if (!nearest_rotation_polar(Lin, Rd)) nearest_rotation(Lin, Rd);
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (float)Rd[i];
}
__device__ __forceinline__ void wf_store_T(float* T, const float R[9], float t0, float t1, float t2) {      // column-major 4 x 4
  T[0] = R[0]; T[1] = R[3]; T[2] = R[6]; T[3] = 0.0f; T[4] = R[1]; T[5] = R[4]; T[6] = R[7]; T[7] = 0.0f;
  T[8] = R[2]; T[9] = R[5]; T[10] = R[8]; T[11] = 0.0f; T[12] = t0; T[13] = t1; T[14] = t2; T[15] = 1.0f;
}

// (a, b, c, t) -> Rz(c) Ry(b) Rx(a), polished, and t (:1833-1843)
__global__ void k_wf_to_transforms(uint32_t n_ctrl, const float* __restrict__ tf, float* __restrict__ T) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_ctrl; i += gridDim.x * blockDim.x) {
    const float* t6 = tf + 6 * (size_t)i;
    float sina, cosa, sinb, cosb, sinc, cosc;
    sincosf(t6[0], &sina, &cosa); sincosf(t6[1], &sinb, &cosb); sincosf(t6[2], &sinc, &cosc);
    const float L[9] = {cosc * cosb, -sinc * cosa + cosc * sinb * sina, sinc * sina + cosc * sinb * cosa,
                        sinc * cosb, cosc * cosa + sinc * sinb * sina,  -cosc * sina + sinc * sinb * cosa,
                        -sinb,       cosb * sina,                       cosb * cosa};
    float R[9];
    wf_polish(L, R);
    wf_store_T(T + 16 * (size_t)i, R, t6[3], t6[4], t6[5]);
  }
}

// the affine unknowns are copied out as they are (:2222-2231): no rotation()
__global__ void k_wf_to_transforms_affine(uint32_t n_ctrl, const float* __restrict__ tf, float* __restrict__ T) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_ctrl; i += gridDim.x * blockDim.x) {
    const float* t12 = tf + 12 * (size_t)i;
    float L[9];
#pragma unroll
    for (int q = 0; q < 9; ++q) L[q] = t12[q];
    wf_store_T(T + 16 * (size_t)i, L, t12[9], t12[10], t12[11]);
  }
}

__global__ void k_wf_identity(size_t n, float* __restrict__ T) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < 16 * n; i += (size_t)gridDim.x * blockDim.x) T[i] = (i & 15) % 5 == 0 ? 1.0f : 0.0f;
}

// resampleTransforms, the list overload (warp_field_utilities.hpp:14-48), with the weights of the set-up; POLISH: through rotation()
// (the Isometry mode), otherwise the blend as it is (A7)
template <bool POLISH>
__global__ void k_wf_resample(WfGraph g, const float* __restrict__ ctrl_T, float* __restrict__ dense_T) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < g.n_src; i += gridDim.x * blockDim.x) {
    float L[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t[3] = {0, 0, 0};
    float tot = 0.0f;
    for (uint32_t j = 0; j < g.k_ctrl; ++j) {
      const size_t e = (size_t)i * g.k_ctrl + j;
      const uint32_t id = g.ctrl_idx[e];
      if (id == NONE_U32) continue;
      const float w = g.ctrl_w[e];
      const float* T = ctrl_T + 16 * (size_t)id;
      tot = __fadd_rn(tot, w);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) L[3 * r + c] += w * T[4 * c + r];
        t[r] += w * T[12 + r];
      }
    }
    float R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (tot == 0.0f) { t[0] = t[1] = t[2] = 0.0f; }
    else {
      const float inv = 1.0f / tot;
#pragma unroll
      for (int q = 0; q < 9; ++q) L[q] *= inv;
      if (POLISH) wf_polish(L, R);
      else {
#pragma unroll
        for (int q = 0; q < 9; ++q) R[q] = L[q];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) t[q] *= inv;
    }
    wf_store_T(dense_T + 16 * (size_t)i, R, t[0], t[1], t[2]);
  }
}

// out = T_i * s_i: ((L0 x + L1 y) + L2 z) + t, every operation rounded once (pinned like the project's T * s)
__global__ void k_wf_transform_points(size_t n, const float* __restrict__ T, const float* __restrict__ xyz, float* __restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float* M = T + 16 * i;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
#pragma unroll
    for (int r = 0; r < 3; ++r) out[3 * i + r] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[r], x), __fmul_rn(M[4 + r], y)), __fmul_rn(M[8 + r], z)), M[12 + r]);
  }
}

// T[i] = It[i] * T[i]; delta[i] = |R_it - I|_F^2 + |t_it|^2 (icp_warp_field_combined_metric_sparse.hpp:227-238)
__global__ void k_wf_compose(uint32_t n, const float* __restrict__ It, float* __restrict__ T, float* __restrict__ delta) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const float* A = It + 16 * (size_t)i;
    float* B = T + 16 * (size_t)i;
    float out[16];
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) out[4 * c + r] = ((A[r] * B[4 * c] + A[4 + r] * B[4 * c + 1]) + A[8 + r] * B[4 * c + 2]) + (c == 3 ? A[12 + r] : 0.0f);
    out[3] = out[7] = out[11] = 0.0f; out[15] = 1.0f;
    float d2 = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < 3; ++r) { const float v = A[4 * c + r] - (r == c ? 1.0f : 0.0f); d2 += v * v; }
#pragma unroll
    for (int r = 0; r < 3; ++r) d2 += A[12 + r] * A[12 + r];
#pragma unroll
    for (int q = 0; q < 16; ++q) B[q] = out[q];
    delta[i] = d2;
  }
}
__global__ __launch_bounds__(WF_CG_THREADS) void k_wf_max(uint32_t n, const float* __restrict__ v, WfScal* sc) {
  __shared__ float lds[16];
  float mx = 0.0f;
  for (uint32_t i = threadIdx.x; i < n; i += WF_CG_THREADS) if (v[i] > mx) mx = v[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int i = 1; i < WF_CG_THREADS / 64; ++i) mx = fmaxf(mx, lds[i]);
    sc->max_delta_sq = mx;
  }
}

__global__ void k_wf_unsort_target(uint32_t n, const float4* __restrict__ pts, const float4* __restrict__ nrm, float* __restrict__ xyz, float* __restrict__ out_n) {
  for (uint32_t j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
    const float4 p = pts[j];
    const uint32_t i = __float_as_uint(p.w);
    if (i >= n) continue;
    xyz[3 * (size_t)i] = p.x; xyz[3 * (size_t)i + 1] = p.y; xyz[3 * (size_t)i + 2] = p.z;
    if (nrm) { const float4 q = nrm[j]; out_n[3 * (size_t)i] = q.x; out_n[3 * (size_t)i + 1] = q.y; out_n[3 * (size_t)i + 2] = q.z; }
  }
}

inline bool wf_finite(float v) { return std::isfinite(v); }

}  // namespace

}  // namespace cilhip

// the graph of the set-up and the solver's scratch, device-resident
struct cilhip_warp_field {
  int device = 0;
  size_t n_src = 0, n_ctrl = 0, k_ctrl = 0, k_reg = 0, n_arcs = 0;
  cilhip::DevBuf<uint32_t> ctrl_idx, node_ptr, node_items, arc_s, arc_n, anode_ptr, anode_items;
  cilhip::DevBuf<float> ctrl_w, total_w, arc_w;
  cilhip::DevBuf<float> rows, u_pt, arc_d, arc_b, u_arc, vec;      // vec: tf, atb, invdiag, x, r, p, tmp (6 n_ctrl each), then n_ctrl deltas
  cilhip::DevBuf<double> node_dot;
  cilhip::DevBuf<cilhip::WfScal> sc;
  cilhip::DevBuf<float> loop[7];
  cilhip::DevBuf<uint32_t> loop_nn;
  cilhip::StreamGuard st;      // (last: drained and destroyed before the buffers)

  cilhip::WfGraph graph() const {
    return cilhip::WfGraph{(uint32_t)n_src, (uint32_t)n_ctrl, (uint32_t)k_ctrl, (uint32_t)n_arcs, ctrl_idx, ctrl_w, total_w, node_ptr, node_items, arc_s, arc_n, arc_w, anode_ptr, anode_items};
  }
  float* v(int which, int nu = 6) const { return vec.get() + (size_t)which * nu * n_ctrl; }
  // the solver's scratch is sized for 6 unknowns per node at creation; the first affine call grows it to 12 (contents are per call)
  hipError_t grow(int nu) {
    hipError_t e = vec.ensure((size_t)7 * nu * n_ctrl + n_ctrl);
    if (e == hipSuccess) e = arc_d.ensure(nu * n_arcs);
    if (e == hipSuccess) e = arc_b.ensure(nu * n_arcs);
    if (e == hipSuccess) e = u_arc.ensure(nu * n_arcs);
    return e;
  }
};

namespace cilhip {

size_t wf_n_src(const cilhip_warp_field* wf) { return wf->n_src; }
size_t wf_n_ctrl(const cilhip_warp_field* wf) { return wf->n_ctrl; }
int wf_device(const cilhip_warp_field* wf) { return wf->device; }
hipStream_t wf_stream(cilhip_warp_field* wf) { return wf->st.s; }

const char* wf_params_refusal(const cilhip_warp_params* p) {
  if (!p) return "params is null";
  if (!wf_finite(p->w_p2p) || !wf_finite(p->w_p2pl) || !wf_finite(p->w_reg) || !wf_finite(p->huber_boundary) || !wf_finite(p->gn_conv_tol) || !wf_finite(p->cg_conv_tol))
    return "a parameter is not finite";
  if (p->w_p2p < 0.0f || p->w_p2pl < 0.0f || p->w_reg < 0.0f) return "a metric or regularisation weight is negative";
  if (!(p->huber_boundary > 0.0f)) return "huber_boundary must be positive";
  if ((unsigned long long)p->max_gn_iter >= WF_LIMIT || (unsigned long long)p->max_cg_iter >= WF_LIMIT) return "an iteration limit must be below 2^32 - 16";
  return nullptr;
}

int wf_set_identity_dev(const char* F, hipStream_t s, float* d_T, size_t n) {
  if (!n) return CILHIP_OK;
  hipLaunchKernelGGL(k_wf_identity, dim3(wf_blocks(16 * n)), dim3(WF_THREADS), 0, s, n, d_T);
  ST_CK(F, hipGetLastError());
  return CILHIP_OK;
}

int wf_resample_dev(const char* F, cilhip_warp_field* wf, const float* d_ctrl_T, float* d_dense_T, WfKind kind) {
  if (kind == WF_AFFINE) hipLaunchKernelGGL(k_wf_resample<false>, dim3(wf_blocks(wf->n_src)), dim3(WF_THREADS), 0, wf->st.s, wf->graph(), d_ctrl_T, d_dense_T);
  else hipLaunchKernelGGL(k_wf_resample<true>, dim3(wf_blocks(wf->n_src)), dim3(WF_THREADS), 0, wf->st.s, wf->graph(), d_ctrl_T, d_dense_T);
  ST_CK(F, hipGetLastError());
  return CILHIP_OK;
}

int wf_transform_points_dev(const char* F, hipStream_t s, const float* d_T, const float* d_xyz, size_t n, float* d_out) {
  if (!n) return CILHIP_OK;
  hipLaunchKernelGGL(k_wf_transform_points, dim3(wf_blocks(n)), dim3(WF_THREADS), 0, s, n, d_T, d_xyz, d_out);
  ST_CK(F, hipGetLastError());
  return CILHIP_OK;
}

int wf_compose_dev(const char* F, cilhip_warp_field* wf, const float* d_T_iter, float* d_T, float* max_delta_sq) {
  hipStream_t s = wf->st.s;
  float* delta = wf->v(7);
  hipLaunchKernelGGL(k_wf_compose, dim3(wf_blocks(wf->n_ctrl)), dim3(WF_THREADS), 0, s, (uint32_t)wf->n_ctrl, d_T_iter, d_T, delta);
  ST_CK(F, hipGetLastError());
  hipLaunchKernelGGL(k_wf_max, dim3(1), dim3(WF_CG_THREADS), 0, s, (uint32_t)wf->n_ctrl, (const float*)delta, wf->sc.get());
  ST_CK(F, hipGetLastError());
  WfScal h{};
  ST_CK(F, hipMemcpyAsync(&h, wf->sc.get(), sizeof(WfScal), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  *max_delta_sq = h.max_delta_sq;
  return CILHIP_OK;
}

int wf_loop_buffers(const char* F, cilhip_warp_field* wf, size_t n_dst, float* bufs[7], uint32_t** nn) {
  const size_t want[7] = {3 * wf->n_src, 3 * wf->n_src, 16 * wf->n_src, 16 * wf->n_ctrl, 16 * wf->n_ctrl, 3 * n_dst, 3 * n_dst};
  for (int i = 0; i < 7; ++i) { ST_CK(F, wf->loop[i].ensure(want[i])); bufs[i] = wf->loop[i].get(); }
  ST_CK(F, wf->loop_nn.ensure(wf->n_src));
  *nn = wf->loop_nn.get();
  return CILHIP_OK;
}

int wf_unsort_target_dev(const char* F, hipStream_t s, const float4* pts, const float4* nrm, uint32_t n, float* d_xyz, float* d_nrm) {
  if (!n) return CILHIP_OK;
  hipLaunchKernelGGL(k_wf_unsort_target, dim3(wf_blocks(n)), dim3(WF_THREADS), 0, s, n, pts, nrm, d_xyz, d_nrm);
  ST_CK(F, hipGetLastError());
  return CILHIP_OK;
}

namespace {

// the Gauss-Newton loop over NU unknowns per node: 6 = (a, b, c, t) of section 17.1, 12 = (L row-major, t) of section 17.4
template <int NU>
int wf_estimate_impl(const char* F, cilhip_warp_field* wf, const float* d_dst, const float* d_nrm, size_t n_dst, const float* d_src, const uint32_t* d_nn,
                     const cilhip_warp_params& prm, float* d_T_out, cilhip_warp_stats* stats) {
  hipStream_t s = wf->st.s;
  if (NU != 6) ST_CK(F, wf->grow(NU));
  const WfGraph g = wf->graph();
  const uint32_t n6 = (uint32_t)(NU * wf->n_ctrl);
  cilhip_warp_stats st{0, 0, 0u, 0.0f, 0.0f};
  WfScal h{};
  float *tf = wf->v(0, NU), *atb = wf->v(1, NU), *invdiag = wf->v(2, NU), *x = wf->v(3, NU), *r = wf->v(4, NU), *p = wf->v(5, NU), *tmp = wf->v(6, NU);
  WfScal* sc = wf->sc.get();
  const bool has_pt = prm.w_p2p > 0.0f, has_pl = prm.w_p2pl > 0.0f;
  ST_CK(F, hipMemsetAsync(sc, 0, sizeof(WfScal), s));
  if (NU == 6) ST_CK(F, hipMemsetAsync(tf, 0, (size_t)n6 * sizeof(float), s));
  else {
    hipLaunchKernelGGL(k_wf_affine_start, dim3(wf_blocks(n6)), dim3(WF_THREADS), 0, s, g.n_ctrl, tf);
    ST_CK(F, hipGetLastError());
  }
  if (has_pt || has_pl) {
    hipLaunchKernelGGL(k_wf_count_matches, dim3(wf_blocks(wf->n_src)), dim3(WF_THREADS), 0, s, g.n_src, (uint32_t)n_dst, d_nn, sc);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(&h, sc, sizeof(WfScal), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
  }
  if (h.n_match == 0) {      // no data term: identity transforms, not converged (:1427-1433)
    if (const int rc = wf_set_identity_dev(F, s, d_T_out, wf->n_ctrl)) return rc;
    ST_CK(F, hipStreamSynchronize(s));
    if (stats) *stats = st;
    return CILHIP_OK;
  }
  const float w_pt_sqrt = has_pt ? std::sqrt(prm.w_p2p) : 0.0f, w_pl_sqrt = has_pl ? std::sqrt(prm.w_p2pl) : 0.0f, w_reg_sqrt = std::sqrt(prm.w_reg);
  const float gn_tol_sq = prm.gn_conv_tol * prm.gn_conv_tol;
  const uint32_t max_cg = (uint32_t)prm.max_cg_iter;
  const unsigned row_blocks = wf_blocks(wf->n_src + wf->n_arcs), node_blocks = wf_node_blocks(wf->n_ctrl);
  while ((size_t)st.gn_iterations < prm.max_gn_iter) {
    hipLaunchKernelGGL(NU == 6 ? k_wf_lin_points : k_wf_lin_points_affine, dim3(wf_blocks(wf->n_src)), dim3(WF_THREADS), 0, s, g, (const float*)tf, d_dst, d_nrm, (uint32_t)n_dst, d_src,
                       d_nn, w_pt_sqrt, w_pl_sqrt, wf->rows.get());
    ST_CK(F, hipGetLastError());
    if (wf->n_arcs) {
      hipLaunchKernelGGL(k_wf_lin_arcs<NU>, dim3(wf_blocks(wf->n_arcs)), dim3(WF_THREADS), 0, s, g, (const float*)tf, w_reg_sqrt, prm.huber_boundary, wf->arc_d.get(), wf->arc_b.get());
      ST_CK(F, hipGetLastError());
    }
    hipLaunchKernelGGL(k_wf_gather_rhs<NU>, dim3(node_blocks), dim3(WF_THREADS), 0, s, g, (const float*)wf->rows.get(), (const float*)wf->arc_d.get(), (const float*)wf->arc_b.get(), atb,
                       invdiag);
    ST_CK(F, hipGetLastError());
    hipLaunchKernelGGL(k_wf_cg_init, dim3(1), dim3(WF_CG_THREADS), 0, s, n6, (const float*)atb, (const float*)invdiag, x, r, p, sc, prm.cg_conv_tol, max_cg);
    ST_CK(F, hipGetLastError());
    for (uint32_t launched = 0; launched < max_cg;) {
      const uint32_t batch = std::min<uint32_t>(WF_CG_BATCH, max_cg - launched);
      for (uint32_t b = 0; b < batch; ++b) {
        hipLaunchKernelGGL(k_wf_apply_rows<NU>, dim3(row_blocks), dim3(WF_THREADS), 0, s, g, (const float*)wf->rows.get(), (const float*)wf->arc_d.get(), (const float*)p,
                           (const WfScal*)sc, wf->u_pt.get(), wf->u_arc.get());
        hipLaunchKernelGGL(k_wf_apply_nodes<NU>, dim3(node_blocks), dim3(WF_THREADS), 0, s, g, (const float*)wf->rows.get(), (const float*)wf->arc_d.get(), (const float*)wf->u_pt.get(),
                           (const float*)wf->u_arc.get(), (const float*)p, (const WfScal*)sc, tmp, wf->node_dot.get());
        hipLaunchKernelGGL(k_wf_cg_update, dim3(1), dim3(WF_CG_THREADS), 0, s, n6, g.n_ctrl, (const double*)wf->node_dot.get(), (const float*)tmp, (const float*)invdiag, x, r, p, sc,
                           max_cg);
      }
      ST_CK(F, hipGetLastError());
      launched += batch;
      ST_CK(F, hipMemcpyAsync(&h, sc, sizeof(WfScal), hipMemcpyDeviceToHost, s));
      ST_CK(F, hipStreamSynchronize(s));
      if (h.done) break;
    }
    hipLaunchKernelGGL(k_wf_gn_update<NU>, dim3(1), dim3(WF_CG_THREADS), 0, s, g.n_ctrl, (const float*)x, tf, sc);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(&h, sc, sizeof(WfScal), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    st.gn_iterations += 1;
    st.cg_iterations_total += h.iters;
    st.last_cg_residual_norm2 = h.resid2;
    st.max_delta_sq = h.max_delta_sq;
    if (h.max_delta_sq < gn_tol_sq) { st.converged = 1; break; }
  }
  hipLaunchKernelGGL(NU == 6 ? k_wf_to_transforms : k_wf_to_transforms_affine, dim3(wf_blocks(wf->n_ctrl)), dim3(WF_THREADS), 0, s, g.n_ctrl, (const float*)tf, d_T_out);
  ST_CK(F, hipGetLastError());
  ST_CK(F, hipStreamSynchronize(s));
  if (stats) *stats = st;
  return CILHIP_OK;
}

}  // namespace

int wf_estimate_dev(const char* F, cilhip_warp_field* wf, const float* d_dst, const float* d_nrm, size_t n_dst, const float* d_src, const uint32_t* d_nn,
                    const cilhip_warp_params& prm, float* d_T_out, cilhip_warp_stats* stats, WfKind kind) {
  return kind == WF_AFFINE ? wf_estimate_impl<12>(F, wf, d_dst, d_nrm, n_dst, d_src, d_nn, prm, d_T_out, stats)
                           : wf_estimate_impl<6>(F, wf, d_dst, d_nrm, n_dst, d_src, d_nn, prm, d_T_out, stats);
}

namespace {

struct WfLists { const uint32_t* idx; const float* d2; size_t k; int kernel; float sigma; };

const char* wf_check_indices(const uint32_t* idx, size_t n, size_t n_ctrl) {
  for (size_t i = 0; i < n; ++i)
    if (idx[i] != NONE_U32 && idx[i] >= n_ctrl) return "a list names a control node >= n_ctrl (0xFFFFFFFF is the only padding value)";
  return nullptr;
}

int wf_create(int device, size_t n_src, size_t n_ctrl, const WfLists& ctrl, const WfLists& reg, int mem, cilhip_warp_field** out) {
  constexpr const char* F = "warp_field_create";
  if (const int open = st_open(F, device)) return open;
  std::unique_ptr<cilhip_warp_field> wf(new cilhip_warp_field());
  wf->device = device; wf->n_src = n_src; wf->n_ctrl = n_ctrl; wf->k_ctrl = ctrl.k; wf->k_reg = reg.k;
  ST_CK(F, wf->st.create());
  hipStream_t s = wf->st.s;
  const size_t nc = n_src * ctrl.k, nr = n_ctrl * reg.k;
  // the index lists on the host: the transposes are a counting sort there
  std::vector<uint32_t> hold_c, hold_r;
  const uint32_t *ci = ctrl.idx, *ri = reg.idx;
  if (mem == CILHIP_MEM_DEVICE) {
    hold_c.resize(nc); hold_r.resize(nr);
    ST_CK(F, hipMemcpyAsync(hold_c.data(), ctrl.idx, nc * 4, hipMemcpyDeviceToHost, s));
    ST_CK(F, hipMemcpyAsync(hold_r.data(), reg.idx, nr * 4, hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    ci = hold_c.data(); ri = hold_r.data();
    const char* bad = wf_check_indices(ci, nc, n_ctrl);
    if (!bad) bad = wf_check_indices(ri, nr, n_ctrl);
    if (bad) return st_fail(CILHIP_ERR_INVALID, F, bad);
  }
  std::vector<uint32_t> node_ptr(n_ctrl + 1, 0), node_items;
  for (size_t e = 0; e < nc; ++e) if (ci[e] != NONE_U32) node_ptr[ci[e] + 1]++;
  for (size_t i = 0; i < n_ctrl; ++i) node_ptr[i + 1] += node_ptr[i];
  node_items.resize(std::max<size_t>(node_ptr[n_ctrl], 1));
  {
    std::vector<uint32_t> fill(node_ptr.begin(), node_ptr.end() - 1);
    for (size_t e = 0; e < nc; ++e) if (ci[e] != NONE_U32) node_items[fill[ci[e]]++] = (uint32_t)e;      // ascending source index, then slot
  }
  // arcs (:1736-1748): row i, entries j >= 1 -> (neighbors[0], neighbors[j]), the lower unknown offset first
  std::vector<uint32_t> arc_s, arc_n, arc_pos;
  for (size_t i = 0; i < n_ctrl; ++i) {
    const uint32_t owner = ri[i * reg.k];
    if (owner == NONE_U32) continue;
    for (size_t j = 1; j < reg.k; ++j) {
      const uint32_t nb = ri[i * reg.k + j];
      if (nb == NONE_U32) continue;
      arc_s.push_back(std::min(owner, nb)); arc_n.push_back(std::max(owner, nb)); arc_pos.push_back((uint32_t)(i * reg.k + j));
    }
  }
  const size_t n_arcs = arc_s.size();
  if ((unsigned long long)n_arcs * 2 >= WF_LIMIT) return st_fail(CILHIP_ERR_INVALID, F, "too many regularisation arcs");
  wf->n_arcs = n_arcs;
  std::vector<uint32_t> anode_ptr(n_ctrl + 1, 0), anode_items(std::max<size_t>(2 * n_arcs, 1));
  for (size_t a = 0; a < n_arcs; ++a) { anode_ptr[arc_s[a] + 1]++; anode_ptr[arc_n[a] + 1]++; }
  for (size_t i = 0; i < n_ctrl; ++i) anode_ptr[i + 1] += anode_ptr[i];
  {
    std::vector<uint32_t> fill(anode_ptr.begin(), anode_ptr.end() - 1);
    for (size_t a = 0; a < n_arcs; ++a) { anode_items[fill[arc_s[a]]++] = (uint32_t)(2 * a); anode_items[fill[arc_n[a]]++] = (uint32_t)(2 * a + 1); }
  }
  auto up = [&](DevBuf<uint32_t>& b, const uint32_t* src, size_t n) -> hipError_t {
    const hipError_t e = b.alloc(std::max<size_t>(n, 1));
    return e != hipSuccess || !n ? e : hipMemcpyAsync(b.get(), src, n * 4, hipMemcpyHostToDevice, s);
  };
  ST_CK(F, up(wf->ctrl_idx, ci, nc));
  ST_CK(F, up(wf->node_ptr, node_ptr.data(), n_ctrl + 1));
  ST_CK(F, up(wf->node_items, node_items.data(), node_ptr[n_ctrl]));
  ST_CK(F, up(wf->arc_s, arc_s.data(), n_arcs));
  ST_CK(F, up(wf->arc_n, arc_n.data(), n_arcs));
  ST_CK(F, up(wf->anode_ptr, anode_ptr.data(), n_ctrl + 1));
  ST_CK(F, up(wf->anode_items, anode_items.data(), 2 * n_arcs));
  ST_CK(F, wf->ctrl_w.alloc(nc)); ST_CK(F, wf->total_w.alloc(n_src)); ST_CK(F, wf->arc_w.alloc(n_arcs));
  ST_CK(F, wf->rows.alloc(n_src * WF_ROW)); ST_CK(F, wf->u_pt.alloc(4 * n_src));
  ST_CK(F, wf->arc_d.alloc(6 * n_arcs)); ST_CK(F, wf->arc_b.alloc(6 * n_arcs)); ST_CK(F, wf->u_arc.alloc(6 * n_arcs));
  ST_CK(F, wf->vec.alloc(7 * 6 * n_ctrl + n_ctrl)); ST_CK(F, wf->node_dot.alloc(n_ctrl)); ST_CK(F, wf->sc.alloc(1));
  // weights
  DevPool pool;
  const float *d_cd2 = nullptr, *d_rd2 = nullptr;
  uint32_t* d_pos = nullptr;
  ST_CK(F, st_stage(pool, s, mem, ctrl.d2, nc, &d_cd2));
  ST_CK(F, st_stage(pool, s, mem, reg.d2, nr, &d_rd2));
  const auto coeff = [](const WfLists& l) { return l.kernel == 1 ? -0.5f / (l.sigma * l.sigma) : 0.0f; };
  hipLaunchKernelGGL(k_wf_ctrl_weights, dim3(wf_blocks(n_src)), dim3(WF_THREADS), 0, s, (uint32_t)n_src, (uint32_t)ctrl.k, (const uint32_t*)wf->ctrl_idx.get(), d_cd2,
                     ctrl.kernel == 1 ? (int)CW_RBF : (int)CW_UNITY, coeff(ctrl), wf->ctrl_w.get(), wf->total_w.get());
  ST_CK(F, hipGetLastError());
  if (n_arcs) {
    ST_CK(F, pool.get(&d_pos, n_arcs));
    ST_CK(F, hipMemcpyAsync(d_pos, arc_pos.data(), n_arcs * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_wf_arc_weights, dim3(wf_blocks(n_arcs)), dim3(WF_THREADS), 0, s, (uint32_t)n_arcs, (const uint32_t*)d_pos, d_rd2, reg.kernel == 1 ? (int)CW_RBF : (int)CW_UNITY,
                       coeff(reg), wf->arc_w.get());
    ST_CK(F, hipGetLastError());
  }
  ST_CK(F, hipStreamSynchronize(s));      // (the host vectors and the pool leave scope)
  *out = wf.release();
  return CILHIP_OK;
}

}  // namespace

}  // namespace cilhip

extern "C" void cilhip_warp_default_params(cilhip_warp_params* p) {
  if (!p) return;
  p->w_p2p = 0.0f; p->w_p2pl = 1.0f; p->w_reg = 1.0f; p->huber_boundary = 1e-4f;      // icp_warp_field_combined_metric_sparse.hpp:67-70
  p->max_gn_iter = 10; p->gn_conv_tol = 1e-5f; p->max_cg_iter = 1000; p->cg_conv_tol = 1e-5f;      // warp_field_estimation.hpp:1411-1415
}

extern "C" int cilhip_warp_field_create(int device, size_t n_src, size_t n_ctrl, const uint32_t* ctrl_idx, const float* ctrl_d2, size_t k_ctrl, int ctrl_kernel, float ctrl_sigma,
                                        const uint32_t* reg_idx, const float* reg_d2, size_t k_reg, int reg_kernel, float reg_sigma, int mem, cilhip_warp_field** out) {
  using namespace cilhip;
  constexpr const char* F = "warp_field_create";
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (!out) return refuse("out is null");
  if (!ctrl_idx || !ctrl_d2 || !reg_idx || !reg_d2) return refuse("a list array is null");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (n_ctrl == 0) return refuse("n_ctrl is 0");
  if (n_src == 0) return refuse("n_src is 0");
  if (k_ctrl < 1 || k_ctrl > 32 || k_reg < 1 || k_reg > 32) return refuse("k_ctrl and k_reg must be in 1 .. 32");
  if ((unsigned long long)n_src * k_ctrl >= WF_LIMIT || (unsigned long long)n_ctrl * k_reg >= WF_LIMIT / 16) return refuse("n_src * k_ctrl must be below 2^32 - 16 and n_ctrl * k_reg below 2^28 - 1");
  if ((ctrl_kernel != 0 && ctrl_kernel != 1) || (reg_kernel != 0 && reg_kernel != 1)) return st_fail(CILHIP_ERR_UNSUPPORTED, F, "a weight kernel other than 0 (Unity) and 1 (RBF)");
  if (!wf_finite(ctrl_sigma) || !wf_finite(reg_sigma)) return refuse("a sigma is not finite");
  if ((ctrl_kernel == 1 && ctrl_sigma == 0.0f) || (reg_kernel == 1 && reg_sigma == 0.0f)) return refuse("the sigma of an RBF kernel is 0");
  if (mem == CILHIP_MEM_HOST) {
    const char* bad = wf_check_indices(ctrl_idx, n_src * k_ctrl, n_ctrl);
    if (!bad) bad = wf_check_indices(reg_idx, n_ctrl * k_reg, n_ctrl);
    if (bad) return refuse(bad);
  }
  st_clear();
  try {
    return wf_create(device, n_src, n_ctrl, WfLists{ctrl_idx, ctrl_d2, k_ctrl, ctrl_kernel, ctrl_sigma}, WfLists{reg_idx, reg_d2, k_reg, reg_kernel, reg_sigma}, mem, out);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

extern "C" void cilhip_warp_field_destroy(cilhip_warp_field* wf) {
  if (!wf) return;
  (void)hipSetDevice(wf->device);
  delete wf;
}

namespace cilhip {
namespace {

int wf_estimate_entry(const char* F, WfKind kind, cilhip_warp_field* wf, const float* dst_xyz, const float* dst_normals, size_t n_dst, const float* src_xyz, const uint32_t* nn_idx,
                      int mem, const cilhip_warp_params* params, float* ctrl_transforms_out, cilhip_warp_stats* stats_or_null) {
  auto refuse = [F](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (!wf) return refuse("the warp field is null");
  if (!src_xyz || !nn_idx || !ctrl_transforms_out) return refuse("src_xyz, nn_idx or ctrl_transforms_out is null");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (const char* why = wf_params_refusal(params)) return refuse(why);
  if ((unsigned long long)n_dst >= WF_LIMIT) return refuse("n_dst must be below 2^32 - 16");
  if (n_dst > 0 && !dst_xyz) return refuse("dst_xyz is null with n_dst > 0");
  if (n_dst > 0 && params->w_p2pl > 0.0f && !dst_normals) return refuse("dst_normals is null with w_p2pl > 0");
  st_clear();
  ST_CK(F, hipSetDevice(wf->device));
  hipStream_t s = wf->st.s;
  try {
    DevPool pool;
    const float *d_dst = nullptr, *d_nrm = nullptr, *d_src = nullptr, *d_nn = nullptr;
    if (n_dst) ST_CK(F, st_stage(pool, s, mem, dst_xyz, 3 * n_dst, &d_dst));
    if (n_dst && dst_normals) ST_CK(F, st_stage(pool, s, mem, dst_normals, 3 * n_dst, &d_nrm));
    ST_CK(F, st_stage(pool, s, mem, src_xyz, 3 * wf->n_src, &d_src));
    ST_CK(F, st_stage(pool, s, mem, reinterpret_cast<const float*>(nn_idx), wf->n_src, &d_nn));
    float* d_T = ctrl_transforms_out;
    if (mem == CILHIP_MEM_HOST) ST_CK(F, pool.get(&d_T, 16 * wf->n_ctrl));
    cilhip_warp_stats st{};
    if (const int rc = wf_estimate_dev(F, wf, d_dst, d_nrm, n_dst, d_src, reinterpret_cast<const uint32_t*>(d_nn), *params, d_T, &st, kind)) return rc;
    if (mem == CILHIP_MEM_HOST) {
      ST_CK(F, hipMemcpyAsync(ctrl_transforms_out, d_T, 16 * wf->n_ctrl * sizeof(float), hipMemcpyDeviceToHost, s));
      ST_CK(F, hipStreamSynchronize(s));
    }
    if (stats_or_null) *stats_or_null = st;
    return CILHIP_OK;
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

int wf_resample_entry(const char* F, WfKind kind, cilhip_warp_field* wf, const float* ctrl_T, float* dense_T_out, int mem) {
  auto refuse = [F](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (!wf) return refuse("the warp field is null");
  if (!ctrl_T || !dense_T_out) return refuse("ctrl_T or dense_T_out is null");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  st_clear();
  ST_CK(F, hipSetDevice(wf->device));
  hipStream_t s = wf->st.s;
  try {
    DevPool pool;
    const float* d_in = nullptr;
    ST_CK(F, st_stage(pool, s, mem, ctrl_T, 16 * wf->n_ctrl, &d_in));
    float* d_out = dense_T_out;
    if (mem == CILHIP_MEM_HOST) ST_CK(F, pool.get(&d_out, 16 * wf->n_src));
    if (const int rc = wf_resample_dev(F, wf, d_in, d_out, kind)) return rc;
    if (mem == CILHIP_MEM_HOST) ST_CK(F, hipMemcpyAsync(dense_T_out, d_out, 16 * wf->n_src * sizeof(float), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    return CILHIP_OK;
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

}  // namespace
}  // namespace cilhip

extern "C" int cilhip_warp_field_estimate3f(cilhip_warp_field* wf, const float* dst_xyz, const float* dst_normals, size_t n_dst, const float* src_xyz, const uint32_t* nn_idx,
                                            int mem, const cilhip_warp_params* params, float* ctrl_transforms_out, cilhip_warp_stats* stats_or_null) {
  return cilhip::wf_estimate_entry("warp_field_estimate", cilhip::WF_RIGID, wf, dst_xyz, dst_normals, n_dst, src_xyz, nn_idx, mem, params, ctrl_transforms_out, stats_or_null);
}
extern "C" int cilhip_warp_field_estimate_affine3f(cilhip_warp_field* wf, const float* dst_xyz, const float* dst_normals, size_t n_dst, const float* src_xyz, const uint32_t* nn_idx,
                                                   int mem, const cilhip_warp_params* params, float* ctrl_transforms_out, cilhip_warp_stats* stats_or_null) {
  return cilhip::wf_estimate_entry("warp_field_estimate_affine", cilhip::WF_AFFINE, wf, dst_xyz, dst_normals, n_dst, src_xyz, nn_idx, mem, params, ctrl_transforms_out, stats_or_null);
}
extern "C" int cilhip_warp_field_resample3f(cilhip_warp_field* wf, const float* ctrl_T, float* dense_T_out, int mem) {
  return cilhip::wf_resample_entry("warp_field_resample", cilhip::WF_RIGID, wf, ctrl_T, dense_T_out, mem);
}
extern "C" int cilhip_warp_field_resample_affine3f(cilhip_warp_field* wf, const float* ctrl_T, float* dense_T_out, int mem) {
  return cilhip::wf_resample_entry("warp_field_resample_affine", cilhip::WF_AFFINE, wf, ctrl_T, dense_T_out, mem);
}

extern "C" int cilhip_transform_points_per_point3f(int device, const float* T, const float* xyz, size_t n, int mem, float* out) {
  using namespace cilhip;
  constexpr const char* F = "transform_points_per_point";
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if ((unsigned long long)n >= WF_LIMIT / 16) return refuse("n must be below 2^28 - 1");
  if (n > 0 && (!T || !xyz || !out)) return refuse("T, xyz or out is null with n > 0");
  st_clear();
  if (n == 0) return CILHIP_OK;
  if (const int open = st_open(F, device)) return open;
  try {
    DevPool pool;
    StreamGuard st;
    ST_CK(F, st.create());
    const float *d_T = nullptr, *d_xyz = nullptr;
    ST_CK(F, st_stage(pool, st.s, mem, T, 16 * n, &d_T));
    ST_CK(F, st_stage(pool, st.s, mem, xyz, 3 * n, &d_xyz));
    float* d_out = out;
    if (mem == CILHIP_MEM_HOST) ST_CK(F, pool.get(&d_out, 3 * n));
    if (const int rc = wf_transform_points_dev(F, st.s, d_T, d_xyz, n, d_out)) return rc;
    if (mem == CILHIP_MEM_HOST) ST_CK(F, hipMemcpyAsync(out, d_out, 3 * n * sizeof(float), hipMemcpyDeviceToHost, st.s));
    ST_CK(F, hipStreamSynchronize(st.s));
    return CILHIP_OK;
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

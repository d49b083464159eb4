// mds.hip -- MultidimensionalScaling<float> on the device (the rules M1-M5 are stated in c_api.h):
//   M1  the squared distances, f32, read where they lie; never squared into a second matrix       k_mds_stream (the square is fused)
//   M2  B = -1/2 J Dhat J as an operator that is never formed                                       k_mds_stream (the hot path: one pass over
//       the n x n matrix per block product), k_mds_moments_stage1 / k_stage2, k_mds_combine; the column means once: k_mds_means
//   M4  locked, Chebyshev-filtered subspace iteration for the pairs of largest magnitude, f64       subspace_device.hpp (shared with
//       spectral.hip): Gram and residual sums, CholQR2, the recurrence; small dense work: small_sym.hpp; scalar decisions: mds_host.hpp
//   M5  order, clamping, signs, scaling, rounding                                                   k_sign_stage1 / 2, k_mds_epilogue
// Every sum runs in an order n and the block width alone decide and there is no atomic: two runs agree bit for bit.
#include "../../include/cilantro_hip/c_api.h"
#include "mds_host.hpp"
#include "small_sym.hpp"
#include "stateless.hpp"
#include "subspace_device.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int MDS_TILE = 64;          // rows of the block staged in LDS at a time
constexpr int MDS_MAX_NEV = 17;

// the rows j of the matrix are cut into chunks of max(128, ceil(n / 64)) consecutive rows: at most 64 chunks, a shape n alone decides
struct MdsChunks { uint32_t rows; int count; };
inline MdsChunks mds_chunks(size_t n) {
  const size_t rows = std::max<size_t>(128, (n + 63) / 64);
  return MdsChunks{(uint32_t)rows, (int)((n + rows - 1) / rows)};
}

// The hot path.  partial[chunk][i][c] = sum over the chunk's rows j, ascending, of Dhat[j][i] * X[j][c0 + c] for c < w: the transposed
// matrix is applied (M1: symmetry is the caller's promise), so a wave reads VEC * 64 consecutive floats of row j in one load and nothing
// crosses lanes.  Lane t of block (tile, chunk) owns the VEC columns i = (tile * 256 + t) * VEC ...; X[j][:] is the same for every lane and
// comes from LDS, MDS_TILE rows at a time, padded with zeros to CB columns (CB: the compile-time width, w <= CB).  Dhat = D, or d * d as
// one f32 product.  VEC = 4 (2) wants n % 4 (2) == 0 and a 16 (8)-byte aligned matrix; the sums do not depend on VEC or CB.
template <int CB, int VEC>
__global__ __launch_bounds__(SP_THREADS) void k_mds_stream(const float* __restrict__ D, uint32_t n, int is_squared, const double* __restrict__ X, int ldx, int c0, int w,
                                                           uint32_t rows_per_chunk, double* __restrict__ partial) {
  __shared__ double xs[MDS_TILE * CB];
  const int t = threadIdx.x;
  const uint64_t i0 = ((uint64_t)blockIdx.x * SP_THREADS + t) * VEC;
  const bool on = i0 < n;      // (n is a multiple of VEC, so i0 + VEC - 1 < n as well)
  const uint64_t j0 = std::min<uint64_t>((uint64_t)blockIdx.y * rows_per_chunk, n), j1 = std::min<uint64_t>(j0 + rows_per_chunk, n);
  double acc[VEC][CB];
#pragma unroll
  for (int v = 0; v < VEC; ++v)
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[v][c] = 0.0;
  for (uint64_t base = j0; base < j1; base += MDS_TILE) {
    const int cnt = (int)std::min<uint64_t>(MDS_TILE, j1 - base);
    for (int u = t; u < cnt * CB; u += SP_THREADS) {
      const int rr = u / CB, c = u - rr * CB;
      xs[u] = c < w ? X[(base + rr) * ldx + c0 + c] : 0.0;
    }
    __syncthreads();
    if (on) {
      const float* row = D + base * n + i0;
#pragma unroll 4
      for (int rr = 0; rr < cnt; ++rr) {
        float d[VEC];
        if (VEC == 4) {
          const float4 q = *reinterpret_cast<const float4*>(row + (size_t)rr * n);
          d[0] = q.x; d[1 % VEC] = q.y; d[2 % VEC] = q.z; d[3 % VEC] = q.w;
        } else if (VEC == 2) {
          const float2 q = *reinterpret_cast<const float2*>(row + (size_t)rr * n);
          d[0] = q.x; d[1 % VEC] = q.y;
        } else {
          d[0] = row[(size_t)rr * n];
        }
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
          const double dv = (double)(is_squared ? d[v] : __fmul_rn(d[v], d[v]));
#pragma unroll
          for (int c = 0; c < CB; ++c) acc[v][c] = fma(dv, xs[rr * CB + c], acc[v][c]);
        }
      }
    }
    __syncthreads();
  }
  if (on) {
#pragma unroll
    for (int v = 0; v < VEC; ++v)
#pragma unroll
      for (int c = 0; c < CB; ++c)
        if (c < w) partial[((size_t)blockIdx.y * n + i0 + v) * w + c] = acc[v][c];
  }
}

// r[i] = (partial[0][i] + partial[1][i] + ...) / n in ascending chunk order: the mean of column i of Dhat (width-1 partial sums against ones)
__global__ __launch_bounds__(SP_THREADS) void k_mds_means(const double* __restrict__ partial, int chunks, uint32_t n, double* __restrict__ r) {
  for (uint64_t i = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_THREADS) {
    double a = 0.0;
    for (int k = 0; k < chunks; ++k) a += partial[(size_t)k * n + i];
    r[i] = a / (double)n;
  }
}

// stage 1 of the two moments the centring needs of the columns [c0, c0 + w) of X: s_c = sum_j X[j][c] and q_c = sum_j r[j] X[j][c].  Lane
// (rl, c) sums the rows rl, rl + rpb, ... of the block's range, the rpb sums of a column are added in ascending rl; partial[B][2 w]
__global__ __launch_bounds__(SP_THREADS) void k_mds_moments_stage1(const double* __restrict__ X, int ldx, int c0, int w, const double* __restrict__ r, uint32_t n,
                                                                   uint32_t rows_per_block, double* __restrict__ partial) {
  __shared__ double ps[SP_THREADS], pq[SP_THREADS];
  const int t = threadIdx.x, rpb = SP_THREADS / w, rl = t / w, c = t - rl * w;
  const uint64_t r0 = std::min<uint64_t>((uint64_t)blockIdx.x * rows_per_block, n), r1 = std::min<uint64_t>(r0 + rows_per_block, n);
  double s = 0.0, q = 0.0;
  if (rl < rpb)
    for (uint64_t row = r0 + rl; row < r1; row += rpb) {
      const double x = X[row * ldx + c0 + c];
      s += x;
      q = fma(r[row], x, q);
    }
  ps[t] = s; pq[t] = q;
  __syncthreads();
  if (t < w) {
    double a = 0.0, bq = 0.0;
    for (int u = 0; u < rpb; ++u) { a += ps[u * w + t]; bq += pq[u * w + t]; }
    partial[(size_t)blockIdx.x * 2 * w + t] = a;
    partial[(size_t)blockIdx.x * 2 * w + w + t] = bq;
  }
}

// Y = alpha (B X - shift X) + beta Z on the columns [c0, c0 + w) of row-major [n][ld] blocks -- k_block_product's step of the recurrence --
// with (B X)[i][c] = -1/2 (((sum over the chunks, ascending, of partial[chunk][i][c]) - r[i] s_c - q_c) + g s_c), mom = {s[w], q[w]}.  The
// columns before c0 (locked) are copied from X when copy_leading is set and left alone otherwise.  Y must not be X; Z may be null.
__global__ __launch_bounds__(SP_THREADS) void k_mds_combine(const double* __restrict__ partial, int chunks, uint32_t n, int ld, int c0, int w, const double* __restrict__ r, double g,
                                                            const double* __restrict__ mom, const double* __restrict__ X, const double* __restrict__ Z, double* __restrict__ Y,
                                                            double alpha, double shift, double beta, int copy_leading) {
  const uint64_t total = (uint64_t)n * ld;
  for (uint64_t o = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; o < total; o += (uint64_t)gridDim.x * SP_THREADS) {
    const uint64_t row = o / ld;
    const int col = (int)(o - row * ld), c = col - c0;
    if (c < 0) { if (copy_leading) Y[o] = X[o]; continue; }
    if (c >= w) continue;
    double a = 0.0;
    for (int k = 0; k < chunks; ++k) a += partial[((size_t)k * n + row) * w + c];
    const double s = mom[c], q = mom[w + c], x = X[o];
    const double bx = -0.5 * (((a - r[row] * s) - q) + g * s);
    double y = alpha * (bx - shift * x);
    if (Z != nullptr) y = fma(beta, Z[o], y);
    Y[o] = y;
  }
}

__global__ __launch_bounds__(SP_THREADS) void k_mds_fill(double* __restrict__ x, uint64_t total, double v) {
  for (uint64_t o = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; o < total; o += (uint64_t)gridDim.x * SP_THREADS) x[o] = v;
}

// M5: out[r][c] = sqrtf(ev[c]) * (float)(sign * x) for the dim columns col[c] of the block
struct MdsOut { int col[MDS_MAX_NEV]; float root[MDS_MAX_NEV]; };
__global__ __launch_bounds__(SP_THREADS) void k_mds_epilogue(const double* __restrict__ X, const double* __restrict__ sign, uint32_t n, int b, int dim, MdsOut o, float* __restrict__ out) {
  const uint64_t total = (uint64_t)n * dim;
  for (uint64_t e = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; e < total; e += (uint64_t)gridDim.x * SP_THREADS) {
    const uint64_t r = e / dim;
    const int c = (int)(e - r * dim), k = o.col[c];
    out[e] = __fmul_rn(o.root[c], (float)(sign[k] * X[r * b + k]));
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// the operator: the matrix, its column means and what one product needs
struct MdsOp : SubspaceOps {
  const float* D = nullptr;
  int is_squared = 1;
  MdsChunks ch{};
  double* r = nullptr;             // [n] column means of Dhat
  double g = 0.0;                  // their mean
  double* stream_partial = nullptr;      // [ch.count][n][SP_MAX_B]
  double* mom_partial = nullptr;   // [SP_PARTIAL_BLOCKS][2 SP_MAX_B]
  double* mom = nullptr;           // [2 SP_MAX_B]
  size_t products = 0;

  // the load width: 16 bytes per lane up to 16 columns, 8 bytes above (4 x 24 or 4 x 32 f64 accumulators per lane leave no register for
  // anything else: measured at n = 32768, 25 columns, 5.03 ms with 16-byte loads), 4 bytes where n or the address does not allow more
  void stream(const double* X, int ld, int c0, int w) {
    const uintptr_t addr = reinterpret_cast<uintptr_t>(D);
    const int vec = w <= 16 ? ((n % 4 == 0 && addr % 16 == 0) ? 4 : 1) : ((n % 2 == 0 && addr % 8 == 0) ? 2 : 1);
    const dim3 grid((unsigned)((n + (size_t)SP_THREADS * vec - 1) / ((size_t)SP_THREADS * vec)), (unsigned)ch.count);
#define MDS_STREAM(CB, VEC) hipLaunchKernelGGL((k_mds_stream<CB, VEC>), grid, dim3(SP_THREADS), 0, s, D, (uint32_t)n, is_squared, X, ld, c0, w, ch.rows, stream_partial)
#define MDS_NARROW(CB) do { if (vec == 4) MDS_STREAM(CB, 4); else MDS_STREAM(CB, 1); } while (0)
#define MDS_WIDE(CB) do { if (vec == 2) MDS_STREAM(CB, 2); else MDS_STREAM(CB, 1); } while (0)
    if (w <= 1) MDS_NARROW(1);
    else if (w <= 4) MDS_NARROW(4);
    else if (w <= 8) MDS_NARROW(8);
    else if (w <= 12) MDS_NARROW(12);
    else if (w <= 16) MDS_NARROW(16);
    else if (w <= 24) MDS_WIDE(24);
    else MDS_WIDE(32);
#undef MDS_WIDE
#undef MDS_NARROW
#undef MDS_STREAM
  }
  int open(cilhip::DevPool& pool, const float* d_D, size_t n_, int squared_) {
    D = d_D; n = n_; is_squared = squared_; ts = two_stage(n_); ch = mds_chunks(n_);
    ST_CK(F, pool.get(&r, n)); ST_CK(F, pool.get(&stream_partial, (size_t)ch.count * n * SP_MAX_B));
    ST_CK(F, pool.get(&mom_partial, (size_t)SP_PARTIAL_BLOCKS * 2 * SP_MAX_B)); ST_CK(F, pool.get(&mom, 2 * SP_MAX_B));
    // M2: the column means, by the stream kernel against a column of ones; M1: a non-finite entry makes its column's mean non-finite
    double* ones = nullptr;
    ST_CK(F, pool.get(&ones, n));
    hipLaunchKernelGGL(k_mds_fill, dim3(sp_grid(n)), dim3(SP_THREADS), 0, s, ones, (uint64_t)n, 1.0);
    stream(ones, 1, 0, 1);
    hipLaunchKernelGGL(k_mds_means, dim3(sp_grid(n)), dim3(SP_THREADS), 0, s, (const double*)stream_partial, ch.count, (uint32_t)n, r);
    ST_CK(F, hipGetLastError());
    std::vector<double> hr(n);
    ST_CK(F, hipMemcpyAsync(hr.data(), r, n * sizeof(double), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    double sum = 0.0;
    for (size_t i = 0; i < n; ++i) {      // ascending
      if (!std::isfinite(hr[i])) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "M1: an entry of the (squared) distance matrix is not finite");
      sum += hr[i];
    }
    g = sum / (double)n;
    return CILHIP_OK;
  }
  // Y = alpha (B X - shift X) + beta Z on the columns [c0, ld) of [n][ld] blocks
  int product(const double* X, const double* Z, double* Y, int ld, int c0, double alpha, double shift, double beta, int copy_leading) {
    const int w = ld - c0;
    hipLaunchKernelGGL(k_mds_moments_stage1, dim3(ts.blocks), dim3(SP_THREADS), 0, s, X, ld, c0, w, (const double*)r, (uint32_t)n, ts.rows_per_block, mom_partial);
    hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)mom_partial, ts.blocks, 2 * w, mom);
    stream(X, ld, c0, w);
    hipLaunchKernelGGL(k_mds_combine, dim3(sp_grid(n * ld, 2048)), dim3(SP_THREADS), 0, s, (const double*)stream_partial, ch.count, (uint32_t)n, ld, c0, w, (const double*)r, g,
                       (const double*)mom, X, Z, Y, alpha, shift, beta, copy_leading);
    ST_CK(F, hipGetLastError());
    ++products;
    return CILHIP_OK;
  }
};

int embedding_impl(const float* D, size_t n, int mem, const cilhip_mds_params& prm, const cilhip::MdsSizes& z, float* embedded_out, float* eigenvalues_out,
                   cilhip_mds_result* result) {
  const char* F = "mds_embedding";
  const auto t0 = std::chrono::steady_clock::now();
  const int nev = (int)z.nev;
  const int b = (int)std::min<size_t>(z.nev + std::max<size_t>((size_t)prm.guard, z.nev / 2), n);
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  const float* d_D = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, mem, D, n * n, &d_D));
  MdsOp so;
  so.F = F; so.s = s; so.b = b;
  ST_CK(F, pool.get(&so.small, 1088)); ST_CK(F, pool.get(&so.out, 1024)); ST_CK(F, pool.get(&so.partial, (size_t)SP_PARTIAL_BLOCKS * 1024));
  if (const int rc = so.open(pool, d_D, n, prm.distances_are_squared ? 1 : 0)) return rc;
  SignRec* sign_partial = nullptr;
  ST_CK(F, pool.get(&sign_partial, (size_t)SP_PARTIAL_BLOCKS * SP_MAX_B));
  double* P[4];
  for (int i = 0; i < 4; ++i) ST_CK(F, pool.get(&P[i], n * (size_t)b));
  double *X = P[0], *AX = P[1], *T1 = P[2], *T2 = P[3];
  hipLaunchKernelGGL(k_start_block, dim3(sp_grid(n * b, 2048)), dim3(SP_THREADS), 0, s, X, (uint64_t)n * b, b);
  ST_CK(F, hipGetLastError());
  ST_CK(F, hipMemsetAsync(AX, 0, n * (size_t)b * sizeof(double), s));
  if (const int rc = so.orthonormalise(&X, &T1)) return rc;

  double G[SP_MAX_B * SP_MAX_B], Ga[SP_MAX_B * SP_MAX_B], Sa[SP_MAX_B * SP_MAX_B], S[SP_MAX_B * SP_MAX_B], theta[SP_MAX_B], wa[SP_MAX_B], res2[SP_MAX_B];
  int order[SP_MAX_B];
  for (int i = 0; i < b; ++i) theta[i] = 0.0;
  size_t outer = 0;
  int locked = 0;
  double max_res = 0.0;
  for (;;) {
    ++outer;
    // Rayleigh-Ritz on the unlocked columns; the Ritz pairs by descending magnitude
    const int m = b - locked;
    if (const int rc = so.product(X, nullptr, AX, b, locked, 1.0, 0.0, 0.0, 0)) return rc;
    if (const int rc = so.gram(X, AX, G)) return rc;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) Ga[i * m + j] = 0.5 * (G[(locked + i) * b + locked + j] + G[(locked + j) * b + locked + i]);
    cilhip::sym_jacobi(Ga, m, wa, Sa);
    cilhip::magnitude_order(wa, m, order);
    for (int i = 0; i < b; ++i)
      for (int j = 0; j < b; ++j) S[i * b + j] = (i >= locked && j >= locked) ? Sa[(i - locked) * m + order[j - locked]] : (i == j ? 1.0 : 0.0);
    for (int j = 0; j < m; ++j) theta[locked + j] = wa[order[j]];
    if (const int rc = so.mul(X, S, T1)) return rc;
    if (const int rc = so.mul(AX, S, T2)) return rc;
    std::swap(X, T1); std::swap(AX, T2);
    // the true residuals; leading pairs that pass M4 are locked
    ST_CK(F, hipMemcpyAsync(so.small + 1024, theta, b * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_residual_stage1, dim3(so.ts.blocks), dim3(SP_THREADS), 0, s, (const double*)X, (const double*)AX, (const double*)(so.small + 1024), (uint32_t)n, b,
                       so.ts.rows_per_block, so.partial);
    hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)so.partial, so.ts.blocks, b, so.out);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(res2, so.out, b * sizeof(double), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    while (locked < nev && cilhip::mds_accepts(std::sqrt(res2[locked]), theta[locked])) ++locked;
    max_res = 0.0;
    for (int i = 0; i < nev; ++i) max_res = std::max(max_res, std::sqrt(res2[i]));
    if (locked == nev || outer >= prm.max_outer) break;
    // the filter on the unlocked columns: damp [-e, e], 1 at the first unlocked magnitude
    const double a0 = std::fabs(theta[locked]);
    if (a0 > 0.0 && std::isfinite(a0)) {
      const cilhip::MdsFilterPlan plan = cilhip::mds_filter_plan(a0, std::fabs(theta[b - 1]), std::fabs(theta[nev - 1]), locked > 0 ? std::fabs(theta[0]) : 0.0, prm.degree);
      auto product = [&](const double* Xi, const double* Zi, double* Yo, double alpha, double cc, double beta) { return so.product(Xi, Zi, Yo, b, locked, alpha, cc, beta, 1); };
      if (const int rc = cheb_filter(product, plan.e, 0.0, a0, plan.degree, X, T1, T2)) return rc;
    }
    // twice: the unlocked columns minus their components along the locked ones
    for (int pass = 0; pass < 2 && locked > 0; ++pass) {
      if (const int rc = so.gram(X, X, G)) return rc;
      for (int i = 0; i < b; ++i)
        for (int j = 0; j < b; ++j) S[i * b + j] = (i < locked && j >= locked) ? -G[i * b + j] : (i == j ? 1.0 : 0.0);
      if (const int rc = so.mul(X, S, T1)) return rc;
      std::swap(X, T1);
    }
    if (const int rc = so.orthonormalise(&X, &T1, locked)) return rc;
  }

  // M5
  cilhip::magnitude_order(theta, nev, order);
  std::vector<float> ev(nev);
  for (int i = 0; i < nev; ++i) { ev[i] = (float)theta[order[i]]; if (ev[i] < 0.0f) ev[i] = 0.0f; }
  size_t dim = z.dim;
  if (z.estimate) dim = cilhip::mds_embedding_dim(ev.data(), (size_t)nev, z.dim);
  if (dim > (size_t)nev) dim = (size_t)nev;
  MdsOut mo{};
  for (size_t c = 0; c < dim; ++c) { mo.col[c] = order[c]; mo.root[c] = sqrtf(ev[c]); }
  hipLaunchKernelGGL(k_sign_stage1, dim3(so.ts.blocks), dim3(SP_THREADS), 0, s, (const double*)X, (uint32_t)n, b, so.ts.rows_per_block, sign_partial);
  hipLaunchKernelGGL(k_sign_stage2, dim3(1), dim3(64), 0, s, (const SignRec*)sign_partial, so.ts.blocks, b, so.small + 1056);
  float* d_out = embedded_out;
  if (mem != CILHIP_MEM_DEVICE) ST_CK(F, pool.get(&d_out, n * dim));
  hipLaunchKernelGGL(k_mds_epilogue, dim3(sp_grid(n * dim, 2048)), dim3(SP_THREADS), 0, s, (const double*)X, (const double*)(so.small + 1056), (uint32_t)n, b, (int)dim, mo, d_out);
  ST_CK(F, hipGetLastError());
  if (mem != CILHIP_MEM_DEVICE) ST_CK(F, hipMemcpyAsync(embedded_out, d_out, n * dim * sizeof(float), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  std::memcpy(eigenvalues_out, ev.data(), nev * sizeof(float));
  result->dim = dim; result->num_eigenvalues = (size_t)nev; result->n_converged = (size_t)locked; result->outer_iterations = outer; result->block_products = so.products;
  result->locked = (size_t)locked; result->max_residual = max_res;
  result->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return CILHIP_OK;
}

int apply_impl(const float* D, size_t n, int mem, int is_squared, const double* x, int b, double* y_out, double* product_ms) {
  const char* F = "mds_apply";
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  cilhip::EventGuard e0, e1;
  ST_CK(F, s.create()); ST_CK(F, e0.create()); ST_CK(F, e1.create());
  const float* d_D = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, mem, D, n * n, &d_D));
  MdsOp so;
  so.F = F; so.s = s; so.b = b;
  if (const int rc = so.open(pool, d_D, n, is_squared)) return rc;
  const double* d_x = x;
  double* d_y = y_out;
  if (mem != CILHIP_MEM_DEVICE) {
    double* up = nullptr;
    ST_CK(F, pool.get(&up, n * (size_t)b)); ST_CK(F, pool.get(&d_y, n * (size_t)b));
    ST_CK(F, hipMemcpyAsync(up, x, n * (size_t)b * sizeof(double), hipMemcpyHostToDevice, s));
    d_x = up;
  }
  ST_CK(F, hipEventRecord(e0, s));
  if (const int rc = so.product(d_x, nullptr, d_y, b, 0, 1.0, 0.0, 0.0, 0)) return rc;
  ST_CK(F, hipEventRecord(e1, s));
  if (mem != CILHIP_MEM_DEVICE) ST_CK(F, hipMemcpyAsync(y_out, d_y, n * (size_t)b * sizeof(double), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  float ms = 0.0f;
  ST_CK(F, hipEventElapsedTime(&ms, e0, e1));
  if (product_ms) *product_ms = (double)ms;
  return CILHIP_OK;
}

}  // namespace

extern "C" {

void cilhip_mds_default_params(cilhip_mds_params* p) {
  if (!p) return;
  p->max_dim = 2; p->estimate_dim = 0; p->distances_are_squared = 1; p->max_outer = 1000; p->degree = 24; p->guard = 3;
}

int cilhip_mds_embedding(int device, const float* D, size_t n, int mem, const cilhip_mds_params* params, float* embedded_out, float* eigenvalues_out, cilhip_mds_result* result) {
  const char* F = "mds_embedding";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!D || !params || !embedded_out || !eigenvalues_out || !result) return refuse("M1: D, params, embedded_out, eigenvalues_out or result is NULL");
  if (n < 3 || n >= SP_MAX_N) return refuse("M1: n must lie in [3, 2^32 - 16)");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("M1: mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (params->degree < 1 || params->degree > 512) return refuse("degree must lie in [1, 512]");
  if (params->guard < 1 || params->guard > 15) return refuse("guard must lie in [1, 15]");
  if (params->max_outer == 0) return refuse("max_outer must be positive");
  const cilhip::MdsSizes z = cilhip::mds_sizes(n, params->max_dim, params->estimate_dim != 0);
  if (z.dim > 16) return cilhip::st_fail(CILHIP_ERR_UNSUPPORTED, F, "M3: max_dim is above 16");
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device)) return open;
  return sp_guard(F, [&]() -> int { return embedding_impl(D, n, mem, *params, z, embedded_out, eigenvalues_out, result); });
}

int cilhip_mds_apply(int device, const float* D, size_t n, int mem, int distances_are_squared, const double* x, size_t b, double* y_out, double* product_ms_out) {
  const char* F = "mds_apply";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!D || !x || !y_out) return refuse("D, x or y_out is NULL");
  if (n < 3 || n >= SP_MAX_N) return refuse("M1: n must lie in [3, 2^32 - 16)");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("M1: mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (b == 0 || b > (size_t)SP_MAX_B) return refuse("b must lie in [1, 32]");
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device)) return open;
  return sp_guard(F, [&]() -> int { return apply_impl(D, n, mem, distances_are_squared ? 1 : 0, x, (int)b, y_out, product_ms_out); });
}

}  // extern "C"

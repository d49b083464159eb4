// subspace_device.hpp -- what a matrix-free f64 subspace iteration needs besides its operator (DESIGN.md sections 18 and 19): shared by
// spectral.hip (the sparse Laplacian, smallest pairs) and mds.hip (the dense centred distance matrix, largest magnitudes).
//   k_gram_stage1 / k_stage2   b x b products X^T Y: fixed-shape two-stage sums          k_block_mul          X S, Y R^-1
//   k_residual_stage1          squared residual norms                                     k_sign_stage1 / 2    the sign rule
//   k_start_block              the start block (a counter-based hash)                     two_stage            shape of a two-stage sum
//   SubspaceOps                gram, mul, orthonormalise (CholQR2) over one stream        cheb_filter          the three-term recurrence
// Every sum runs in an order n and b alone decide; there is no atomic.  Included by .hip files only; everything has internal linkage.
#pragma once

#include "../../include/cilantro_hip/c_api.h"
#include "small_sym.hpp"
#include "stateless.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>

namespace {

constexpr int SP_THREADS = 256;
constexpr uint32_t SP_NONE = 0xFFFFFFFFu;
constexpr int SP_MAX_B = 32;                 // columns of the block: nev <= 17, guard <= 15
constexpr int SP_PARTIAL_BLOCKS = 256;       // stage-1 blocks of every two-stage sum
constexpr size_t SP_MAX_N = 0xFFFFFFF0ull;

// one lane per row or element, grid-stride: at most one block per CU
inline unsigned sp_grid(size_t work, unsigned cap = 256) { return (unsigned)std::min<size_t>(std::max<size_t>((work + SP_THREADS - 1) / SP_THREADS, 1), cap); }

// ---- the b x b products, the block updates, the residuals ---------------------------------------------------------------------------
// stage 1 of C = X^T Y: block B owns the rows [B rows_per_block, (B + 1) rows_per_block) and sums them in ascending order, 32 rows at a
// time through LDS; partial[B][b * b].  The shape depends on n and b alone.
constexpr int GR_TILE = 32;
__global__ __launch_bounds__(SP_THREADS) void k_gram_stage1(const double* __restrict__ X, const double* __restrict__ Y, uint32_t n, int b, uint32_t rows_per_block,
                                                            double* __restrict__ partial) {
  __shared__ double sx[GR_TILE * SP_MAX_B], sy[GR_TILE * SP_MAX_B];
  const int t = threadIdx.x, bb = b * b;
  const uint64_t r0 = std::min<uint64_t>((uint64_t)blockIdx.x * rows_per_block, n), r1 = std::min<uint64_t>(r0 + rows_per_block, n);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (uint64_t base = r0; base < r1; base += GR_TILE) {
    const int cnt = (int)std::min<uint64_t>(GR_TILE, r1 - base);
    for (int u = t; u < cnt * b; u += SP_THREADS) { sx[u] = X[base * b + u]; sy[u] = Y[base * b + u]; }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t + SP_THREADS * q;
      if (e < bb) {
        const int i = e / b, j = e - i * b;
        double a = acc[q];
        for (int rr = 0; rr < cnt; ++rr) a = fma(sx[rr * b + i], sy[rr * b + j], a);
        acc[q] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int e = t + SP_THREADS * q;
    if (e < bb) partial[(size_t)blockIdx.x * bb + e] = acc[q];
  }
}

// stage 2 of every two-stage sum: out[e] = partial[0][e] + partial[1][e] + ... in ascending block order
__global__ __launch_bounds__(SP_THREADS) void k_stage2(const double* __restrict__ partial, int blocks, int width, double* __restrict__ out) {
  for (int e = threadIdx.x; e < width; e += SP_THREADS) {
    double a = 0.0;
    for (int B = 0; B < blocks; ++B) a += partial[(size_t)B * width + e];
    out[e] = a;
  }
}

// Out = X S (S: b x b, row-major); Out must not be X
__global__ __launch_bounds__(SP_THREADS) void k_block_mul(const double* __restrict__ X, const double* __restrict__ S, double* __restrict__ Out, uint64_t total, int b) {
  __shared__ double sS[SP_MAX_B * SP_MAX_B];
  for (int u = threadIdx.x; u < b * b; u += SP_THREADS) sS[u] = S[u];
  __syncthreads();
  for (uint64_t o = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; o < total; o += (uint64_t)gridDim.x * SP_THREADS) {
    const uint64_t r = o / b;
    const int c = (int)(o - r * b);
    double a = 0.0;
    for (int k = 0; k < b; ++k) a = fma(X[r * b + k], sS[k * b + c], a);
    Out[o] = a;
  }
}

// stage 1 of the squared residual norms ||AX_c - theta_c X_c||^2: lane (rl, c) sums the rows rl, rl + rpb, ... of the block's range for
// column c, the rpb sums of a column are added in ascending rl; partial[B][b]
__global__ __launch_bounds__(SP_THREADS) void k_residual_stage1(const double* __restrict__ X, const double* __restrict__ AX, const double* __restrict__ theta, uint32_t n, int b,
                                                                uint32_t rows_per_block, double* __restrict__ partial) {
  __shared__ double part[SP_THREADS];
  const int t = threadIdx.x, rpb = SP_THREADS / b, rl = t / b, c = t - rl * b;
  const uint64_t r0 = std::min<uint64_t>((uint64_t)blockIdx.x * rows_per_block, n), r1 = std::min<uint64_t>(r0 + rows_per_block, n);
  double acc = 0.0;
  if (rl < rpb) {
    const double th = theta[c];
    for (uint64_t r = r0 + rl; r < r1; r += rpb) {
      const double d = AX[r * b + c] - th * X[r * b + c];
      acc = fma(d, d, acc);
    }
  }
  part[t] = acc;
  __syncthreads();
  if (t < b) {
    double a = 0.0;
    for (int u = 0; u < rpb; ++u) a += part[u * b + t];
    partial[(size_t)blockIdx.x * b + t] = a;
  }
}

// the sign rule, stage 1: per block and column the largest |x| of the block's rows, the lowest row among equals, and x there
struct SignRec { double mag, value; uint32_t row; uint32_t pad; };
__global__ __launch_bounds__(SP_THREADS) void k_sign_stage1(const double* __restrict__ X, uint32_t n, int b, uint32_t rows_per_block, SignRec* __restrict__ partial) {
  __shared__ SignRec part[SP_THREADS];
  const int t = threadIdx.x, rpb = SP_THREADS / b, rl = t / b, c = t - rl * b;
  const uint64_t r0 = std::min<uint64_t>((uint64_t)blockIdx.x * rows_per_block, n), r1 = std::min<uint64_t>(r0 + rows_per_block, n);
  SignRec best{-1.0, 0.0, SP_NONE, 0u};
  if (rl < rpb)
    for (uint64_t r = r0 + rl; r < r1; r += rpb) {
      const double v = X[r * b + c], m = fabs(v);
      if (m > best.mag) best = SignRec{m, v, (uint32_t)r, 0u};      // (ascending rows: the first one stays)
    }
  part[t] = best;
  __syncthreads();
  if (t < b) {
    SignRec a = part[t];
    for (int u = 1; u < rpb; ++u) {
      const SignRec o = part[u * b + t];
      if (o.mag > a.mag || (o.mag == a.mag && o.row < a.row)) a = o;
    }
    partial[(size_t)blockIdx.x * b + t] = a;
  }
}
__global__ void k_sign_stage2(const SignRec* __restrict__ partial, int blocks, int b, double* __restrict__ sign) {
  const int c = threadIdx.x;
  if (c >= b) return;
  SignRec a = partial[c];
  for (int B = 1; B < blocks; ++B) {
    const SignRec o = partial[(size_t)B * b + c];
    if (o.mag > a.mag || (o.mag == a.mag && o.row < a.row)) a = o;
  }
  sign[c] = a.value < 0.0 ? -1.0 : 1.0;
}

// the start block: a counter-based hash of (row, column) (splitmix64's finaliser), uniform in [-1, 1)
__global__ __launch_bounds__(SP_THREADS) void k_start_block(double* __restrict__ X, uint64_t total, int b) {
  for (uint64_t o = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; o < total; o += (uint64_t)gridDim.x * SP_THREADS) {
    const uint64_t r = o / b, c = o - r * b;
    uint64_t z = (r * 64u + c + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    X[o] = (double)(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;      // 2^-52: [0, 2) - 1
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
// shape of a two-stage sum over n rows
struct TwoStage { int blocks; uint32_t rows_per_block; };
inline TwoStage two_stage(size_t n) {
  const size_t nb = std::min<size_t>(SP_PARTIAL_BLOCKS, std::max<size_t>((n + 63) / 64, 1));
  return TwoStage{(int)nb, (uint32_t)((n + nb - 1) / nb)};
}

// the b x b work of a subspace iteration over row-major [n][b] f64 blocks on one stream
struct SubspaceOps {
  const char* F = "spectral_embedding";
  hipStream_t s;
  int b = 0;
  size_t n = 0;
  TwoStage ts{};
  double* small = nullptr;      // [0, 1024) a b x b matrix, [1024, 1056) theta, [1056, 1088) signs
  double* out = nullptr;        // [1024] result of a two-stage sum
  double* partial = nullptr;    // [SP_PARTIAL_BLOCKS * 1024]

  // host[b * b] = X^T Y
  int gram(const double* X, const double* Y, double* host) {
    hipLaunchKernelGGL(k_gram_stage1, dim3(ts.blocks), dim3(SP_THREADS), 0, s, X, Y, (uint32_t)n, b, ts.rows_per_block, partial);
    hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)partial, ts.blocks, b * b, out);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(host, out, (size_t)b * b * sizeof(double), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    return CILHIP_OK;
  }
  // Out = X M (M: host b x b)
  int mul(const double* X, const double* M, double* Out) {
    ST_CK(F, hipMemcpyAsync(small, M, (size_t)b * b * sizeof(double), hipMemcpyHostToDevice, s));
    ST_CK(F, hipStreamSynchronize(s));      // (M is the caller's stack)
    hipLaunchKernelGGL(k_block_mul, dim3(sp_grid(n * b, 2048)), dim3(SP_THREADS), 0, s, X, (const double*)small, Out, (uint64_t)n * b, b);
    ST_CK(F, hipGetLastError());
    return CILHIP_OK;
  }
  // CholQR2 of the columns [first, b) with the columns scaled to unit length first (the filter leaves columns of very different lengths);
  // the columns before `first` (locked, already orthonormal, and the rest already orthogonal to them) pass through unchanged; *X and *T swap
  int orthonormalise(double** X, double** T, int first = 0) {
    double G[SP_MAX_B * SP_MAX_B], R[SP_MAX_B * SP_MAX_B], Ri[SP_MAX_B * SP_MAX_B], dd[SP_MAX_B], Gf[SP_MAX_B * SP_MAX_B], M[SP_MAX_B * SP_MAX_B];
    const int m = b - first;
    int passes = 2;
    for (int pass = 0; pass < passes; ++pass) {
      if (const int rc = gram(*X, *X, Gf)) return rc;
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) G[i * m + j] = Gf[(first + i) * b + first + j];
      for (int i = 0; i < m; ++i) { const double g = G[i * m + i]; dd[i] = (g > 0.0 && std::isfinite(g)) ? std::sqrt(g) : 1.0; }
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) G[i * m + j] = 0.5 * (G[i * m + j] + G[j * m + i]) / (dd[i] * dd[j]);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < i; ++j) G[i * m + j] = G[j * m + i];
      double shift = 0.0;
      for (int attempt = 0; !cilhip::sym_cholesky(G, m, R); ++attempt) {      // (nearly dependent columns: shifted CholQR, one more pass)
        if (attempt == 8) return cilhip::st_fail(CILHIP_ERR_HIP, F, "the block lost its rank");
        const double add = shift == 0.0 ? 1e-13 * m : shift * 99.0;
        for (int i = 0; i < m; ++i) G[i * m + i] += add;
        shift += add;
        if (passes < 4) passes = pass + 3 > 4 ? 4 : pass + 3;
      }
      cilhip::upper_inverse(R, m, Ri);
      for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) Ri[i * m + j] /= dd[i];
      const double* Mp = Ri;
      if (first > 0) {
        for (int i = 0; i < b; ++i)
          for (int j = 0; j < b; ++j) M[i * b + j] = (i >= first && j >= first) ? Ri[(i - first) * m + j - first] : (i == j ? 1.0 : 0.0);
        Mp = M;
      }
      if (const int rc = mul(*X, Mp, *T)) return rc;
      std::swap(*X, *T);
    }
    return CILHIP_OK;
  }
};

// The filter: `degree` steps of the three-term recurrence that damps [c - e, c + e] and is scaled to 1 at a0, each step one call
// product(X, Z, Y, alpha, c, beta): Y = alpha (A X - c X) + beta Z.  X is the block on entry and the filtered block on return; T1 and T2
// are the two spare blocks (the three pointers rotate).
template <class Product> int cheb_filter(Product&& product, double e, double c, double a0, int degree, double*& X, double*& T1, double*& T2) {
  double sigma = e / (a0 - c);
  const double sigma1 = sigma;
  double *Yp = X, *Yc = T1, *Yn = T2;
  if (const int rc = product(Yp, nullptr, Yc, sigma1 / e, c, 0.0)) return rc;
  for (int i = 2; i <= degree; ++i) {
    const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
    if (const int rc = product(Yc, Yp, Yn, 2.0 * sigma2 / e, c, -sigma * sigma2)) return rc;
    double* const old = Yp;
    Yp = Yc; Yc = Yn; Yn = old;
    sigma = sigma2;
  }
  X = Yc; T1 = Yp; T2 = Yn;
  return CILHIP_OK;
}

template <class Fn> int sp_guard(const char* family, Fn&& fn) {
  try { return fn(); } catch (const std::bad_alloc&) { return cilhip::st_fail(CILHIP_ERR_HIP, family, "out of host memory"); } catch (...) { return cilhip::st_fail(CILHIP_ERR_HIP, family, "unexpected exception"); }
}

}  // namespace

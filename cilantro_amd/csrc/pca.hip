// pca.hip -- PrincipalComponentAnalysis<float> on the device (the rules P1-P5 are stated in c_api.h):
//   P1, P2  mean and covariance of n points in 1 <= D <= 16 dimensions (optionally of a subset): fixed-order f64 two-stage sums
//           k_pca_moments_stage1<0 / 1>, k_stage2 (subspace_device.hpp)
//   P4      eigenpairs of the D x D covariance: sym_jacobi on the host (small_sym.hpp), signs, determinant
//   P5      project / reconstruct: one lane per point, matrix and mean in LDS                       k_pca_project, k_pca_reconstruct
// No atomic touches a sum: two runs agree bit for bit.
#include "../../include/cilantro_hip/c_api.h"
#include "small_sym.hpp"
#include "stateless.hpp"
#include "subspace_device.hpp"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <limits>

namespace {

constexpr int PCA_MAX_DIM = 16;

// stage 1 of the moment sums.  Block B owns the entries [B rows_per_block, (B + 1) rows_per_block) of the sample (the subset list, or the
// points themselves) and one lane per accumulator sums them in ascending order.  PASS 0: the D coordinate sums; PASS 1: the D * D sums of
// products of tmp = x - mean (f32, as the reference subtracts), each product and the sum in f64.  partial[B][D or D * D].  PASS 0 also
// flags a subset index that is not below n.
template <int PASS>
__global__ __launch_bounds__(SP_THREADS) void k_pca_moments_stage1(const float* __restrict__ x, uint32_t n, int D, const uint32_t* __restrict__ subset, uint32_t count,
                                                                   const float* __restrict__ mean, uint32_t rows_per_block, double* __restrict__ partial, unsigned int* __restrict__ err) {
  const int t = threadIdx.x, nacc = PASS == 0 ? D : D * D;
  const uint64_t r0 = std::min<uint64_t>((uint64_t)blockIdx.x * rows_per_block, count), r1 = std::min<uint64_t>(r0 + rows_per_block, count);
  if (t >= nacc) return;
  const int a = PASS == 0 ? t : t / D, c = PASS == 0 ? 0 : t - a * D;
  const float ma = PASS == 0 ? 0.0f : mean[a], mc = PASS == 0 ? 0.0f : mean[c];
  double acc = 0.0;
  bool bad = false;
  for (uint64_t e = r0; e < r1; ++e) {
    uint64_t i = e;
    if (subset != nullptr) {
      i = subset[e];
      if (i >= n) { bad = true; continue; }
    }
    if (PASS == 0) acc += (double)x[i * D + a];
    else acc = fma((double)__fsub_rn(x[i * D + a], ma), (double)__fsub_rn(x[i * D + c], mc), acc);
  }
  partial[(size_t)blockIdx.x * nacc + t] = acc;
  if (PASS == 0 && bad) atomicOr(err, 1u);
}

// P5: out[i][t] = (float)(sum over k, ascending, of V[t][k] * (x[i][k] - mean[k])): the difference in f32, products and sum in f64
__global__ __launch_bounds__(SP_THREADS) void k_pca_project(const float* __restrict__ x, uint32_t m, int D, int target, const float* __restrict__ mean, const float* __restrict__ vec,
                                                            float* __restrict__ out) {
  __shared__ float sv[PCA_MAX_DIM * PCA_MAX_DIM], sm[PCA_MAX_DIM];
  for (int u = threadIdx.x; u < D * D; u += SP_THREADS) sv[u] = vec[u];
  if (threadIdx.x < D) sm[threadIdx.x] = mean[threadIdx.x];
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < m; i += (uint64_t)gridDim.x * SP_THREADS) {
    float d[PCA_MAX_DIM];
#pragma unroll
    for (int k = 0; k < PCA_MAX_DIM; ++k) d[k] = k < D ? __fsub_rn(x[i * D + k], sm[k]) : 0.0f;
    for (int t = 0; t < target; ++t) {
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < PCA_MAX_DIM; ++k)
        if (k < D) a = fma((double)sv[t * D + k], (double)d[k], a);
      out[i * target + t] = (float)a;
    }
  }
}

// P5: out[i][k] = (float)((sum over t < source, ascending, of V[t][k] * y[i][t]) + mean[k]) in f64, rounded once
__global__ __launch_bounds__(SP_THREADS) void k_pca_reconstruct(const float* __restrict__ y, uint32_t m, int source, int D, const float* __restrict__ mean, const float* __restrict__ vec,
                                                                float* __restrict__ out) {
  __shared__ float sv[PCA_MAX_DIM * PCA_MAX_DIM], sm[PCA_MAX_DIM];
  for (int u = threadIdx.x; u < D * D; u += SP_THREADS) sv[u] = vec[u];
  if (threadIdx.x < D) sm[threadIdx.x] = mean[threadIdx.x];
  __syncthreads();
  for (uint64_t i = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < m; i += (uint64_t)gridDim.x * SP_THREADS) {
    float p[PCA_MAX_DIM];
#pragma unroll
    for (int t = 0; t < PCA_MAX_DIM; ++t) p[t] = t < source ? y[i * source + t] : 0.0f;
    for (int k = 0; k < D; ++k) {
      double a = 0.0;
#pragma unroll
      for (int t = 0; t < PCA_MAX_DIM; ++t)
        if (t < source) a = fma((double)sv[t * D + k], (double)p[t], a);
      out[i * D + k] = (float)(a + (double)sm[k]);
    }
  }
}

// determinant of a D x D matrix (row-major, destroyed): elimination with partial pivoting
double small_det(double* A, int D) {
  double det = 1.0;
  for (int c = 0; c < D; ++c) {
    int p = c;
    for (int r = c + 1; r < D; ++r) if (std::fabs(A[r * D + c]) > std::fabs(A[p * D + c])) p = r;
    if (A[p * D + c] == 0.0) return 0.0;
    if (p != c) { for (int k = 0; k < D; ++k) std::swap(A[p * D + k], A[c * D + k]); det = -det; }
    det *= A[c * D + c];
    for (int r = c + 1; r < D; ++r) {
      const double f = A[r * D + c] / A[c * D + c];
      for (int k = c; k < D; ++k) A[r * D + k] -= f * A[c * D + k];
    }
  }
  return det;
}

// P4 (principal_component_analysis.hpp:76-84): eigenvalues descending, vector c in vectors[c * D ...]
void pca_eigen(const float* cov, int D, float* values, float* vectors) {
  double A[PCA_MAX_DIM * PCA_MAX_DIM], V[PCA_MAX_DIM * PCA_MAX_DIM], w[PCA_MAX_DIM], Q[PCA_MAX_DIM * PCA_MAX_DIM];
  for (int i = 0; i < D; ++i)
    for (int j = 0; j < D; ++j) A[i * D + j] = 0.5 * ((double)cov[i * D + j] + (double)cov[j * D + i]);
  cilhip::sym_jacobi(A, D, w, V);
  for (int c = 0; c < D; ++c) {      // descending: column D - 1 - c of V becomes row c of Q
    const int src = D - 1 - c;
    int pick = 0;
    for (int k = 1; k < D; ++k) if (std::fabs(V[k * D + src]) > std::fabs(V[pick * D + src])) pick = k;      // (the lowest index among equals)
    const double sign = (c < D - 1 && V[pick * D + src] < 0.0) ? -1.0 : 1.0;
    for (int k = 0; k < D; ++k) Q[c * D + k] = sign * V[k * D + src];
    values[c] = (float)w[src];
  }
  for (int i = 0; i < D * D; ++i) A[i] = Q[i];
  if (small_det(A, D) < 0.0)
    for (int k = 0; k < D; ++k) Q[(D - 1) * D + k] = -Q[(D - 1) * D + k];
  for (int i = 0; i < D * D; ++i) vectors[i] = (float)Q[i];
}

int fit_impl(const float* x, size_t n, int D, const uint32_t* subset, size_t n_subset, int mem, float* mean_out, float* cov_out, float* values_out, float* vectors_out, int* valid_out) {
  const char* F = "pca_fit";
  const size_t count = subset ? n_subset : n;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  const float* d_x = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, mem, x, n * (size_t)D, &d_x));
  const uint32_t* d_sub = subset;
  if (subset && mem != CILHIP_MEM_DEVICE) {
    uint32_t* up = nullptr;
    ST_CK(F, pool.get(&up, n_subset));
    if (n_subset) ST_CK(F, hipMemcpyAsync(up, subset, n_subset * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    d_sub = up;
  }
  const TwoStage ts = two_stage(count);
  double *partial = nullptr, *sums = nullptr;
  float* d_mean = nullptr;
  unsigned int* d_err = nullptr;
  ST_CK(F, pool.get(&partial, (size_t)SP_PARTIAL_BLOCKS * PCA_MAX_DIM * PCA_MAX_DIM)); ST_CK(F, pool.get(&sums, PCA_MAX_DIM * PCA_MAX_DIM));
  ST_CK(F, pool.get(&d_mean, PCA_MAX_DIM)); ST_CK(F, pool.get(&d_err, 1));
  ST_CK(F, hipMemsetAsync(d_err, 0, sizeof(unsigned int), s));
  double hs[PCA_MAX_DIM * PCA_MAX_DIM];
  unsigned int err = 0;
  hipLaunchKernelGGL(k_pca_moments_stage1<0>, dim3(ts.blocks), dim3(SP_THREADS), 0, s, d_x, (uint32_t)n, D, d_sub, (uint32_t)count, (const float*)nullptr, ts.rows_per_block, partial, d_err);
  hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)partial, ts.blocks, D, sums);
  ST_CK(F, hipGetLastError());
  ST_CK(F, hipMemcpyAsync(hs, sums, D * sizeof(double), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipMemcpyAsync(&err, d_err, sizeof(err), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  if (err) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "a subset index is not below n");
  if (count < 2) {      // P3 (covariance.hpp:35-39)
    for (int i = 0; i < D; ++i) mean_out[i] = values_out[i] = nan;
    for (int i = 0; i < D * D; ++i) cov_out[i] = vectors_out[i] = nan;
    *valid_out = 0;
    return CILHIP_OK;
  }
  float mean[PCA_MAX_DIM];
  for (int i = 0; i < D; ++i) mean[i] = (float)(hs[i] / (double)count);
  ST_CK(F, hipMemcpyAsync(d_mean, mean, D * sizeof(float), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_pca_moments_stage1<1>, dim3(ts.blocks), dim3(SP_THREADS), 0, s, d_x, (uint32_t)n, D, d_sub, (uint32_t)count, (const float*)d_mean, ts.rows_per_block, partial, d_err);
  hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)partial, ts.blocks, D * D, sums);
  ST_CK(F, hipGetLastError());
  ST_CK(F, hipMemcpyAsync(hs, sums, (size_t)D * D * sizeof(double), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  for (int i = 0; i < D; ++i) mean_out[i] = mean[i];
  for (int i = 0; i < D * D; ++i) cov_out[i] = (float)(hs[i] / (double)(count - 1));
  pca_eigen(cov_out, D, values_out, vectors_out);
  *valid_out = 1;
  return CILHIP_OK;
}

// project (source == 0) or reconstruct
int map_impl(const char* F, const float* in, size_t m, int D, int other, bool reconstruct, int mem, const float* mean, const float* vectors, float* out) {
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  const size_t in_w = reconstruct ? (size_t)other : (size_t)D, out_w = reconstruct ? (size_t)D : (size_t)other;
  const float* d_in = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, mem, in, m * in_w, &d_in));
  float *d_mean = nullptr, *d_vec = nullptr, *d_out = out;
  ST_CK(F, pool.get(&d_mean, PCA_MAX_DIM)); ST_CK(F, pool.get(&d_vec, PCA_MAX_DIM * PCA_MAX_DIM));
  ST_CK(F, hipMemcpyAsync(d_mean, mean, D * sizeof(float), hipMemcpyHostToDevice, s));
  ST_CK(F, hipMemcpyAsync(d_vec, vectors, (size_t)D * D * sizeof(float), hipMemcpyHostToDevice, s));
  if (mem != CILHIP_MEM_DEVICE) ST_CK(F, pool.get(&d_out, m * out_w));
  if (reconstruct) hipLaunchKernelGGL(k_pca_reconstruct, dim3(sp_grid(m, 2048)), dim3(SP_THREADS), 0, s, d_in, (uint32_t)m, other, D, (const float*)d_mean, (const float*)d_vec, d_out);
  else hipLaunchKernelGGL(k_pca_project, dim3(sp_grid(m, 2048)), dim3(SP_THREADS), 0, s, d_in, (uint32_t)m, D, other, (const float*)d_mean, (const float*)d_vec, d_out);
  ST_CK(F, hipGetLastError());
  if (mem != CILHIP_MEM_DEVICE && m * out_w) ST_CK(F, hipMemcpyAsync(out, d_out, m * out_w * sizeof(float), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  return CILHIP_OK;
}

int map_entry(const char* F, int device, const float* in, size_t m, size_t dim, size_t other, bool reconstruct, int mem, const float* mean, const float* vectors, float* out) {
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!in || !mean || !vectors || !out) return refuse("the points, mean, eigenvectors or the output is NULL");
  if (m == 0 || m >= SP_MAX_N) return refuse("the number of points must lie in [1, 2^32 - 16)");
  if (dim == 0 || dim > (size_t)PCA_MAX_DIM) return refuse("dim must lie in [1, 16]");
  if (other == 0 || other > dim) return refuse(reconstruct ? "P5: source_dim must lie in [1, dim]" : "P5: target_dim must lie in [1, dim]");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device)) return open;
  return sp_guard(F, [&]() -> int { return map_impl(F, in, m, (int)dim, (int)other, reconstruct, mem, mean, vectors, out); });
}

}  // namespace

extern "C" {

int cilhip_pca_fit(int device, const float* x, size_t n, size_t dim, const uint32_t* subset_or_null, size_t n_subset, int mem, float* mean_out, float* cov_out,
                   float* eigenvalues_out, float* eigenvectors_out, int* valid_out) {
  const char* F = "pca_fit";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!x || !mean_out || !cov_out || !eigenvalues_out || !eigenvectors_out || !valid_out) return refuse("x or an output is NULL");
  if (n == 0 || n >= SP_MAX_N) return refuse("n must lie in [1, 2^32 - 16)");
  if (dim == 0 || dim > (size_t)PCA_MAX_DIM) return refuse("dim must lie in [1, 16]");
  if (subset_or_null && n_subset >= SP_MAX_N) return refuse("n_subset must lie below 2^32 - 16");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device)) return open;
  return sp_guard(F, [&]() -> int { return fit_impl(x, n, (int)dim, subset_or_null, n_subset, mem, mean_out, cov_out, eigenvalues_out, eigenvectors_out, valid_out); });
}

int cilhip_pca_project(int device, const float* x, size_t m, size_t dim, int mem, const float* mean, const float* eigenvectors, size_t target_dim, float* out) {
  return map_entry("pca_project", device, x, m, dim, target_dim, false, mem, mean, eigenvectors, out);
}

int cilhip_pca_reconstruct(int device, const float* y, size_t m, size_t source_dim, size_t dim, int mem, const float* mean, const float* eigenvectors, float* out) {
  return map_entry("pca_reconstruct", device, y, m, dim, source_dim, true, mem, mean, eigenvectors, out);
}

}  // extern "C"

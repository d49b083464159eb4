// spectral.hip -- SpectralClustering<float> on the device (the rules S1-S6 are stated in c_api.h):
//   S1  neighbour lists -> sparse affinity matrix (getNNGraphFunctionValueSparseMatrix)      k_graph_*: count, scan, fill, sort, merge
//   S2  the Laplacian as an operator that is never assembled                                  k_degrees, k_block_product
//   S4  Chebyshev-filtered subspace iteration, matrix-free, f64                                k_block_product (the hot path); the b x b products,
//       block updates, residuals, CholQR2 and the recurrence: subspace_device.hpp (shared with mds.hip); small dense work: small_sym.hpp
//   S5  signs, scaling, rounding                                                               k_sign_stage1 / 2 (subspace_device.hpp), k_epilogue
//   S6  k-means in D dimensions                                                                k_nd_assign, k_nd_sums, k_nd_farthest
// Every sum runs in an order the input alone decides and the only atomics are integer ones: two runs agree bit for bit.
#include "../../include/cilantro_hip/c_api.h"
#include "internal.hpp"
#include "search_device.hpp"
#include "small_sym.hpp"
#include "stateless.hpp"
#include "subspace_device.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

struct cilhip_sparse {
  int device = 0;
  size_t n = 0, nnz = 0, longest = 0;
  cilhip::DevBuf<uint64_t> off;   // [n + 1]
  cilhip::DevBuf<uint32_t> col;   // [nnz] strictly ascending per row
  cilhip::DevBuf<float> val;      // [nnz]
  ~cilhip_sparse() { (void)hipSetDevice(device); }
};

namespace {

using cilhip::corr_weight;
using cilhip::CW_IDENTITY;
using cilhip::CW_RBF;
using cilhip::CW_UNITY;

enum { SP_ERR_INDEX = 1u, SP_ERR_OFFSETS = 2u, SP_ERR_ORDER = 4u, SP_ERR_VALUE = 8u };

// ---- S1: the graph builder ----------------------------------------------------------------------------------------------------------
struct SpEnt { uint64_t ord; uint32_t col; float val; };      // ord = (source list i) << 32 | position in that list

struct GraphArgs {
  const uint64_t* offsets;      // CSR lists, or null: the k-NN layout
  const uint32_t* idx;
  const float* d2;              // may be null for the Unity kernel
  uint32_t n;
  uint64_t k_or_total;
  int kind; float coeff;
  int sym;
};

// the list of point i: entries [lo, hi) of idx / d2; false: the offsets are broken
__device__ __forceinline__ bool graph_list(const GraphArgs& a, uint32_t i, uint64_t& lo, uint64_t& hi) {
  if (a.offsets == nullptr) { lo = (uint64_t)i * a.k_or_total; hi = lo + a.k_or_total; return true; }
  lo = a.offsets[i]; hi = a.offsets[i + 1];
  return lo <= hi && hi <= a.k_or_total && (i + 1 < a.n || hi == a.k_or_total) && (i > 0 || lo == 0);
}

// pass 0 counts the entries of every row, pass 1 writes them (cursor: entries written so far per row; any order: the rows are sorted next)
template <int PASS>
__global__ __launch_bounds__(SP_THREADS) void k_graph_scatter(GraphArgs a, uint32_t* __restrict__ count, const uint64_t* __restrict__ row_off, SpEnt* __restrict__ ent,
                                                              unsigned int* __restrict__ err) {
  for (uint64_t t = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; t < a.n; t += (uint64_t)gridDim.x * SP_THREADS) {
    const uint32_t i = (uint32_t)t;
    uint64_t lo, hi;
    if (!graph_list(a, i, lo, hi)) { if (PASS == 0) atomicOr(err, (unsigned int)SP_ERR_OFFSETS); continue; }
    for (uint64_t e = lo; e < hi; ++e) {
      const uint32_t j = a.idx[e];
      if (a.offsets == nullptr && j == SP_NONE) continue;      // padding of a short k-NN list
      if (j >= a.n) { if (PASS == 0) atomicOr(err, (unsigned int)SP_ERR_INDEX); continue; }
      if (PASS == 0) {
        atomicAdd(&count[j], 1u);
        if (a.sym) atomicAdd(&count[i], 1u);
      } else {
        const float v = corr_weight(a.kind, a.coeff, a.kind == CW_UNITY ? 0.0f : a.d2[e]);
        const uint64_t ord = ((uint64_t)i << 32) | (uint64_t)((e - lo) & 0xFFFFFFFFull);
        ent[row_off[j] + atomicAdd(&count[j], 1u)] = SpEnt{ord, i, v};           // M(idx, i) = val
        if (a.sym) ent[row_off[i] + atomicAdd(&count[i], 1u)] = SpEnt{ord, j, v};   // M(i, idx) = val
      }
    }
  }
}

// exclusive scan of count[n] into off[n + 1] and the largest count, by ONE block (n words: microseconds)
__global__ __launch_bounds__(1024) void k_scan_counts(const uint32_t* __restrict__ count, uint32_t n, uint64_t* __restrict__ off, unsigned int* __restrict__ longest) {
  __shared__ uint64_t part[1024];
  const uint32_t chunk = (n + 1023u) / 1024u;
  const uint64_t b0 = std::min<uint64_t>((uint64_t)threadIdx.x * chunk, n), b1 = std::min<uint64_t>(b0 + chunk, n);
  uint64_t s = 0;
  unsigned int mx = 0;
  for (uint64_t r = b0; r < b1; ++r) { s += count[r]; mx = max(mx, count[r]); }
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t run = 0;
    for (int t = 0; t < 1024; ++t) { const uint64_t v = part[t]; part[t] = run; run += v; }
    off[n] = run;
  }
  __syncthreads();
  uint64_t run = part[threadIdx.x];
  for (uint64_t r = b0; r < b1; ++r) { off[r] = run; run += count[r]; }
  if (mx) atomicMax(longest, mx);
}

// one row per lane: the row's entries sorted by (column, ord) in place, then the number of distinct columns
__global__ __launch_bounds__(SP_THREADS) void k_graph_sort_rows(SpEnt* __restrict__ ent, const uint64_t* __restrict__ row_off, uint32_t n, uint32_t* __restrict__ ucount) {
  for (uint64_t r = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * SP_THREADS) {
    SpEnt* const row = ent + row_off[r];
    const uint64_t len = row_off[r + 1] - row_off[r];
    for (uint64_t u = 1; u < len; ++u) {      // insertion sort: rows hold tens of entries
      const SpEnt x = row[u];
      uint64_t v = u;
      while (v > 0 && (row[v - 1].col > x.col || (row[v - 1].col == x.col && row[v - 1].ord > x.ord))) { row[v] = row[v - 1]; --v; }
      row[v] = x;
    }
    uint32_t distinct = 0;
    for (uint64_t u = 0; u < len; ++u) distinct += (u == 0 || row[u].col != row[u - 1].col) ? 1u : 0u;
    ucount[r] = distinct;
  }
}

// duplicates 0: the values on one (row, column) summed in ord order (f32); 1: the last one stays
__global__ __launch_bounds__(SP_THREADS) void k_graph_merge(const SpEnt* __restrict__ ent, const uint64_t* __restrict__ row_off, uint32_t n, int assign,
                                                            const uint64_t* __restrict__ off, uint32_t* __restrict__ col, float* __restrict__ val) {
  for (uint64_t r = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * SP_THREADS) {
    const SpEnt* const row = ent + row_off[r];
    const uint64_t len = row_off[r + 1] - row_off[r];
    uint64_t o = off[r];
    for (uint64_t u = 0; u < len;) {
      const uint32_t c = row[u].col;
      float v = row[u].val;
      for (++u; u < len && row[u].col == c; ++u) v = assign ? row[u].val : __fadd_rn(v, row[u].val);
      col[o] = c; val[o] = v; ++o;
    }
  }
}

// cilhip_sparse_from_csr: the rules a caller's matrix must keep, one row per lane
__global__ __launch_bounds__(SP_THREADS) void k_csr_check(const uint64_t* __restrict__ off, const uint32_t* __restrict__ col, const float* __restrict__ val, uint32_t n, uint64_t nnz,
                                                          unsigned int* __restrict__ err, unsigned int* __restrict__ longest) {
  for (uint64_t r = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * SP_THREADS) {
    const uint64_t lo = off[r], hi = off[r + 1];
    if (!(lo <= hi && hi <= nnz) || (r == 0 && lo != 0)) { atomicOr(err, (unsigned int)SP_ERR_OFFSETS); continue; }
    unsigned int e = 0;
    for (uint64_t u = lo; u < hi; ++u) {
      if (col[u] >= n) e |= SP_ERR_INDEX;
      if (u > lo && col[u] <= col[u - 1]) e |= SP_ERR_ORDER;
      if (!(fabsf(val[u]) < INFINITY)) e |= SP_ERR_VALUE;
    }
    if (e) atomicOr(err, e);
    if (hi - lo) atomicMax(longest, (unsigned int)std::min<uint64_t>(hi - lo, 0xFFFFFFFFull));
  }
}

// ---- S2: degrees and the operator -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void k_degrees(const uint64_t* __restrict__ off, const float* __restrict__ val, uint32_t n, double* __restrict__ deg) {
  for (uint64_t r = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * SP_THREADS) {
    double d = 0.0;
    for (uint64_t e = off[r]; e < off[r + 1]; ++e) d += (double)val[e];      // column order
    deg[r] = d;
  }
}

// (A x)_i = diag_i x_i - s_i sum_j w_ij (s_j x_j): D - W with diag = d, s = 1; I - D^-1/2 W D^-1/2 with diag = 1, s = d^-1/2
struct OpDev {
  const uint64_t* off; const uint32_t* col; const float* val;
  const double* diag; const double* s;
  uint32_t n; int b;
};

// Y = alpha (A X - c X) + beta Z over row-major [n][b] blocks: one whole step of the filter's recurrence.  SPLIT * b lanes work on a row:
// lane (p, c) sums the row's entries p, p + SPLIT, ... for column c -- consecutive lanes read the b consecutive doubles of the gathered
// row of X -- and the SPLIT partial sums are added in ascending p.  Y must not be X; Z may be null when beta is 0.
template <int SPLIT>
__global__ __launch_bounds__(SP_THREADS) void k_block_product(OpDev A, const double* __restrict__ X, const double* __restrict__ Z, double* __restrict__ Y, double alpha,
                                                              double c, double beta) {
  __shared__ double part[SP_THREADS];
  const int lanes = SPLIT * A.b, rpb = SP_THREADS / lanes;
  const int t = threadIdx.x, rl = t / lanes, q = t - rl * lanes, p = q / A.b, cc = q - p * A.b;
  for (uint64_t base = (uint64_t)blockIdx.x * rpb; base < A.n; base += (uint64_t)gridDim.x * rpb) {      // (uniform over the block)
    const uint64_t r = base + rl;
    const bool on = rl < rpb && r < A.n;
    double acc = 0.0;
    if (on) {
      const uint64_t hi = A.off[r + 1];
      for (uint64_t e = A.off[r] + p; e < hi; e += SPLIT) {
        const uint32_t j = A.col[e];
        acc = fma((double)A.val[e] * A.s[j], X[(size_t)j * A.b + cc], acc);
      }
    }
    if (SPLIT > 1) {
      part[t] = acc;
      __syncthreads();
      if (on && p == 0)
        for (int u = 1; u < SPLIT; ++u) acc += part[t + u * A.b];
      __syncthreads();
    }
    if (on && p == 0) {
      const size_t o = (size_t)r * A.b + cc;
      const double x = X[o];
      double y = alpha * ((A.diag[r] * x - A.s[r] * acc) - c * x);
      if (Z != nullptr) y = fma(beta, Z[o], y);
      Y[o] = y;
    }
  }
}

// S5: the first nc vectors, signed, (random walk) scaled by d^-1/2, rounded to f32, (symmetric) each point's vector divided by its norm
__global__ __launch_bounds__(SP_THREADS) void k_epilogue(const double* __restrict__ X, const double* __restrict__ sign, const double* __restrict__ s, uint32_t n, int b, int nc,
                                                         int type, float* __restrict__ out) {
  for (uint64_t r = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; r < n; r += (uint64_t)gridDim.x * SP_THREADS) {
    float v[SP_MAX_B];
    const double scale = type == 2 ? s[r] : 1.0;
    float ss = 0.0f;
#pragma unroll
    for (int c = 0; c < SP_MAX_B; ++c)
      if (c < nc) {
        v[c] = (float)(sign[c] * X[r * b + c] * scale);
        ss = c == 0 ? __fmul_rn(v[c], v[c]) : __fadd_rn(ss, __fmul_rn(v[c], v[c]));
      }
    float f = 1.0f;
    if (type == 1) {
      const float inv = __fdiv_rn(1.0f, __fsqrt_rn(ss));
      if (fabsf(inv) < INFINITY) f = inv;
    }
#pragma unroll
    for (int c = 0; c < SP_MAX_B; ++c)
      if (c < nc) out[r * nc + c] = type == 1 ? __fmul_rn(v[c], f) : v[c];
  }
}

// ---- S6: k-means in D dimensions --------------------------------------------------------------------------------------------------------
constexpr int ND_MAX_DIM = 16;
constexpr size_t ND_MAX_K = 256;

// the pinned distance: ((d0 d0 + d1 d1) + d2 d2) + ... (f32, no contraction)
__device__ __forceinline__ float nd_dist(const float* p, const float* __restrict__ c, int D) {
  float acc = 0.0f;
#pragma unroll
  for (int d = 0; d < ND_MAX_DIM; ++d)
    if (d < D) {
      const float df = __fsub_rn(c[d], p[d]);
      acc = d == 0 ? __fmul_rn(df, df) : __fadd_rn(acc, __fmul_rn(df, df));
    }
  return acc;
}

__global__ __launch_bounds__(SP_THREADS) void k_nd_assign(const float* __restrict__ x, uint32_t n, int D, const float* __restrict__ cent, uint32_t k, uint32_t* __restrict__ labels,
                                                          unsigned int* __restrict__ changed) {
  unsigned int ch = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_THREADS) {
    float p[ND_MAX_DIM];
#pragma unroll
    for (int d = 0; d < ND_MAX_DIM; ++d) p[d] = d < D ? x[i * D + d] : 0.0f;
    float best = INFINITY;
    uint32_t bj = 0;
    for (uint32_t j = 0; j < k; ++j) {      // strict '<' over ascending j
      const float dist = nd_dist(p, cent + (size_t)j * D, D);
      if (dist < best) { best = dist; bj = j; }
    }
    ch += labels[i] != bj ? 1u : 0u;
    labels[i] = bj;
  }
  if (ch) atomicAdd(changed, ch);
}

// stage 1 of the cluster sums: block B owns a chunk of consecutive points; accumulator a = cluster (D + 1) + coordinate (coordinate D: the
// count) is summed by one lane over the chunk in ascending point order; partial[B][k (D + 1)]
__global__ __launch_bounds__(SP_THREADS) void k_nd_sums(const float* __restrict__ x, const uint32_t* __restrict__ labels, uint32_t n, int D, uint32_t k, uint32_t rows_per_block,
                                                        double* __restrict__ partial) {
  const uint32_t nacc = k * (uint32_t)(D + 1);
  const uint64_t r0 = std::min<uint64_t>((uint64_t)blockIdx.x * rows_per_block, n), r1 = std::min<uint64_t>(r0 + rows_per_block, n);
  for (uint32_t a = threadIdx.x; a < nacc; a += SP_THREADS) {
    const uint32_t cluster = a / (uint32_t)(D + 1);
    const int coord = (int)(a - cluster * (uint32_t)(D + 1));
    double acc = 0.0;
    for (uint64_t r = r0; r < r1; ++r)
      if (labels[r] == cluster) acc += coord < D ? (double)x[r * D + coord] : 1.0;
    partial[(size_t)blockIdx.x * nacc + a] = acc;
  }
}

// farthest member of one cluster from a point (the empty-cluster repair, kmeans.hpp:145-168); ties: the lowest index
__global__ __launch_bounds__(SP_THREADS) void k_nd_farthest(const float* __restrict__ x, const uint32_t* __restrict__ labels, uint32_t n, int D, uint32_t cluster,
                                                            const float* __restrict__ from, unsigned long long* __restrict__ best) {
  unsigned long long loc = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SP_THREADS) {
    if (labels[i] != cluster) continue;
    float p[ND_MAX_DIM];
#pragma unroll
    for (int d = 0; d < ND_MAX_DIM; ++d) p[d] = d < D ? x[i * D + d] : 0.0f;
    const float dist = nd_dist(p, from, D);
    const unsigned long long key = ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    loc = key > loc ? key : loc;
  }
  for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_down(loc, off, 64); loc = o > loc ? o : loc; }
  if ((threadIdx.x & 63) == 0 && loc) atomicMax(best, loc);
}

__global__ void k_nd_set_label(uint32_t* labels, uint32_t i, uint32_t v) { if (threadIdx.x == 0 && blockIdx.x == 0) labels[i] = v; }

// ---- host side ----------------------------------------------------------------------------------------------------------------------------
const char* sp_error_text(unsigned int e) {
  return (e & SP_ERR_OFFSETS) ? "offsets must start at 0, ascend and end at the number of entries"
         : (e & SP_ERR_INDEX) ? "an index is not below n"
         : (e & SP_ERR_ORDER) ? "the columns of a row must be strictly ascending (unsorted or duplicate columns)"
                              : "a value is not finite";
}

int graph_impl(int device, size_t n, const uint64_t* offsets, const uint32_t* idx, const float* d2, size_t k_or_total, int mem, int kind, float sigma, int sym, int duplicates,
               cilhip_sparse* h) {
  const char* F = "nn_graph_matrix";
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  const bool knn = offsets == nullptr;
  const size_t total = knn ? n * k_or_total : k_or_total;
  GraphArgs a{};
  a.n = (uint32_t)n; a.k_or_total = k_or_total; a.kind = kind; a.sym = sym ? 1 : 0;
  a.coeff = kind == CW_RBF ? -0.5f / (sigma * sigma) : 0.0f;
  if (mem == CILHIP_MEM_DEVICE) {
    a.offsets = offsets; a.idx = idx; a.d2 = d2;
  } else {
    if (!knn) {
      uint64_t* d = nullptr;
      ST_CK(F, pool.get(&d, n + 1));
      ST_CK(F, hipMemcpyAsync(d, offsets, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
      a.offsets = d;
    }
    uint32_t* di = nullptr;
    ST_CK(F, pool.get(&di, total));
    if (total) ST_CK(F, hipMemcpyAsync(di, idx, total * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    a.idx = di;
    if (d2) {
      float* dd = nullptr;
      ST_CK(F, pool.get(&dd, total));
      if (total) ST_CK(F, hipMemcpyAsync(dd, d2, total * sizeof(float), hipMemcpyHostToDevice, s));
      a.d2 = dd;
    }
  }
  uint32_t *count = nullptr, *ucount = nullptr;
  uint64_t* row_off = nullptr;
  unsigned int* flags = nullptr;      // [0] errors, [1] longest raw row, [2] longest merged row
  ST_CK(F, pool.get(&count, n)); ST_CK(F, pool.get(&ucount, n)); ST_CK(F, pool.get(&row_off, n + 1)); ST_CK(F, pool.get(&flags, 4));
  ST_CK(F, hipMemsetAsync(count, 0, n * sizeof(uint32_t), s));
  ST_CK(F, hipMemsetAsync(flags, 0, 4 * sizeof(unsigned int), s));
  const unsigned grid = sp_grid(n);
  hipLaunchKernelGGL(k_graph_scatter<0>, dim3(grid), dim3(SP_THREADS), 0, s, a, count, (const uint64_t*)nullptr, (SpEnt*)nullptr, flags);
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, (const uint32_t*)count, (uint32_t)n, row_off, flags + 1);
  ST_CK(F, hipGetLastError());
  unsigned int hflags[4] = {0, 0, 0, 0};
  uint64_t raw = 0;
  ST_CK(F, hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipMemcpyAsync(&raw, row_off + n, sizeof(raw), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  if (hflags[0]) return cilhip::st_fail(CILHIP_ERR_INVALID, F, sp_error_text(hflags[0]));
  SpEnt* ent = nullptr;
  ST_CK(F, pool.get(&ent, (size_t)raw));
  ST_CK(F, hipMemsetAsync(count, 0, n * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_graph_scatter<1>, dim3(grid), dim3(SP_THREADS), 0, s, a, count, (const uint64_t*)row_off, ent, flags);
  hipLaunchKernelGGL(k_graph_sort_rows, dim3(grid), dim3(SP_THREADS), 0, s, ent, (const uint64_t*)row_off, (uint32_t)n, ucount);
  ST_CK(F, h->off.alloc(n + 1));
  hipLaunchKernelGGL(k_scan_counts, dim3(1), dim3(1024), 0, s, (const uint32_t*)ucount, (uint32_t)n, h->off.get(), flags + 2);
  ST_CK(F, hipGetLastError());
  uint64_t nnz = 0;
  ST_CK(F, hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipMemcpyAsync(&nnz, h->off.get() + n, sizeof(nnz), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  ST_CK(F, h->col.alloc((size_t)nnz)); ST_CK(F, h->val.alloc((size_t)nnz));
  hipLaunchKernelGGL(k_graph_merge, dim3(grid), dim3(SP_THREADS), 0, s, (const SpEnt*)ent, (const uint64_t*)row_off, (uint32_t)n, duplicates, (const uint64_t*)h->off.get(), h->col.get(),
                     h->val.get());
  ST_CK(F, hipGetLastError());
  ST_CK(F, hipStreamSynchronize(s));
  h->device = device; h->n = n; h->nnz = (size_t)nnz; h->longest = hflags[2];
  return CILHIP_OK;
}

int from_csr_impl(int device, size_t n, const uint64_t* offsets, const uint32_t* columns, const float* values, int mem, cilhip_sparse* h) {
  const char* F = "sparse_from_csr";
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  const hipMemcpyKind kind = mem == CILHIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  uint64_t nnz = 0;
  if (mem == CILHIP_MEM_DEVICE) ST_CK(F, hipMemcpy(&nnz, offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost));
  else nnz = offsets[n];
  if (nnz > ((uint64_t)1 << 40)) return cilhip::st_fail(CILHIP_ERR_INVALID, F, sp_error_text(SP_ERR_OFFSETS));
  ST_CK(F, h->off.alloc(n + 1)); ST_CK(F, h->col.alloc((size_t)nnz)); ST_CK(F, h->val.alloc((size_t)nnz));
  ST_CK(F, hipMemcpyAsync(h->off.get(), offsets, (n + 1) * sizeof(uint64_t), kind, s));
  if (nnz) {
    ST_CK(F, hipMemcpyAsync(h->col.get(), columns, (size_t)nnz * sizeof(uint32_t), kind, s));
    ST_CK(F, hipMemcpyAsync(h->val.get(), values, (size_t)nnz * sizeof(float), kind, s));
  }
  unsigned int* flags = nullptr;
  ST_CK(F, pool.get(&flags, 2));
  ST_CK(F, hipMemsetAsync(flags, 0, 2 * sizeof(unsigned int), s));
  hipLaunchKernelGGL(k_csr_check, dim3(sp_grid(n)), dim3(SP_THREADS), 0, s, (const uint64_t*)h->off.get(), (const uint32_t*)h->col.get(), (const float*)h->val.get(), (uint32_t)n, nnz, flags,
                     flags + 1);
  ST_CK(F, hipGetLastError());
  unsigned int hflags[2] = {0, 0};
  ST_CK(F, hipMemcpyAsync(hflags, flags, sizeof(hflags), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  if (hflags[0]) return cilhip::st_fail(CILHIP_ERR_INVALID, F, sp_error_text(hflags[0]));
  h->device = device; h->n = n; h->nnz = (size_t)nnz; h->longest = hflags[1];
  return CILHIP_OK;
}

// estimateNumberOfClustersEigengap, spectral_clustering.hpp:46-68, literally (f32)
size_t eigengap(const float* ev, size_t count, size_t max_num_clusters) {
  float min_val = INFINITY, max_val = -INFINITY, max_diff = ev[0];
  size_t max_ind = 0;
  for (size_t i = 0; i + 1 < count; ++i) {
    const float diff = ev[i + 1] - ev[i];
    if (diff > max_diff) { max_diff = diff; max_ind = i; }
    if (ev[i] < min_val) min_val = ev[i];
    if (ev[i] > max_val) max_val = ev[i];
  }
  if (ev[count - 1] < min_val) min_val = ev[count - 1];
  if (ev[count - 1] > max_val) max_val = ev[count - 1];
  if (max_val - min_val < FLT_EPSILON) return max_num_clusters;
  return max_ind + 1;
}

struct Solver : SubspaceOps {
  const cilhip_sparse* W;
  OpDev A{};
  int split = 1;
  size_t products = 0;

  int product(const double* X, const double* Z, double* Y, double alpha, double c, double beta) {
    const int rpb = SP_THREADS / (split * b);
    const unsigned grid = (unsigned)std::min<size_t>((n + rpb - 1) / rpb, 2048);
    if (split == 4) hipLaunchKernelGGL(k_block_product<4>, dim3(grid), dim3(SP_THREADS), 0, s, A, X, Z, Y, alpha, c, beta);
    else if (split == 2) hipLaunchKernelGGL(k_block_product<2>, dim3(grid), dim3(SP_THREADS), 0, s, A, X, Z, Y, alpha, c, beta);
    else hipLaunchKernelGGL(k_block_product<1>, dim3(grid), dim3(SP_THREADS), 0, s, A, X, Z, Y, alpha, c, beta);
    ST_CK(F, hipGetLastError());
    ++products;
    return CILHIP_OK;
  }
};

int embedding_impl(const cilhip_sparse* W, const cilhip_spectral_params& prm, size_t max_clusters, bool estimate, size_t nev, float* embedded_out, float* eigenvalues_out, int mem,
                   cilhip_spectral_result* result) {
  const char* F = "spectral_embedding";
  const auto t0 = std::chrono::steady_clock::now();
  const size_t n = W->n;
  const int b = (int)std::min<size_t>(nev + std::max<size_t>((size_t)prm.guard, nev / 2), n);
  const int type = prm.laplacian_type;
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  // S2: degrees
  double *deg = nullptr, *sc = nullptr;
  ST_CK(F, pool.get(&deg, n)); ST_CK(F, pool.get(&sc, n));
  hipLaunchKernelGGL(k_degrees, dim3(sp_grid(n)), dim3(SP_THREADS), 0, s, (const uint64_t*)W->off.get(), (const float*)W->val.get(), (uint32_t)n, deg);
  ST_CK(F, hipGetLastError());
  std::vector<double> hd(n), hs(n);
  ST_CK(F, hipMemcpyAsync(hd.data(), deg, n * sizeof(double), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  double dmax = 0.0;
  for (size_t i = 0; i < n; ++i) {
    if (!std::isfinite(hd[i])) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "a row sum (degree) is not finite");
    if (type != 0 && !(hd[i] > 0.0)) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "a degree is not positive: the normalised Laplacians need d_i > 0");
    dmax = std::max(dmax, hd[i]);
    hs[i] = type == 0 ? 1.0 : 1.0 / std::sqrt(hd[i]);
  }
  double ub = type == 0 ? 2.0 * dmax : 2.0;
  if (!(ub > 0.0)) ub = 1.0;      // (the zero matrix: every value is an eigenvalue's bound)
  if (type != 0) for (size_t i = 0; i < n; ++i) hd[i] = 1.0;      // diag of I - D^-1/2 W D^-1/2
  ST_CK(F, hipMemcpyAsync(deg, hd.data(), n * sizeof(double), hipMemcpyHostToDevice, s));
  ST_CK(F, hipMemcpyAsync(sc, hs.data(), n * sizeof(double), hipMemcpyHostToDevice, s));

  Solver so;
  so.W = W; so.s = s; so.b = b; so.n = n; so.ts = two_stage(n);
  so.A = OpDev{W->off.get(), W->col.get(), W->val.get(), deg, sc, (uint32_t)n, b};
  const double mean_row = (double)W->nnz / (double)n;
  so.split = mean_row >= 48.0 ? 4 : mean_row >= 24.0 ? 2 : 1;      // lanes per row by the mean row length
  ST_CK(F, pool.get(&so.small, 1088)); ST_CK(F, pool.get(&so.out, 1024)); ST_CK(F, pool.get(&so.partial, (size_t)SP_PARTIAL_BLOCKS * 1024));
  SignRec* sign_partial = nullptr;
  ST_CK(F, pool.get(&sign_partial, (size_t)SP_PARTIAL_BLOCKS * SP_MAX_B));
  double* P[4];
  for (int i = 0; i < 4; ++i) ST_CK(F, pool.get(&P[i], n * (size_t)b));
  double *X = P[0], *AX = P[1], *T1 = P[2], *T2 = P[3];
  hipLaunchKernelGGL(k_start_block, dim3(sp_grid(n * b, 2048)), dim3(SP_THREADS), 0, s, X, (uint64_t)n * b, b);
  ST_CK(F, hipGetLastError());
  if (const int rc = so.orthonormalise(&X, &T1)) return rc;

  const double tol = (double)1e-7f, eps23 = (double)std::pow(FLT_EPSILON, 2.0f / 3.0f);
  double G[SP_MAX_B * SP_MAX_B], S[SP_MAX_B * SP_MAX_B], theta[SP_MAX_B], res2[SP_MAX_B];
  size_t outer = 0, n_conv = 0;
  double max_res = 0.0;
  for (;;) {
    ++outer;
    // Rayleigh-Ritz
    if (const int rc = so.product(X, nullptr, AX, 1.0, 0.0, 0.0)) return rc;
    if (const int rc = so.gram(X, AX, G)) return rc;
    for (int i = 0; i < b; ++i)
      for (int j = i + 1; j < b; ++j) G[i * b + j] = G[j * b + i] = 0.5 * (G[i * b + j] + G[j * b + i]);
    cilhip::sym_jacobi(G, b, theta, S);
    if (const int rc = so.mul(X, S, T1)) return rc;
    if (const int rc = so.mul(AX, S, T2)) return rc;
    std::swap(X, T1); std::swap(AX, T2);
    // the true residuals
    ST_CK(F, hipMemcpyAsync(so.small + 1024, theta, b * sizeof(double), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_residual_stage1, dim3(so.ts.blocks), dim3(SP_THREADS), 0, s, (const double*)X, (const double*)AX, (const double*)(so.small + 1024), (uint32_t)n, b,
                       so.ts.rows_per_block, so.partial);
    hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)so.partial, so.ts.blocks, b, so.out);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(res2, so.out, b * sizeof(double), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    n_conv = 0; max_res = 0.0;
    for (size_t i = 0; i < nev; ++i) {
      const double r = std::sqrt(res2[i]);
      max_res = std::max(max_res, r);
      if (r < tol * std::max(eps23, std::fabs(theta[i]))) ++n_conv;
    }
    if (n_conv == nev || outer >= prm.max_outer) break;
    // the filter: damp [a, ub], scaled at a0 (three-term recurrence)
    const double a0 = theta[0];
    double a = theta[b - 1];
    if (!(a > a0)) a = a0 + 0.5 * (ub - a0);
    if (!(a < ub)) a = a0 + 0.5 * (ub - a0);
    if (ub > a0 && a > a0 && a < ub) {
      const double e = 0.5 * (ub - a), c = 0.5 * (ub + a);
      auto product = [&](const double* Xi, const double* Zi, double* Yo, double alpha, double cc, double beta) { return so.product(Xi, Zi, Yo, alpha, cc, beta); };
      if (const int rc = cheb_filter(product, e, c, a0, prm.degree, X, T1, T2)) return rc;
    }
    if (const int rc = so.orthonormalise(&X, &T1)) return rc;
  }

  // S5
  std::vector<float> ev(nev);
  for (size_t i = 0; i < nev; ++i) { ev[i] = (float)theta[i]; if (ev[i] < 0.0f) ev[i] = 0.0f; }
  size_t nc = max_clusters;
  if (estimate) nc = eigengap(ev.data(), nev, max_clusters);
  if (nc > nev) nc = nev;
  hipLaunchKernelGGL(k_sign_stage1, dim3(so.ts.blocks), dim3(SP_THREADS), 0, s, (const double*)X, (uint32_t)n, b, so.ts.rows_per_block, sign_partial);
  hipLaunchKernelGGL(k_sign_stage2, dim3(1), dim3(64), 0, s, (const SignRec*)sign_partial, so.ts.blocks, b, so.small + 1056);
  float* d_out = embedded_out;
  if (mem != CILHIP_MEM_DEVICE) ST_CK(F, pool.get(&d_out, n * nc));
  hipLaunchKernelGGL(k_epilogue, dim3(sp_grid(n)), dim3(SP_THREADS), 0, s, (const double*)X, (const double*)(so.small + 1056), (const double*)sc, (uint32_t)n, b, (int)nc, type, d_out);
  ST_CK(F, hipGetLastError());
  if (mem != CILHIP_MEM_DEVICE) ST_CK(F, hipMemcpyAsync(embedded_out, d_out, n * nc * sizeof(float), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  std::memcpy(eigenvalues_out, ev.data(), nev * sizeof(float));
  result->num_clusters = nc; result->num_eigenvalues = nev; result->n_converged = n_conv; result->outer_iterations = outer; result->block_products = so.products;
  result->max_residual = max_res;
  result->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return CILHIP_OK;
}

int kmeans_nd_impl(const float* x, size_t n, int D, int mem, float* centroids, size_t k, size_t max_iter, float tol, uint32_t* labels_out, size_t* iterations_out) {
  const char* F = "kmeans_nd";
  cilhip::DevPool pool;
  cilhip::StreamGuard s;
  ST_CK(F, s.create());
  const float* d_x = nullptr;
  ST_CK(F, cilhip::st_stage(pool, s, mem, x, n * (size_t)D, &d_x));
  const size_t nacc = k * (size_t)(D + 1);
  const size_t nb = std::min<size_t>(256, (n + 255) / 256);
  const uint32_t rows_per_block = (uint32_t)((n + nb - 1) / nb);
  float* d_c = nullptr; uint32_t* d_lab = nullptr; unsigned int* d_changed = nullptr; unsigned long long* d_best = nullptr; double *d_partial = nullptr, *d_sums = nullptr;
  ST_CK(F, pool.get(&d_c, k * (size_t)D + ND_MAX_DIM)); ST_CK(F, pool.get(&d_lab, n)); ST_CK(F, pool.get(&d_changed, 1)); ST_CK(F, pool.get(&d_best, 1));
  ST_CK(F, pool.get(&d_partial, nb * nacc)); ST_CK(F, pool.get(&d_sums, nacc));
  ST_CK(F, hipMemsetAsync(d_lab, 0, n * sizeof(uint32_t), s));      // point_to_cluster_index_map_.resize(n): zeros (:80)
  std::vector<double> hs(nacc);
  std::vector<float> c_old(k * (size_t)D);
  const float tol_sq = tol * tol;
  const size_t W1 = (size_t)D + 1;
  size_t iter = 0;
  while (iter < max_iter) {
    unsigned int changed = 0;
    ST_CK(F, hipMemcpyAsync(d_c, centroids, k * (size_t)D * sizeof(float), hipMemcpyHostToDevice, s));
    ST_CK(F, hipMemsetAsync(d_changed, 0, sizeof(unsigned int), s));
    hipLaunchKernelGGL(k_nd_assign, dim3(sp_grid(n)), dim3(SP_THREADS), 0, s, d_x, (uint32_t)n, D, (const float*)d_c, (uint32_t)k, d_lab, d_changed);
    hipLaunchKernelGGL(k_nd_sums, dim3((unsigned)nb), dim3(SP_THREADS), 0, s, d_x, (const uint32_t*)d_lab, (uint32_t)n, D, (uint32_t)k, rows_per_block, d_partial);
    hipLaunchKernelGGL(k_stage2, dim3(1), dim3(SP_THREADS), 0, s, (const double*)d_partial, (int)nb, (int)nacc, d_sums);
    ST_CK(F, hipGetLastError());
    ST_CK(F, hipMemcpyAsync(&changed, d_changed, sizeof(changed), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipMemcpyAsync(hs.data(), d_sums, nacc * sizeof(double), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    if (changed == 0 && iter > 0) break;                                              // kmeans.hpp:122
    if (tol > 0.0f) std::memcpy(c_old.data(), centroids, k * (size_t)D * sizeof(float));      // :123
    for (size_t i = 0; i < k; ++i) {                                                  // empty clusters (:134-176), ascending
      if (hs[i * W1 + D] != 0.0) continue;
      size_t mx = 0;
      for (size_t j = 1; j < k; ++j) if (hs[j * W1 + D] > hs[mx * W1 + D]) mx = j;
      const double cm = hs[mx * W1 + D];
      float oc[ND_MAX_DIM];
      for (int d = 0; d < D; ++d) oc[d] = (float)(hs[mx * W1 + d] / cm);
      unsigned long long best = 0;
      ST_CK(F, hipMemcpyAsync(d_c + k * (size_t)D, oc, D * sizeof(float), hipMemcpyHostToDevice, s));
      ST_CK(F, hipMemsetAsync(d_best, 0, sizeof(unsigned long long), s));
      hipLaunchKernelGGL(k_nd_farthest, dim3(sp_grid(n, 1024)), dim3(SP_THREADS), 0, s, d_x, (const uint32_t*)d_lab, (uint32_t)n, D, (uint32_t)mx, (const float*)(d_c + k * (size_t)D), d_best);
      ST_CK(F, hipGetLastError());
      ST_CK(F, hipMemcpyAsync(&best, d_best, sizeof(best), hipMemcpyDeviceToHost, s));
      ST_CK(F, hipStreamSynchronize(s));
      if (best == 0) continue;      // (never taken, n < k included: the counts add up to n >= 1, so the donor -- the largest -- has a member,
                                    // and a member's key ends in 0xFFFFFFFF - i >= 16; kept so that an empty key can never become the index mi)
      const uint32_t mi = 0xFFFFFFFFu - (uint32_t)(best & 0xFFFFFFFFull);
      float p[ND_MAX_DIM];
      hipLaunchKernelGGL(k_nd_set_label, dim3(1), dim3(64), 0, s, d_lab, mi, (uint32_t)i);
      ST_CK(F, hipMemcpyAsync(p, d_x + (size_t)mi * D, D * sizeof(float), hipMemcpyDeviceToHost, s));
      ST_CK(F, hipStreamSynchronize(s));
      for (int d = 0; d < D; ++d) hs[mx * W1 + d] -= (double)p[d];
      hs[mx * W1 + D] -= 1.0; hs[i * W1 + D] += 1.0;      // the reference does not add the point to cluster i's sum (:171-175)
    }
    for (size_t i = 0; i < k; ++i)                                                    // :179-181
      for (int d = 0; d < D; ++d) centroids[i * D + d] = (float)(hs[i * W1 + d] / hs[i * W1 + D]);
    ++iter;
    if (tol > 0.0f) {                                                                  // :186-188
      float mxs = 0.0f;
      for (size_t i = 0; i < k; ++i) {
        float sq = 0.0f;
        for (int d = 0; d < D; ++d) {
          const float df = centroids[i * D + d] - c_old[i * D + d];
          sq = d == 0 ? df * df : sq + df * df;
        }
        if (sq > mxs) mxs = sq;
      }
      if (mxs < tol_sq) break;
    }
  }
  if (labels_out) ST_CK(F, hipMemcpyAsync(labels_out, d_lab, n * sizeof(uint32_t), mem == CILHIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  if (iterations_out) *iterations_out = iter;
  return CILHIP_OK;
}

}  // namespace

extern "C" {

int cilhip_nn_graph_matrix(int device, size_t n, const uint64_t* offsets_or_null, const uint32_t* idx, const float* d2, size_t k_or_total, int mem, int kernel_kind,
                           float kernel_sigma, int force_symmetry, int duplicates, cilhip_sparse** out) {
  const char* F = "nn_graph_matrix";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!out) return refuse("out is NULL");
  if (!idx) return refuse("idx is NULL");
  if (kernel_kind != CW_UNITY && kernel_kind != CW_IDENTITY && kernel_kind != CW_RBF) return refuse("kernel_kind: 0 (Unity), 1 (Identity) or 2 (RBF)");
  if (!d2 && kernel_kind != CW_UNITY) return refuse("d2 is NULL (only the Unity kernel does without distances)");
  if (kernel_kind == CW_RBF && !(std::isfinite(kernel_sigma) && kernel_sigma > 0.0f)) return refuse("kernel_sigma must be finite and positive");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (duplicates != 0 && duplicates != 1) return refuse("duplicates: 0 (summed) or 1 (assigned)");
  if (n == 0 || n >= SP_MAX_N) return refuse("n must lie in [1, 2^32 - 16)");
  if (!offsets_or_null && (k_or_total == 0 || k_or_total >= ((uint64_t)1 << 32) / n)) return refuse("k must be positive and n * k below 2^32");
  if (offsets_or_null && k_or_total >= ((uint64_t)1 << 31)) return refuse("the lists hold 2^31 entries or more");
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device)) return open;
  return sp_guard(F, [&]() -> int {
    cilhip_sparse* h = new (std::nothrow) cilhip_sparse();
    if (!h) return cilhip::st_fail(CILHIP_ERR_HIP, F, "out of host memory");
    h->device = device;
    const int rc = graph_impl(device, n, offsets_or_null, idx, d2, k_or_total, mem, kernel_kind, kernel_sigma, force_symmetry, duplicates, h);
    if (rc != CILHIP_OK) { delete h; return rc; }
    *out = h;
    return CILHIP_OK;
  });
}

int cilhip_sparse_from_csr(int device, size_t n, const uint64_t* offsets, const uint32_t* columns, const float* values, int mem, cilhip_sparse** out) {
  const char* F = "sparse_from_csr";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!out) return refuse("out is NULL");
  if (!offsets || !columns || !values) return refuse("offsets, columns or values is NULL");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (n == 0 || n >= SP_MAX_N) return refuse("n must lie in [1, 2^32 - 16)");
  if (mem == CILHIP_MEM_HOST) {      // the rules, before a device is needed
    if (offsets[0] != 0) return refuse(sp_error_text(SP_ERR_OFFSETS));
    for (size_t r = 0; r < n; ++r)
      if (offsets[r] > offsets[r + 1]) return refuse(sp_error_text(SP_ERR_OFFSETS));
    for (size_t r = 0; r < n; ++r) {
      for (uint64_t u = offsets[r]; u < offsets[r + 1]; ++u) {
        if (columns[u] >= n) return refuse(sp_error_text(SP_ERR_INDEX));
        if (u > offsets[r] && columns[u] <= columns[u - 1]) return refuse(sp_error_text(SP_ERR_ORDER));
        if (!std::isfinite(values[u])) return refuse(sp_error_text(SP_ERR_VALUE));
      }
    }
  }
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device)) return open;
  return sp_guard(F, [&]() -> int {
    cilhip_sparse* h = new (std::nothrow) cilhip_sparse();
    if (!h) return cilhip::st_fail(CILHIP_ERR_HIP, F, "out of host memory");
    h->device = device;
    const int rc = from_csr_impl(device, n, offsets, columns, values, mem, h);
    if (rc != CILHIP_OK) { delete h; return rc; }
    *out = h;
    return CILHIP_OK;
  });
}

int cilhip_sparse_info(const cilhip_sparse* m, size_t* n_out, size_t* nnz_out, size_t* longest_row_out) {
  if (!m) return cilhip::st_fail(CILHIP_ERR_INVALID, "sparse_info", "the matrix is NULL");
  if (n_out) *n_out = m->n;
  if (nnz_out) *nnz_out = m->nnz;
  if (longest_row_out) *longest_row_out = m->longest;
  return CILHIP_OK;
}

int cilhip_sparse_get(const cilhip_sparse* m, uint64_t* offsets_out, uint32_t* columns_out, float* values_out, int mem) {
  const char* F = "sparse_get";
  if (!m) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "the matrix is NULL");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return cilhip::st_fail(CILHIP_ERR_INVALID, F, "mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  cilhip::st_clear();
  ST_CK(F, hipSetDevice(m->device));
  const hipMemcpyKind kind = mem == CILHIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (offsets_out) ST_CK(F, hipMemcpy(offsets_out, m->off.get(), (m->n + 1) * sizeof(uint64_t), kind));
  if (columns_out && m->nnz) ST_CK(F, hipMemcpy(columns_out, m->col.get(), m->nnz * sizeof(uint32_t), kind));
  if (values_out && m->nnz) ST_CK(F, hipMemcpy(values_out, m->val.get(), m->nnz * sizeof(float), kind));
  return CILHIP_OK;
}

void cilhip_sparse_destroy(cilhip_sparse* m) { delete m; }

void cilhip_spectral_default_params(cilhip_spectral_params* p) {
  if (!p) return;
  p->max_num_clusters = 2; p->estimate_num_clusters = 0; p->laplacian_type = 2; p->max_outer = 1000; p->degree = 24; p->guard = 3;
}

int cilhip_spectral_embedding(const cilhip_sparse* W, const cilhip_spectral_params* params, float* embedded_out, float* eigenvalues_out, int mem,
                              cilhip_spectral_result* result) {
  const char* F = "spectral_embedding";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!W) return refuse("the matrix is NULL");
  if (!params || !embedded_out || !eigenvalues_out || !result) return refuse("params, embedded_out, eigenvalues_out or result is NULL");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (params->laplacian_type < 0 || params->laplacian_type > 2) return refuse("laplacian_type: 0 (UNNORMALIZED), 1 (NORMALIZED_SYMMETRIC) or 2 (NORMALIZED_RANDOM_WALK)");
  if (params->degree < 2 || params->degree > 512) return refuse("degree must lie in [2, 512]");
  if (params->guard < 1 || params->guard > 15) return refuse("guard must lie in [1, 15]");
  if (params->max_outer == 0) return refuse("max_outer must be positive");
  if (W->n < 3) return refuse("n < 3: there is no spectrum to choose from");
  // S3
  size_t max_clusters = params->max_num_clusters;
  bool estimate = params->estimate_num_clusters != 0;
  if (max_clusters == 0 || max_clusters >= W->n) { max_clusters = 2; estimate = false; }
  if (max_clusters > 16) return cilhip::st_fail(CILHIP_ERR_UNSUPPORTED, F, "max_num_clusters is above 16");
  const size_t nev = estimate ? std::min(max_clusters + 1, W->n - 1) : max_clusters;
  cilhip::st_clear();
  ST_CK(F, hipSetDevice(W->device));
  return sp_guard(F, [&]() -> int { return embedding_impl(W, *params, max_clusters, estimate, nev, embedded_out, eigenvalues_out, mem, result); });
}

int cilhip_kmeans_nd(int device, const float* x, size_t n, size_t dim, int mem, float* centroids, size_t k, size_t max_iter, float tol, uint32_t* labels_out,
                     size_t* iterations_out) {
  const char* F = "kmeans_nd";
  auto refuse = [&](const char* what) { return cilhip::st_fail(CILHIP_ERR_INVALID, F, what); };
  if (!x || !centroids) return refuse("x or centroids is NULL");
  if (n == 0 || n >= SP_MAX_N) return refuse("n must lie in [1, 2^32 - 16)");
  if (dim == 0 || dim > (size_t)ND_MAX_DIM) return refuse("dim must lie in [1, 16]");
  if (k == 0) return refuse("k must be positive");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (k > ND_MAX_K) return cilhip::st_fail(CILHIP_ERR_UNSUPPORTED, F, "k is above 256");
  cilhip::st_clear();
  if (const int open = cilhip::st_open(F, device, CILHIP_ERR_INVALID)) return open;
  return sp_guard(F, [&]() -> int { return kmeans_nd_impl(x, n, (int)dim, mem, centroids, k, max_iter, tol, labels_out, iterations_out); });
}

}  // extern "C"

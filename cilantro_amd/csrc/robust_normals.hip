// robust_normals.hip -- NormalEstimation<float, 3, MinimumCovarianceDeterminant<float, 3>> on the device
// (examples/robust_normal_estimation.cpp of the reference).  Replaces, per point,
//   core/covariance.hpp:185-371             MinimumCovarianceDeterminant: random elemental starts, concentration steps (Mahalanobis ranking, keep
//                                           the h closest, re-estimate), the minimum-determinant choice, the chi-square test on the point itself
//   core/normal_estimation.hpp:294-420      normal / curvature from the chosen covariance; an outlier gets a NaN normal (:300, :381)
// under the contract of DESIGN.md section 15 (restated in numpy by tests/_robust_normal_refs.py; every decision -- the final subset and the
// inlier flag -- is compared bit for bit).  The k-NN lists are the ones cilhip_knn3f returns (knn.hip, stopped before the download); one lane per
// point then runs every trial over its own list.  The row's points and its column of ranking values q live in LDS, laid out [j][thread] like the
// search's KList, because they are indexed at run time; everything else (mean, covariance, adjugate, the best trial) stays in registers.
// Selection is by rank counting: position j is kept iff fewer than h entries order before (q_j, j) -- no sort, no data-dependent stores.
#include "../../include/cilantro_hip/c_api.h"
#include "internal.hpp"
#include "ransac_sampling.hpp"
#include "stateless.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace cilhip {
namespace {

constexpr int MCD_MAX_K = 32;
// dynamic LDS of a block: k * threads * 20 B (three f32 coordinates and one f64 ranking value per list entry).  The block size follows k so that a block
// stays at or below 64 KB -- at least two blocks per CU (160 KB of LDS), and no opt-in beyond the default dynamic limit.
constexpr size_t MCD_LDS_BUDGET = 64 * 1024;
constexpr size_t MCD_ENTRY_BYTES = 3 * sizeof(float) + sizeof(double);
inline int mcd_block_threads(size_t k) { return k * 256 * MCD_ENTRY_BYTES <= MCD_LDS_BUDGET ? 256 : (k * 128 * MCD_ENTRY_BYTES <= MCD_LDS_BUDGET ? 128 : 64); }

struct McdArgs {
  const float* xyz;          // [3n] original order
  const uint32_t* idx;       // [n*k] the lists
  const uint32_t* cnt;       // [n]
  uint32_t n, k;
  int trials, refinements;
  float chi;
  unsigned long long seed;
  unsigned char h_of_m[MCD_MAX_K + 1];   // h for every list length (host: mcd_h)
  float vp[3];
  int use_vp;
  float* normals;            // [3n]
  float* curvature;          // [n] or null
  uint32_t* mask;            // [n] or null
  unsigned char* inlier;     // [n] or null
};

struct Moments { float m0, m1, m2; double c00, c01, c02, c11, c12, c22; };
struct Adjugate { double a00, a01, a02, a11, a12, a22, det; };

// a lane's view of its row in LDS
struct Row {
  double* q;                 // &q[0][tid], stride T
  float *x, *y, *z;          // &x[0][tid] ..., stride T
  uint32_t T;
};

// cov(S): the arithmetic of k_knn's neighbourhood PCA (knn.hip) over the positions in `set`, ascending
__device__ __forceinline__ Moments cov_of(const Row& r, uint32_t m, uint32_t set) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  uint32_t s = 0;
  for (uint32_t j = 0; j < m; ++j)
    if ((set >> j) & 1u) { s0 += (double)r.x[j * r.T]; s1 += (double)r.y[j * r.T]; s2 += (double)r.z[j * r.T]; ++s; }
  Moments o;
  o.m0 = (float)(s0 / (double)s); o.m1 = (float)(s1 / (double)s); o.m2 = (float)(s2 / (double)s);
  double cs0 = 0, cs1 = 0, cs2 = 0, cs3 = 0, cs4 = 0, cs5 = 0;
  for (uint32_t j = 0; j < m; ++j)
    if ((set >> j) & 1u) {
      const float t0 = __fsub_rn(r.x[j * r.T], o.m0), t1 = __fsub_rn(r.y[j * r.T], o.m1), t2 = __fsub_rn(r.z[j * r.T], o.m2);
      cs0 += (double)__fmul_rn(t0, t0); cs1 += (double)__fmul_rn(t0, t1); cs2 += (double)__fmul_rn(t0, t2);
      cs3 += (double)__fmul_rn(t1, t1); cs4 += (double)__fmul_rn(t1, t2); cs5 += (double)__fmul_rn(t2, t2);
    }
  const double inv = (double)s - 1.0;
  o.c00 = cs0 / inv; o.c01 = cs1 / inv; o.c02 = cs2 / inv; o.c11 = cs3 / inv; o.c12 = cs4 / inv; o.c22 = cs5 / inv;
  return o;
}

// adjugate and determinant, one rounding per operation in the order DESIGN.md 15.1 writes them
__device__ __forceinline__ Adjugate adj_of(const Moments& c) {
  Adjugate a;
  a.a00 = __dsub_rn(__dmul_rn(c.c11, c.c22), __dmul_rn(c.c12, c.c12));
  a.a01 = __dsub_rn(__dmul_rn(c.c02, c.c12), __dmul_rn(c.c01, c.c22));
  a.a02 = __dsub_rn(__dmul_rn(c.c01, c.c12), __dmul_rn(c.c02, c.c11));
  a.a11 = __dsub_rn(__dmul_rn(c.c00, c.c22), __dmul_rn(c.c02, c.c02));
  a.a12 = __dsub_rn(__dmul_rn(c.c01, c.c02), __dmul_rn(c.c00, c.c12));
  a.a22 = __dsub_rn(__dmul_rn(c.c00, c.c11), __dmul_rn(c.c01, c.c01));
  a.det = __dadd_rn(__dmul_rn(c.c00, a.a00), __dadd_rn(__dmul_rn(c.c01, a.a01), __dmul_rn(c.c02, a.a02)));
  return a;
}

// q = d^T adj(C) d, d = (double)(P - mean) with the difference in f32: det times the squared Mahalanobis distance, without a division
__device__ __forceinline__ double q_of(const Moments& c, const Adjugate& a, float px, float py, float pz) {
  const double d0 = (double)__fsub_rn(px, c.m0), d1 = (double)__fsub_rn(py, c.m1), d2 = (double)__fsub_rn(pz, c.m2);
  const double r0 = __dadd_rn(__dmul_rn(a.a00, d0), __dadd_rn(__dmul_rn(a.a01, d1), __dmul_rn(a.a02, d2)));
  const double r1 = __dadd_rn(__dmul_rn(a.a01, d0), __dadd_rn(__dmul_rn(a.a11, d1), __dmul_rn(a.a12, d2)));
  const double r2 = __dadd_rn(__dmul_rn(a.a02, d0), __dadd_rn(__dmul_rn(a.a12, d1), __dmul_rn(a.a22, d2)));
  return __dadd_rn(__dmul_rn(d0, r0), __dadd_rn(__dmul_rn(d1, r1), __dmul_rn(d2, r2)));
}

// select(h) under (c, a): the h entries that order first by (q, position); a NaN q ranks as +inf
__device__ __forceinline__ uint32_t select_h(const Row& r, uint32_t m, uint32_t h, const Moments& c, const Adjugate& a) {
  for (uint32_t j = 0; j < m; ++j) {
    const double q = q_of(c, a, r.x[j * r.T], r.y[j * r.T], r.z[j * r.T]);
    r.q[j * r.T] = q != q ? (double)INFINITY : q;
  }
  uint32_t set = 0;
  for (uint32_t j = 0; j < m; ++j) {
    const double qj = r.q[j * r.T];
    uint32_t before = 0;
    for (uint32_t l = 0; l < m; ++l) {
      const double ql = r.q[l * r.T];
      before += (ql < qj || (ql == qj && l < j)) ? 1u : 0u;
    }
    set |= (before < h ? 1u : 0u) << j;
  }
  return set;
}

__global__ __launch_bounds__(256) void k_robust_normals(McdArgs a) {
  extern __shared__ double mcd_lds[];      // q[k][T], then x[k][T], y[k][T], z[k][T]
  const uint32_t T = blockDim.x;
  const size_t i64 = (size_t)blockIdx.x * T + threadIdx.x;
  if (i64 >= a.n) return;
  const uint32_t i = (uint32_t)i64;
  Row r;
  r.T = T;
  r.q = mcd_lds + threadIdx.x;
  float* f = reinterpret_cast<float*>(mcd_lds + (size_t)a.k * T);
  r.x = f + threadIdx.x; r.y = f + (size_t)a.k * T + threadIdx.x; r.z = f + 2 * (size_t)a.k * T + threadIdx.x;

  const uint32_t m = min(a.cnt[i], a.k);
  for (uint32_t j = 0; j < m; ++j) {
    const size_t id = min((size_t)a.idx[(size_t)i * a.k + j], (size_t)a.n - 1);
    r.x[j * T] = a.xyz[3 * id]; r.y[j * T] = a.xyz[3 * id + 1]; r.z[j * T] = a.xyz[3 * id + 2];
  }
  float n0 = NAN, n1 = NAN, n2 = NAN, curv = NAN;
  uint32_t final_set = 0;
  bool inlier = false;
  if (m >= 3) {
    const uint32_t all = m == 32 ? 0xFFFFFFFFu : ((1u << m) - 1u);
    const uint32_t h = a.h_of_m[m];
    Moments best;
    bool have = false;
    if (m == 3 || h >= m) {      // covariance.hpp:204, :349-352: the plain covariance of the whole list
      best = cov_of(r, m, all);
      final_set = all;
      have = true;
    } else {
      double best_det = (double)INFINITY;
      for (int t = 0; t < a.trials; ++t) {
        uint32_t pick[3];
        draw_samples(a.seed ^ (((unsigned long long)i << 8) | (unsigned long long)t), m, 3, 1, pick);
        uint32_t set = (1u << pick[0]) | (1u << pick[1]) | (1u << pick[2]);
        Moments c = cov_of(r, m, set);
        for (int l = 0; l < a.refinements; ++l) {
          set = select_h(r, m, h, c, adj_of(c));
          c = cov_of(r, m, set);
        }
        const double det = adj_of(c).det;
        if (det < best_det) { best = c; best_det = det; final_set = set; have = true; }      // (NaN and +inf never win)
      }
    }
    if (have) {
      const Adjugate fa = adj_of(best);
      inlier = a.chi <= 0.0f || q_of(best, fa, r.x[0], r.y[0], r.z[0]) <= __dmul_rn((double)a.chi, fa.det);
      if (inlier) {
        const double C[9] = {best.c00, best.c01, best.c02, best.c01, best.c11, best.c12, best.c02, best.c12, best.c22};
        double w[3], V[9];
        sym_eig3(C, w, V);   // as k_knn: descending; the normal is the eigenvector of the smallest eigenvalue
        n0 = (float)V[2]; n1 = (float)V[5]; n2 = (float)V[8];
        if (a.use_vp) {
          const float qx = a.xyz[3 * (size_t)i], qy = a.xyz[3 * (size_t)i + 1], qz = a.xyz[3 * (size_t)i + 2];
          const float d = __fadd_rn(__fmul_rn(n0, __fsub_rn(a.vp[0], qx)), __fadd_rn(__fmul_rn(n1, __fsub_rn(a.vp[1], qy)), __fmul_rn(n2, __fsub_rn(a.vp[2], qz))));
          if (d < 0.0f) { n0 = -n0; n1 = -n1; n2 = -n2; }
        }
        curv = (float)(w[2] / ((w[0] + w[1]) + w[2]));
      }
    } else {
      final_set = 0;
    }
  }
  a.normals[3 * (size_t)i] = n0; a.normals[3 * (size_t)i + 1] = n1; a.normals[3 * (size_t)i + 2] = n2;
  if (a.curvature) a.curvature[i] = curv;
  if (a.mask) a.mask[i] = final_set;
  if (a.inlier) a.inlier[i] = inlier ? 1 : 0;
}

// h = min(max(3, llround(ratio * m)), m) with the product in f32 (covariance.hpp:317-319); a product at or above m needs no rounding
unsigned char mcd_h(float ratio, uint32_t m) {
  const float hf = ratio * (float)m;
  if (hf >= (float)m) return (unsigned char)m;
  const long long h = std::max(3ll, std::llround(hf));
  return (unsigned char)std::min<long long>(h, (long long)m);
}

int mcd_refuse(const char* why) { return st_fail(CILHIP_ERR_INVALID, "robust_normals", why); }

}  // namespace
}  // namespace cilhip

extern "C" void cilhip_mcd_params_default(cilhip_mcd_params* p) {
  if (!p) return;
  *p = cilhip_mcd_params{};
  p->max_sq_dist = INFINITY;
  p->num_trials = 6;             // covariance.hpp:365-369
  p->num_refinements = 3;
  p->inlier_ratio = 0.75f;
  p->chi_square_threshold = -1.0f;
}

extern "C" int cilhip_robust_normals_knn3f(int device, const float* xyz, size_t n, int mem, const cilhip_mcd_params* p, const float* view_point, float* normals_out,
                                           float* curvature_or_null, uint32_t* subset_mask_or_null, uint8_t* inlier_or_null) {
  using namespace cilhip;
  if (!p) return mcd_refuse("params is null");
  if (n && !xyz) return mcd_refuse("xyz is null");
  if (!normals_out) return mcd_refuse("normals_out is null");
  if (p->k < 1 || p->k > (size_t)MCD_MAX_K) return mcd_refuse("k must be in 1..32");
  if (p->num_trials < 1 || p->num_trials > 64) return mcd_refuse("num_trials must be in 1..64");
  if (p->num_refinements < 0 || p->num_refinements > 16) return mcd_refuse("num_refinements must be in 0..16");
  if (!(std::isfinite(p->inlier_ratio) && p->inlier_ratio > 0.0f)) return mcd_refuse("inlier_ratio must be finite and positive");
  if (std::isnan(p->chi_square_threshold)) return mcd_refuse("chi_square_threshold is NaN");
  if ((unsigned long long)n >= 0xFFFFFFF0ull) return mcd_refuse("n must be below 2^32 - 16");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return mcd_refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  const cilhip_mcd_params prm = *p;
  const KnnListsConsumer consume = [&](const KnnDeviceLists& L) -> int {
    McdArgs a{};
    a.xyz = L.xyz; a.idx = L.idx; a.cnt = L.cnt; a.n = (uint32_t)L.n; a.k = (uint32_t)L.k;
    a.trials = prm.num_trials; a.refinements = prm.num_refinements; a.chi = prm.chi_square_threshold; a.seed = prm.seed;
    for (uint32_t m = 0; m <= (uint32_t)MCD_MAX_K; ++m) a.h_of_m[m] = mcd_h(prm.inlier_ratio, m);
    if (view_point && std::isfinite(view_point[0]) && std::isfinite(view_point[1]) && std::isfinite(view_point[2])) {
      a.use_vp = 1;
      for (int c = 0; c < 3; ++c) a.vp[c] = view_point[c];
    }
    const bool host = mem == CILHIP_MEM_HOST;
    a.normals = normals_out; a.curvature = curvature_or_null; a.mask = subset_mask_or_null; a.inlier = inlier_or_null;
    if (host) {
      ST_CK("robust_normals", L.pool->get(&a.normals, 3 * L.n));
      if (curvature_or_null) ST_CK("robust_normals", L.pool->get(&a.curvature, L.n));
      if (subset_mask_or_null) ST_CK("robust_normals", L.pool->get(&a.mask, L.n));
      if (inlier_or_null) ST_CK("robust_normals", L.pool->get(&a.inlier, L.n));
    }
    const int threads = mcd_block_threads(L.k);
    const size_t lds = L.k * (size_t)threads * MCD_ENTRY_BYTES;
    hipLaunchKernelGGL(k_robust_normals, dim3((unsigned)((L.n + threads - 1) / threads)), dim3(threads), lds, L.s, a);
    ST_CK("robust_normals", hipGetLastError());
    if (host) {
      ST_CK("robust_normals", hipMemcpyAsync(normals_out, a.normals, 3 * L.n * sizeof(float), hipMemcpyDeviceToHost, L.s));
      if (curvature_or_null) ST_CK("robust_normals", hipMemcpyAsync(curvature_or_null, a.curvature, L.n * sizeof(float), hipMemcpyDeviceToHost, L.s));
      if (subset_mask_or_null) ST_CK("robust_normals", hipMemcpyAsync(subset_mask_or_null, a.mask, L.n * sizeof(uint32_t), hipMemcpyDeviceToHost, L.s));
      if (inlier_or_null) ST_CK("robust_normals", hipMemcpyAsync(inlier_or_null, a.inlier, L.n * sizeof(uint8_t), hipMemcpyDeviceToHost, L.s));
    }
    ST_CK("robust_normals", hipStreamSynchronize(L.s));
    return CILHIP_OK;
  };
  try {
    return knn_self_lists_on_device(device, xyz, n, mem, prm.k, prm.max_sq_dist, consume);
  } catch (...) {      // (out of host memory: never across the C boundary)
    return st_fail(CILHIP_ERR_HIP, "robust_normals", "out of host memory");
  }
}

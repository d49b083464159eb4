// knn_nd.hip -- exact k-NN, k-NN-in-radius and radius search over n x dim float points, 1 <= dim <= 16.  Replaces
//   core/kd_tree.hpp:144-406      KDTree<float, EigenDim, KDTreeDistanceAdaptors::L2> for EigenDim != 3 (KDTree2f, KDTreeXf): kNNSearch,
//                                 kNNInRadiusSearch, radiusSearch, nearestNeighborSearch
//   nanoflann.hpp:570-604         L2_Adaptor::evalMetric, the distance all of them order by
//
// Exhaustive: a cell grid does not survive 9 or 16 dimensions.  One query per lane, its DIM coordinates in registers, its k best
// candidates in the KList column of knn_lists.hpp.  The reference points stream past in ascending index, KNN_ND_TILE at a time, the same
// ones for every lane of the block: their addresses are wave-uniform, so the loads are scalar loads and the coordinates reach the vector
// ALU as scalar operands -- no LDS traffic beside the list insertions.  Those are rare for a lane and frequent for a wave (it pays whenever
// any of its 64 lanes inserts), so the list is kept unordered while the stream runs -- an entry overwrites the largest key and one pass of
// independent LDS reads finds the new largest -- and sorted once at the end.  When the queries alone do not fill the device the stream is cut
// into slices that run side by side (blockIdx.y), and k_merge_nd picks each query's k smallest keys from its slices' lists.
// N1  d2 is evalMetric in f32, every operation rounded, nothing contracted: r = 0; per full group of four coordinates
//     r = r + (((s0 + s1) + s2) + s3); then r = r + s for each coordinate left over (s_i = (q_i - p_i)^2).  dim = 3: knn.hip's d2_pinned.
// N2  a candidate enters iff bits(d2) < bits(bound) as unsigned words (bound > 0): d2 < bound, and false for +inf and for NaN.
// N3  lists ascend by (d2, index).  A slice's stream ascends by index, so a candidate at exactly the list's largest distance never enters:
//     among equal distances the lowest indices stay; the merge compares whole keys.  (cilhip_knn3f under tie rule 0;
//     cilhip_knn_set_tie_rule does not apply.)
// N6  no atomics: two runs agree bit for bit.
#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "internal.hpp"
#include "knn_lists.hpp"
#include "knn_nd_host.hpp"
#include "nd_device.hpp"
#include "stateless.hpp"

#include <hip/hip_runtime.h>

#include <cmath>

namespace cilhip {
namespace {

constexpr int KNN_ND_TILE = 4;      // candidates loaded and evaluated together (4 x 16 coordinates: 64 scalar registers)

__device__ __forceinline__ unsigned long long nd_key(float d2, uint32_t j) { return ((unsigned long long)__float_as_uint(d2) << 32) | j; }

__device__ __forceinline__ void nd_list_init(KList& L, unsigned long long* lists, uint32_t k, float bound) {
  L.col = lists + threadIdx.x;
  L.k = k; L.cnt = 0; L.wpos = 0;
  L.none_key = (unsigned long long)__float_as_uint(bound) << 32;
  L.worst = L.none_key;
  L.tie_bits = 0xFFFFFFFFu;
}
// rows by query: out_idx [nq * k] NONE-padded, out_d2 [nq * k] +inf-padded or null, out_cnt [nq] or null; L sorted
__device__ __forceinline__ void nd_write_rows(const KList& L, uint32_t qi, uint32_t k, uint32_t* __restrict__ out_idx, float* __restrict__ out_d2, uint32_t* __restrict__ out_cnt) {
  const uint32_t m = L.cnt;
  if (out_cnt) out_cnt[qi] = m;
  for (uint32_t s = 0; s < k; ++s) {
    const unsigned long long key = s < m ? L.col[(size_t)s * KNN_THREADS] : 0ull;
    out_idx[(size_t)qi * k + s] = s < m ? (uint32_t)key : NONE_U32;
    if (out_d2) out_d2[(size_t)qi * k + s] = s < m ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
  }
}
constexpr unsigned long long ND_NO_KEY = 0xFFFFFFFFFFFFFFFFull;      // pads a slice's list: behind every key

// Candidates that passed the test against the list's largest distance wait here, in registers, newest first, until some lane of the wave
// has fewer than KNN_ND_TILE free places; then every lane enters what it holds.  The wave pays for list entries once per flush, not
// once per tile in which one of its lanes found something.  The test a candidate passed may be stale by then: flush() compares whole keys.
constexpr int KNN_ND_STAGE = 8;
struct NdStage {
  unsigned long long s[KNN_ND_STAGE];
  uint32_t n;
  __device__ __forceinline__ void push(unsigned long long key) {
#pragma unroll
    for (int i = KNN_ND_STAGE - 1; i > 0; --i) s[i] = s[i - 1];
    s[0] = key;
    ++n;
  }
  __device__ __forceinline__ bool crowded() const { return n > (uint32_t)(KNN_ND_STAGE - KNN_ND_TILE); }
  __device__ __forceinline__ void flush(KList& L) {
#pragma unroll
    for (int i = KNN_ND_STAGE - 1; i >= 0; --i)      // oldest first
      if ((uint32_t)i < n && s[i] < L.worst) L.put(s[i]);
    n = 0;
  }
};

// ref [n_ref * DIM], qry [nq * DIM] point-major; bound > 0 (+inf: plain k-NN).  Block (x, y): the queries 256 x .. 256 x + 255 against the
// reference points [y * slice, (y + 1) * slice) (slice: a multiple of KNN_ND_TILE).  One slice (part == null): the rows are written.  Several:
// part[(y * k + s) * nq + query] = the slice's s-th best key, ND_NO_KEY behind the last; k_merge_nd makes the rows.
// Dynamic LDS: k * KNN_THREADS keys.
template <int DIM>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_nd(const float* __restrict__ ref, uint32_t n_ref, uint32_t slice, const float* __restrict__ qry, uint32_t nq, uint32_t k,
                                                        float bound, unsigned long long* __restrict__ part, uint32_t* __restrict__ out_idx, float* __restrict__ out_d2,
                                                        uint32_t* __restrict__ out_cnt) {
  extern __shared__ unsigned long long lists[];   // [k][KNN_THREADS]
  const uint32_t qi = blockIdx.x * KNN_THREADS + threadIdx.x;
  if (qi >= nq) return;
  NdQuery<DIM> q;
  q.load(qry + (size_t)qi * DIM);
  KList L;
  nd_list_init(L, lists, k, bound);
  NdStage st;
  st.n = 0;
  uint32_t worst_hi = __float_as_uint(bound);      // N2 / N3: a candidate enters iff bits(d2) < worst_hi
  const unsigned long long first = (unsigned long long)blockIdx.y * slice;
  const uint32_t end = (uint32_t)min(first + slice, (unsigned long long)n_ref);
  uint32_t j = (uint32_t)min(first, (unsigned long long)n_ref);
  for (; j + KNN_ND_TILE <= end; j += KNN_ND_TILE) {
    const float* __restrict__ p = ref + (size_t)j * DIM;
    float d[KNN_ND_TILE];
    uint32_t best = 0xFFFFFFFFu;
#pragma unroll
    for (int t = 0; t < KNN_ND_TILE; ++t) { d[t] = q.d2(p + t * DIM); best = min(best, __float_as_uint(d[t])); }
    if (best < worst_hi) {      // (rare for a lane once its list has filled)
#pragma unroll
      for (int t = 0; t < KNN_ND_TILE; ++t)
        if (__float_as_uint(d[t]) < worst_hi) st.push(nd_key(d[t], j + t));
    }
    // (outside the branch: the whole wave flushes together, so the next flush is a whole stage away for every lane)
    if (__any(st.crowded())) { st.flush(L); worst_hi = (uint32_t)(L.worst >> 32); }
  }
  for (; j < end; ++j) {      // (fewer than KNN_ND_TILE points: they fit behind a stage that is not crowded)
    const float dj = q.d2(ref + (size_t)j * DIM);
    if (__float_as_uint(dj) < worst_hi) st.push(nd_key(dj, j));
  }
  st.flush(L);
  L.sort();
  if (part == nullptr) { nd_write_rows(L, qi, k, out_idx, out_d2, out_cnt); return; }
  for (uint32_t s = 0; s < k; ++s) part[((size_t)blockIdx.y * k + s) * nq + qi] = s < L.cnt ? L.col[(size_t)s * KNN_THREADS] : ND_NO_KEY;
}

// the k smallest keys of a query's `slices` sorted lists (keys are unique: no two carry one index) -> its rows
__global__ __launch_bounds__(KNN_THREADS) void k_merge_nd(const unsigned long long* __restrict__ part, uint32_t slices, uint32_t nq, uint32_t k, float bound,
                                                          uint32_t* __restrict__ out_idx, float* __restrict__ out_d2, uint32_t* __restrict__ out_cnt) {
  extern __shared__ unsigned long long lists[];   // [k][KNN_THREADS]
  const uint32_t qi = blockIdx.x * KNN_THREADS + threadIdx.x;
  if (qi >= nq) return;
  KList L;
  nd_list_init(L, lists, k, bound);
  for (uint32_t y = 0; y < slices; ++y)
    for (uint32_t s = 0; s < k; ++s) {
      const unsigned long long key = part[((size_t)y * k + s) * nq + qi];
      if (key >= L.worst) break;      // (ascending: nothing further in this list enters either)
      L.put(key);
    }
  L.sort();
  nd_write_rows(L, qi, k, out_idx, out_d2, out_cnt);
}

// Block (x, y) as in k_knn_nd; entry e = query * gridDim.y + y.  FILL = false: counts[e] = the query's neighbours in slice y; FILL = true:
// keys[offsets[e] + i] = the i-th one met.  With the entries query-major, one exclusive sum gives every slice of every list its place, and
// a query's slices lie one behind the other: its list.  radius_sq > 0, finite
template <int DIM, bool FILL>
__global__ __launch_bounds__(KNN_THREADS) void k_radius_nd(const float* __restrict__ ref, uint32_t n_ref, uint32_t slice, const float* __restrict__ qry, uint32_t nq,
                                                           float radius_sq, unsigned long long* __restrict__ counts_or_offsets, unsigned long long* __restrict__ keys) {
  const uint32_t qi = blockIdx.x * KNN_THREADS + threadIdx.x;
  if (qi >= nq) return;
  NdQuery<DIM> q;
  q.load(qry + (size_t)qi * DIM);
  const uint32_t rbits = __float_as_uint(radius_sq);
  const size_t e = (size_t)qi * gridDim.y + blockIdx.y;
  const unsigned long long base = FILL ? counts_or_offsets[e] : 0ull;
  unsigned long long cnt = 0;
  const unsigned long long first = (unsigned long long)blockIdx.y * slice;
  const uint32_t end = (uint32_t)min(first + slice, (unsigned long long)n_ref);
  uint32_t j = (uint32_t)min(first, (unsigned long long)n_ref);
  for (; j + KNN_ND_TILE <= end; j += KNN_ND_TILE) {
    const float* __restrict__ p = ref + (size_t)j * DIM;
    float d[KNN_ND_TILE];
#pragma unroll
    for (int t = 0; t < KNN_ND_TILE; ++t) d[t] = q.d2(p + t * DIM);
#pragma unroll
    for (int t = 0; t < KNN_ND_TILE; ++t)
      if (__float_as_uint(d[t]) < rbits) {
        if (FILL) keys[base + cnt] = nd_key(d[t], j + t);
        ++cnt;
      }
  }
  for (; j < end; ++j) {
    const float dj = q.d2(ref + (size_t)j * DIM);
    if (__float_as_uint(dj) < rbits) {
      if (FILL) keys[base + cnt] = nd_key(dj, j);
      ++cnt;
    }
  }
  if (!FILL) counts_or_offsets[e] = cnt;
}
// offsets[i] = where query i's list begins = its first slice's place (i = nq: the total)
__global__ void k_list_offsets(const unsigned long long* __restrict__ slice_offsets, uint32_t slices, uint32_t n, unsigned long long* __restrict__ offsets) {
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) offsets[i] = slice_offsets[(size_t)i * slices];
}

inline unsigned nd_blocks(size_t nq) { return (unsigned)((nq + KNN_THREADS - 1) / KNN_THREADS); }      // (nq < 2^32: below 2^24 blocks)

template <int DIM>
void launch_knn_nd(hipStream_t s, const float* ref, size_t n_ref, size_t slices, size_t slice, const float* qry, size_t nq, size_t k, float bound, unsigned long long* part,
                   uint32_t* idx, float* d2, uint32_t* cnt) {
  hipLaunchKernelGGL(k_knn_nd<DIM>, dim3(nd_blocks(nq), (unsigned)slices), dim3(KNN_THREADS), k * KNN_THREADS * sizeof(unsigned long long), s, ref, (uint32_t)n_ref,
                     (uint32_t)slice, qry, (uint32_t)nq, (uint32_t)k, bound, part, idx, d2, cnt);
}
template <int DIM, bool FILL>
void launch_radius_nd(hipStream_t s, const float* ref, size_t n_ref, size_t slices, size_t slice, const float* qry, size_t nq, float radius_sq, unsigned long long* cnt,
                      unsigned long long* keys) {
  hipLaunchKernelGGL((k_radius_nd<DIM, FILL>), dim3(nd_blocks(nq), (unsigned)slices), dim3(KNN_THREADS), 0, s, ref, (uint32_t)n_ref, (uint32_t)slice, qry, (uint32_t)nq,
                     radius_sq, cnt, keys);
}

int knn_nd_impl(int device, const float* ref, size_t n_ref, const float* query, size_t n_query, size_t dim, int mem, size_t k, float max_sq_dist, uint32_t* idx_out,
                float* d2_out, uint32_t* counts_out) {
  const bool self = query == nullptr;
  if (self) n_query = n_ref;
  const NdVerdict v = nd_check_knn(ref, n_ref, n_query, dim, mem, k, max_sq_dist, idx_out);
  if (v.status) return st_fail(v.status, "knn_nd", v.what);
  st_clear();
  if (nd_knn_trivial(n_ref, n_query, max_sq_dist)) { nd_pad_rows(n_query, k, idx_out, d2_out, counts_out); return CILHIP_OK; }
  DevPool pool;
  float *d_ref = nullptr, *d_q = nullptr, *d_d2 = nullptr;
  uint32_t *d_idx = nullptr, *d_cnt = nullptr;
  unsigned long long* d_part = nullptr;
  StreamGuard s;      // (declared last: drained and destroyed before anything is freed)
  if (const int open = st_open("knn_nd", device)) return open;
  ST_CK("knn_nd", s.create());
  ST_CK("knn_nd", st_stage(pool, s, mem, ref, dim * n_ref, &d_ref));
  if (self) d_q = d_ref;
  else ST_CK("knn_nd", st_stage(pool, s, mem, query, dim * n_query, &d_q));
  ST_CK("knn_nd", pool.get(&d_idx, n_query * k));
  if (d2_out) ST_CK("knn_nd", pool.get(&d_d2, n_query * k));
  if (counts_out) ST_CK("knn_nd", pool.get(&d_cnt, n_query));
  // few queries: slices of the reference stream side by side, merged afterwards (knn_nd_host.hpp)
  const size_t slices = nd_slices(n_ref, n_query, k), slice = nd_slice_length(n_ref, slices, KNN_ND_TILE);
  if (slices > 1) ST_CK("knn_nd", pool.get(&d_part, slices * k * n_query));
#define ND_KNN(D) launch_knn_nd<D>(s, d_ref, n_ref, slices, slice, d_q, n_query, k, max_sq_dist, d_part, d_idx, d_d2, d_cnt)
  ND_DISPATCH(dim, ND_KNN)
#undef ND_KNN
  ST_CK("knn_nd", hipGetLastError());
  if (slices > 1) {
    hipLaunchKernelGGL(k_merge_nd, dim3(nd_blocks(n_query)), dim3(KNN_THREADS), k * KNN_THREADS * sizeof(unsigned long long), s, (const unsigned long long*)d_part,
                       (uint32_t)slices, (uint32_t)n_query, (uint32_t)k, max_sq_dist, d_idx, d_d2, d_cnt);
    ST_CK("knn_nd", hipGetLastError());
  }
  ST_CK("knn_nd", hipMemcpyAsync(idx_out, d_idx, n_query * k * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (d2_out) ST_CK("knn_nd", hipMemcpyAsync(d2_out, d_d2, n_query * k * sizeof(float), hipMemcpyDeviceToHost, s));
  if (counts_out) ST_CK("knn_nd", hipMemcpyAsync(counts_out, d_cnt, n_query * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ST_CK("knn_nd", hipStreamSynchronize(s));
  return CILHIP_OK;
}

// count -> exclusive sum -> fill of packed keys -> one segmented radix sort -> unpack: the stages of radius_impl (knn.hip), the last two shared
int radius_nd_impl(int device, const float* ref, size_t n_ref, const float* query, size_t n_query, size_t dim, int mem, float radius_sq, uint64_t* offsets_out,
                   uint32_t* idx_out, float* d2_out, size_t capacity, size_t* total_out) {
  const bool self = query == nullptr;
  if (self) n_query = n_ref;
  const NdVerdict v = nd_check_radius(ref, n_ref, n_query, dim, mem, radius_sq, offsets_out);
  if (v.status) return st_fail(v.status, "radius_search_nd", v.what);
  st_clear();
  if (nd_radius_trivial(n_ref, n_query, radius_sq)) { nd_empty_offsets(n_query, offsets_out, total_out); return CILHIP_OK; }
  if (total_out) *total_out = 0;
  DevPool pool;
  float *d_ref = nullptr, *d_q = nullptr;
  unsigned long long *d_cnt = nullptr, *d_off = nullptr, *d_keys = nullptr;
  StreamGuard s;      // (declared last: drained and destroyed before anything is freed)
  if (const int open = st_open("radius_search_nd", device)) return open;
  ST_CK("radius_search_nd", s.create());
  ST_CK("radius_search_nd", st_stage(pool, s, mem, ref, dim * n_ref, &d_ref));
  if (self) d_q = d_ref;
  else ST_CK("radius_search_nd", st_stage(pool, s, mem, query, dim * n_query, &d_q));
  const size_t slices = nd_slices(n_ref, n_query, 1), slice = nd_slice_length(n_ref, slices, KNN_ND_TILE), entries = n_query * slices;
  ST_CK("radius_search_nd", pool.get(&d_cnt, entries + 1));
  ST_CK("radius_search_nd", hipMemsetAsync(d_cnt, 0, (entries + 1) * sizeof(unsigned long long), s));
#define ND_COUNT(D) launch_radius_nd<D, false>(s, d_ref, n_ref, slices, slice, d_q, n_query, radius_sq, d_cnt, nullptr)
  ND_DISPATCH(dim, ND_COUNT)
#undef ND_COUNT
  ST_CK("radius_search_nd", hipGetLastError());
  {  // counts -> offsets (exclusive scan over entries + 1 words: the last one is the total), in place
    const auto scan = prim_exclusive_sum(d_cnt, d_cnt, entries + 1, s);
    size_t tmp_bytes = 0;
    ST_CK("radius_search_nd", scan(nullptr, tmp_bytes));
    DevBuf<unsigned char> d_tmp;
    ST_CK("radius_search_nd", d_tmp.alloc(tmp_bytes));
    ST_CK("radius_search_nd", scan(d_tmp.get(), tmp_bytes));
    d_off = d_cnt;
    if (slices > 1) {
      ST_CK("radius_search_nd", pool.get(&d_off, n_query + 1));
      hipLaunchKernelGGL(k_list_offsets, dim3(prim_blocks(n_query + 1)), dim3(PRIM_THREADS), 0, s, (const unsigned long long*)d_cnt, (uint32_t)slices, (uint32_t)(n_query + 1), d_off);
      ST_CK("radius_search_nd", hipGetLastError());
    }
    ST_CK("radius_search_nd", hipMemcpyAsync(offsets_out, d_off, (n_query + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    ST_CK("radius_search_nd", hipStreamSynchronize(s));      // (before the scan's temporary goes)
  }
  const size_t total = (size_t)offsets_out[n_query];
  if (total_out) *total_out = total;
  const int plan = nd_radius_plan(idx_out, capacity, total);
  if (plan < 0) return st_fail(CILHIP_ERR_UNSUPPORTED, "radius_search_nd", "the lists hold more than 2^32 - 16 entries together");   // one segmented sort call takes 32-bit sizes
  if (plan == 0) return CILHIP_OK;
  ST_CK("radius_search_nd", pool.get(&d_keys, total));
#define ND_FILL(D) launch_radius_nd<D, true>(s, d_ref, n_ref, slices, slice, d_q, n_query, radius_sq, d_cnt, d_keys)
  ND_DISPATCH(dim, ND_FILL)
#undef ND_FILL
  ST_CK("radius_search_nd", hipGetLastError());
  return radius_sort_unpack("radius_search_nd", pool, s, d_off, n_query, total, d_keys, idx_out, d2_out);
}

}  // namespace
}  // namespace cilhip

extern "C" {

int cilhip_knn_nd(int device, const float* ref, size_t n_ref, const float* query_or_null, size_t n_query, size_t dim, int mem, size_t k, float max_sq_dist,
                  uint32_t* idx_out, float* d2_out, uint32_t* counts_out) {
  return cilhip::knn_nd_impl(device, ref, n_ref, query_or_null, n_query, dim, mem, k, max_sq_dist, idx_out, d2_out, counts_out);
}

int cilhip_radius_search_nd(int device, const float* ref, size_t n_ref, const float* query_or_null, size_t n_query, size_t dim, int mem, float radius_sq,
                            uint64_t* offsets_out, uint32_t* idx_out, float* d2_out, size_t capacity, size_t* total_out_or_null) {
  return cilhip::radius_nd_impl(device, ref, n_ref, query_or_null, n_query, dim, mem, radius_sq, offsets_out, idx_out, d2_out, capacity, total_out_or_null);
}

}  // extern "C"

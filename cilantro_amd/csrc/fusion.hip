// fusion.hip -- the map step of cilantro's examples/fusion.cpp (:147-236) on device-resident arrays: a surfel model (points, normals,
// colours, one confidence per point) takes in one registered frame; and cleanup_callback (:51-59).
//
// The contract (DESIGN.md section 16 has it in full, rule by rule; tests/_fusion_refs.py restates it in numpy, bit for bit):
//   F1  model map = index map of the model under extrinsics cam_pose (c = to_cam p, nc = linear(to_cam) n); frame map: no extrinsics
//   F2  interior pixels in ascending k = y w + x; an empty frame entry does nothing                                  :172-180
//   F3  fz, mz = c_m.z, rw = pinned_expf(radial_factor * (dx dx + dy dy)), ang(v) = (float)acos((double)clamp(v))    :182-186
//   F4  fuse / append / remove / untouched, the first that holds                                                    :188-226
//   F5  g = rw / (rw + conf), gc = 1 - g; gc old + g new; normalized normal; conf += g                              :194-203
//   F6  remove(): the k-th smallest hole below n' takes the k-th largest surviving row of [n', n)       point_cloud.hpp:154-198
//   F7  appended rows in ascending pixel order, conf = rw                                                           :229-235
//   F9  remove_unstable: S = {i : conf[i] < thresh}                                                                 :51-59
//
// The kernels (one block per 256 consecutive pixels or rows; ballot / popcount per wave, as k_ic_unproject):
//   k_ic_splat<IC_INDEX>  (image_device.hpp) twice: the model under to_cam and the frame onto two 64-bit key images
//   k_fu_decide    one lane per pixel: the decision byte of the pixel and, per block, the four populations
//   (one rocPRIM exclusive scan of the per-block populations; its last element is what the host reads: counts and capacity)
//   k_fu_fuse      decision FUSE: the model row in place; decision REMOVE: the row's index into S at the block's offset plus its rank
//   k_fu_tail / k_fu_move  F6 over the sorted S: which rows of the tail [n', n) leave, how many above each (one scan), one lane per tail row moves a survivor
//   k_fu_append    decision APPEND: the new row at n' + the block's offset + its rank
//   k_fu_unstable<COUNT>   F9: per block the rows below the threshold, then their indices (ascending: no sort)
// Every decision is in scratch before the first model row changes.  No floating-point atomics: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "image_device.hpp"
#include "internal.hpp"
#include "search_device.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

enum : unsigned char { FU_NONE = 0, FU_FUSE = 1, FU_APPEND = 2, FU_REMOVE = 3, FU_UNTOUCHED = 4 };

struct FuCount { uint32_t fused, appended, removed, untouched; };
struct FuPlus {
  __host__ __device__ FuCount operator()(const FuCount& a, const FuCount& b) const { return FuCount{a.fused + b.fused, a.appended + b.appended, a.removed + b.removed, a.untouched + b.untouched}; }
};

struct FuModel { F3 *xyz, *nrm, *rgb; float* conf; };

struct FuArgs {
  FuModel model;
  uint32_t n_model;
  const F3 *fxyz, *fnrm, *frgb;
  uint32_t n_frame;
  const unsigned long long *keys_m, *keys_f;      // [w * h]
  uint32_t w, h, npix;
  IcRigid to_cam, pose;
  float k02, k12;
  float fusion_dist, occlusion_dist, radial_factor;
  double t_fuse, t_append, t_free;                // T(deg) = ((double)deg * M_PI) / 180.0
  unsigned char* decision;                        // [w * h]
  FuCount* block_counts;                          // k_fu_decide: [blocks]; afterwards their exclusive scan
  uint32_t* removed_idx;                          // S in pixel order
  uint32_t n_after_remove;                        // n'
};

// F3: ang(v) = (float)acos((double)min(1.0f, max(-1.0f, v))), std::min / std::max as written (NaN -> -1), widened for the comparison
__device__ __forceinline__ double fu_ang(float v) {
  const float lo = -1.0f < v ? v : -1.0f;      // std::max(-1.0f, v)
  const float c = lo < 1.0f ? lo : 1.0f;       // std::min(1.0f, .)
  return (double)(float)acos((double)c);
}
__device__ __forceinline__ float fu_radial(const FuArgs& a, uint32_t x, uint32_t y) {
  const float dx = __fsub_rn((float)x, a.k02), dy = __fsub_rn((float)y, a.k12);
  return pinned_expf(__fmul_rn(a.radial_factor, __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy))));
}
__device__ __forceinline__ bool fu_interior(const FuArgs& a, size_t k, uint32_t* x, uint32_t* y) {
  if (k >= a.npix || a.w < 3 || a.h < 3) return false;
  *y = (uint32_t)(k / a.w); *x = (uint32_t)(k - (size_t)*y * a.w);
  return *x >= 1 && *y >= 1 && *x + 2 <= a.w && *y + 2 <= a.h;
}

// F2-F4 for pixel k
__device__ __forceinline__ unsigned char fu_decision(const FuArgs& a, size_t k) {
  uint32_t x, y;
  if (!fu_interior(a, k, &x, &y)) return FU_NONE;
  const unsigned long long fkey = a.keys_f[k];
  if (fkey == IC_EMPTY) return FU_NONE;                      // :177
  const uint32_t f = (uint32_t)fkey;
  if (f >= a.n_frame) return FU_NONE;                        // (a map entry is < n_frame by construction)
  const unsigned long long mkey = a.keys_m[k];
  const bool has_m = mkey != IC_EMPTY && (uint32_t)mkey < a.n_model;
  if (!has_m) {                                              // :204-206 (interior: the four neighbours are inside the image)
    const bool alone = a.keys_m[k - 1] == IC_EMPTY && a.keys_m[k + 1] == IC_EMPTY && a.keys_m[k - a.w] == IC_EMPTY && a.keys_m[k + a.w] == IC_EMPTY;
    return alone ? FU_APPEND : FU_UNTOUCHED;
  }
  const uint32_t m = (uint32_t)mkey;
  // the keys carry the bits of the winners' c_z: the frame's is frame_xyz[f].z (no extrinsics), the model's is c_m.z
  const float fz = __int_as_float((int)(uint32_t)(fkey >> 32)), mz = __int_as_float((int)(uint32_t)(mkey >> 32));
  const F3 nc = ic_linear(a.to_cam, a.model.nrm[m]), fn = a.fnrm[f];
  const double ang = fu_ang(ic_dot3(nc.x, nc.y, nc.z, fn.x, fn.y, fn.z));
  if (fabsf(__fsub_rn(mz, fz)) < a.fusion_dist && ang < a.t_fuse) return FU_FUSE;      // :188-192
  if (ang > a.t_append) return FU_APPEND;                                              // :207-211
  if (fz > __fadd_rn(mz, a.occlusion_dist)) {                                          // :218-223
    const F3 cn = ic_normalized(ic_apply(a.to_cam, a.model.xyz[m]));
    if (fu_ang(-ic_dot3(cn.x, cn.y, cn.z, nc.x, nc.y, nc.z)) < a.t_free) return FU_REMOVE;
  }
  return FU_UNTOUCHED;
}

__global__ __launch_bounds__(IC_BLOCK) void k_fu_decide(FuArgs a) {
  const size_t k = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  const unsigned char d = fu_decision(a, k);
  if (k < a.npix) a.decision[k] = d;
  FuCount c;
  (void)block_rank<IC_BLOCK>(d == FU_FUSE, &c.fused);
  (void)block_rank<IC_BLOCK>(d == FU_APPEND, &c.appended);
  (void)block_rank<IC_BLOCK>(d == FU_REMOVE, &c.removed);
  (void)block_rank<IC_BLOCK>(d == FU_UNTOUCHED, &c.untouched);
  if (threadIdx.x == 0) a.block_counts[blockIdx.x] = c;
}

// F5 for the pixels that fuse; the pixels that remove leave their model index in S, in pixel order
__global__ __launch_bounds__(IC_BLOCK) void k_fu_fuse(FuArgs a) {
  const size_t k = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  const unsigned char d = k < a.npix ? a.decision[k] : (unsigned char)FU_NONE;
  uint32_t total;
  const uint32_t rank = block_rank<IC_BLOCK>(d == FU_REMOVE, &total);
  if (d != FU_FUSE && d != FU_REMOVE) return;
  const uint32_t m = (uint32_t)a.keys_m[k];      // (< n_model: k_fu_decide checked it)
  if (d == FU_REMOVE) {
    a.removed_idx[(size_t)a.block_counts[blockIdx.x].removed + rank] = m;
    return;
  }
  const uint32_t f = (uint32_t)a.keys_f[k];
  const uint32_t y = (uint32_t)(k / a.w), x = (uint32_t)(k - (size_t)y * a.w);
  const float rw = fu_radial(a, x, y), conf = a.model.conf[m];
  const float g = (float)((double)rw / (double)__fadd_rn(rw, conf));      // (the correctly rounded f32 quotient)
  const float gc = __fsub_rn(1.0f, g);
  const F3 q = ic_apply(a.pose, a.fxyz[f]), nq = ic_linear(a.pose, a.fnrm[f]), fc = a.frgb[f];
  const F3 p = a.model.xyz[m], n = a.model.nrm[m], c = a.model.rgb[m];
  auto mix = [gc, g](float o, float v) { return __fadd_rn(__fmul_rn(gc, o), __fmul_rn(g, v)); };
  a.model.xyz[m] = F3{mix(p.x, q.x), mix(p.y, q.y), mix(p.z, q.z)};
  a.model.nrm[m] = ic_normalized(F3{mix(n.x, nq.x), mix(n.y, nq.y), mix(n.z, nq.z)});
  a.model.rgb[m] = F3{mix(c.x, fc.x), mix(c.y, fc.y), mix(c.z, fc.z)};
  a.model.conf[m] = __fadd_rn(conf, g);
}

// F7: the appended rows, after the removal: row = n' + (appended rows of the blocks before) + (rank in the block)
__global__ __launch_bounds__(IC_BLOCK) void k_fu_append(FuArgs a, size_t capacity) {
  const size_t k = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  const unsigned char d = k < a.npix ? a.decision[k] : (unsigned char)FU_NONE;
  uint32_t total;
  const uint32_t rank = block_rank<IC_BLOCK>(d == FU_APPEND, &total);
  if (d != FU_APPEND) return;
  const size_t row = (size_t)a.n_after_remove + a.block_counts[blockIdx.x].appended + rank;
  if (row >= capacity) return;      // (the host compared the total with the capacity before this launch)
  const uint32_t f = (uint32_t)a.keys_f[k];
  const uint32_t y = (uint32_t)(k / a.w), x = (uint32_t)(k - (size_t)y * a.w);
  a.model.xyz[row] = ic_apply(a.pose, a.fxyz[f]);
  a.model.nrm[row] = ic_linear(a.pose, a.fnrm[f]);
  a.model.rgb[row] = a.frgb[f];
  a.model.conf[row] = fu_radial(a, x, y);
}

// F6.  S sorted ascending, cnt members, all < n; n' = n - cnt > 0.  Tail position j stands for row n - 1 - j (descending rows).
__global__ __launch_bounds__(IC_BLOCK) void k_fu_tail(const uint32_t* __restrict__ S, uint32_t cnt, uint32_t n, uint32_t* __restrict__ gone) {
  const size_t i = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t row = S[i];
  if (row < n && row >= n - cnt) gone[n - 1 - row] = 1u;      // (n - 1 - row < cnt)
}
// gone[j]: row n - 1 - j leaves; gone_before[j]: how many rows above it leave.  The surviving tail row of rank r = j - gone_before[j] fills hole S[r].
__global__ __launch_bounds__(IC_BLOCK) void k_fu_move(const uint32_t* __restrict__ S, uint32_t cnt, uint32_t n, const uint32_t* __restrict__ gone,
                                                      const uint32_t* __restrict__ gone_before, FuModel m) {
  const size_t j = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  if (j >= cnt || gone[j]) return;
  const uint32_t r = (uint32_t)j - gone_before[j];
  if (r >= cnt) return;
  const uint32_t dst = S[r], src = n - 1 - (uint32_t)j;
  if (dst >= n - cnt) return;      // (there are as many holes below n' as survivors in the tail)
  m.xyz[dst] = m.xyz[src]; m.nrm[dst] = m.nrm[src]; m.rgb[dst] = m.rgb[src]; m.conf[dst] = m.conf[src];
}

// F9: rows whose confidence is below the threshold (NaN: not below)
template <bool COUNT>
__global__ __launch_bounds__(IC_BLOCK) void k_fu_unstable(const float* __restrict__ conf, uint32_t n, float thresh, uint32_t* __restrict__ block_counts, uint32_t* __restrict__ S) {
  const size_t i = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  const bool out = i < n && conf[i] < thresh;
  uint32_t total;
  const uint32_t rank = block_rank<IC_BLOCK>(out, &total);
  if (COUNT) { if (threadIdx.x == 0) block_counts[blockIdx.x] = total; return; }
  if (out) S[(size_t)block_counts[blockIdx.x] + rank] = (uint32_t)i;
}

// F6 on the device: S (cnt members, `sorted` or not) leaves the n rows of m; returns through ST_CK's convention
int fu_remove_rows(const char* F, DevPool& pool, hipStream_t s, uint32_t* S, uint32_t cnt, bool sorted, uint32_t n, const FuModel& m) {
  if (cnt == 0 || cnt >= n) return CILHIP_OK;      // (nothing leaves / the model is cleared: no row moves)
  if (!sorted) {
    uint32_t* sorted_S = nullptr;
    ST_CK(F, pool.get(&sorted_S, cnt));
    ST_CK(F, prim_run(pool, prim_sort_keys(S, sorted_S, (size_t)cnt, 0, 32, s)));
    S = sorted_S;
  }
  uint32_t *gone = nullptr, *gone_before = nullptr;
  ST_CK(F, pool.get(&gone, cnt));
  ST_CK(F, pool.get(&gone_before, cnt));
  ST_CK(F, hipMemsetAsync(gone, 0, (size_t)cnt * sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_fu_tail, dim3(ic_blocks(cnt)), dim3(IC_BLOCK), 0, s, (const uint32_t*)S, cnt, n, gone);
  ST_CK(F, hipGetLastError());
  ST_CK(F, prim_run(pool, prim_exclusive_sum(gone, gone_before, (size_t)cnt, s)));
  hipLaunchKernelGGL(k_fu_move, dim3(ic_blocks(cnt)), dim3(IC_BLOCK), 0, s, (const uint32_t*)S, cnt, n, (const uint32_t*)gone, (const uint32_t*)gone_before, m);
  ST_CK(F, hipGetLastError());
  return CILHIP_OK;
}

struct FuCall {
  float *xyz, *nrm, *rgb, *conf; size_t n_model, capacity;
  const float *fxyz, *fnrm, *frgb; size_t n_frame; int mem;
  const float *pose, *K; size_t w, h; cilhip_fusion_params p; size_t* n_out; cilhip_fusion_counts* counts;
};

// the model's device image: the caller's arrays, or `rows` staged rows of which the first n hold the caller's
int fu_stage_model(const char* F, DevPool& pool, hipStream_t s, int mem, float* xyz, float* nrm, float* rgb, float* conf, size_t n, size_t rows, FuModel* m) {
  if (mem == CILHIP_MEM_DEVICE) {
    *m = FuModel{reinterpret_cast<F3*>(xyz), reinterpret_cast<F3*>(nrm), reinterpret_cast<F3*>(rgb), conf};
    return CILHIP_OK;
  }
  ST_CK(F, pool.get(&m->xyz, rows));
  ST_CK(F, pool.get(&m->nrm, rows));
  ST_CK(F, pool.get(&m->rgb, rows));
  ST_CK(F, pool.get(&m->conf, rows));
  if (n) {
    ST_CK(F, hipMemcpyAsync(m->xyz, xyz, n * sizeof(F3), hipMemcpyHostToDevice, s));
    ST_CK(F, hipMemcpyAsync(m->nrm, nrm, n * sizeof(F3), hipMemcpyHostToDevice, s));
    ST_CK(F, hipMemcpyAsync(m->rgb, rgb, n * sizeof(F3), hipMemcpyHostToDevice, s));
    ST_CK(F, hipMemcpyAsync(m->conf, conf, n * sizeof(float), hipMemcpyHostToDevice, s));
  }
  return CILHIP_OK;
}
int fu_model_back(const char* F, hipStream_t s, int mem, float* xyz, float* nrm, float* rgb, float* conf, size_t n, const FuModel& m) {
  if (mem == CILHIP_MEM_HOST && n) {
    ST_CK(F, hipMemcpyAsync(xyz, m.xyz, n * sizeof(F3), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipMemcpyAsync(nrm, m.nrm, n * sizeof(F3), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipMemcpyAsync(rgb, m.rgb, n * sizeof(F3), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipMemcpyAsync(conf, m.conf, n * sizeof(float), hipMemcpyDeviceToHost, s));
  }
  ST_CK(F, hipStreamSynchronize(s));
  return CILHIP_OK;
}

int fu_run(const FuCall& c, int device) {
  constexpr const char* F = "fuse_frame";
  if (const int open = st_open(F, device)) return open;
  DevPool pool;
  StreamGuard st;
  ST_CK(F, st.create());
  hipStream_t s = st.s;
  const size_t npix = c.w * c.h;
  const unsigned nblocks = ic_blocks(npix);
  FuArgs a{};
  if (const int rc = fu_stage_model(F, pool, s, c.mem, c.xyz, c.nrm, c.rgb, c.conf, c.n_model, c.capacity, &a.model)) return rc;
  ST_CK(F, st_stage(pool, s, c.mem, c.fxyz, c.n_frame, &a.fxyz));
  ST_CK(F, st_stage(pool, s, c.mem, c.fnrm, c.n_frame, &a.fnrm));
  ST_CK(F, st_stage(pool, s, c.mem, c.frgb, c.n_frame, &a.frgb));
  a.n_model = (uint32_t)c.n_model; a.n_frame = (uint32_t)c.n_frame;
  a.w = (uint32_t)c.w; a.h = (uint32_t)c.h; a.npix = (uint32_t)npix;
  a.to_cam = ic_to_cam(c.pose); a.pose = ic_rigid(c.pose);
  a.k02 = c.K[6]; a.k12 = c.K[7];
  a.fusion_dist = c.p.fusion_dist_thresh; a.occlusion_dist = c.p.occlusion_dist_thresh; a.radial_factor = c.p.radial_factor;
  a.t_fuse = ((double)c.p.fuse_max_angle_deg * M_PI) / 180.0;
  a.t_append = ((double)c.p.append_min_angle_deg * M_PI) / 180.0;
  a.t_free = ((double)c.p.free_space_max_angle_deg * M_PI) / 180.0;

  // F1: the two key images, side by side (one memset)
  unsigned long long* keys = nullptr;
  ST_CK(F, pool.get(&keys, 2 * npix));
  ST_CK(F, hipMemsetAsync(keys, 0xFF, 2 * npix * sizeof(unsigned long long), s));
  a.keys_m = keys; a.keys_f = keys + npix;
  IcSplat sp{};
  for (int j = 0; j < 3; ++j) { sp.k0[j] = c.K[0 + 3 * j]; sp.k1[j] = c.K[1 + 3 * j]; }
  sp.w = a.w; sp.h = a.h; sp.conv = IcConv{1.0f, 1.0f, 0.0f, 0, CILHIP_DEPTH_U16};
  if (c.n_model) {
    sp.xyz = a.model.xyz; sp.n = a.n_model; sp.has_cam = 1; sp.to_cam = a.to_cam; sp.keys = keys;
    hipLaunchKernelGGL((k_ic_splat<IC_INDEX>), dim3(ic_blocks(c.n_model)), dim3(IC_BLOCK), 0, s, sp);
    ST_CK(F, hipGetLastError());
  }
  sp.xyz = a.fxyz; sp.n = a.n_frame; sp.has_cam = 0; sp.keys = keys + npix;
  hipLaunchKernelGGL((k_ic_splat<IC_INDEX>), dim3(ic_blocks(c.n_frame)), dim3(IC_BLOCK), 0, s, sp);
  ST_CK(F, hipGetLastError());

  // F2-F4: every decision, and the populations per block
  ST_CK(F, pool.get(&a.decision, npix));
  ST_CK(F, pool.get(&a.block_counts, (size_t)nblocks + 1));
  ST_CK(F, hipMemsetAsync(a.block_counts + nblocks, 0, sizeof(FuCount), s));
  hipLaunchKernelGGL(k_fu_decide, dim3(nblocks), dim3(IC_BLOCK), 0, s, a);
  ST_CK(F, hipGetLastError());
  ST_CK(F, prim_run(pool, prim_exclusive_scan(a.block_counts, a.block_counts, FuCount{0, 0, 0, 0}, (size_t)nblocks + 1, FuPlus(), s)));
  FuCount total{};
  ST_CK(F, hipMemcpyAsync(&total, a.block_counts + nblocks, sizeof(FuCount), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));

  // F8, and the capacity: decided on the host word, before the first model row changes
  if (total.removed > c.n_model) return st_fail(CILHIP_ERR_HIP, F, "more rows removed than the model has (a model point won two pixels)");
  const size_t n_after = c.n_model - total.removed, n_new = n_after + total.appended;
  *c.n_out = n_new;
  if (c.counts) *c.counts = cilhip_fusion_counts{(size_t)total.fused + total.appended + total.removed + total.untouched, total.fused, total.appended, total.removed, total.untouched};
  if (n_new > c.capacity) return st_fail(CILHIP_ERR_INVALID, F, "capacity is smaller than the model after the update (*n_out has it; capacity = n_model + min(n_frame, w * h) always suffices)");
  a.n_after_remove = (uint32_t)n_after;
  if (total.fused || total.removed) {
    if (total.removed) ST_CK(F, pool.get(&a.removed_idx, total.removed));
    hipLaunchKernelGGL(k_fu_fuse, dim3(nblocks), dim3(IC_BLOCK), 0, s, a);
    ST_CK(F, hipGetLastError());
    if (const int rc = fu_remove_rows(F, pool, s, a.removed_idx, total.removed, false, a.n_model, a.model)) return rc;
  }
  if (total.appended) {
    hipLaunchKernelGGL(k_fu_append, dim3(nblocks), dim3(IC_BLOCK), 0, s, a, c.capacity);
    ST_CK(F, hipGetLastError());
  }
  return fu_model_back(F, s, c.mem, c.xyz, c.nrm, c.rgb, c.conf, n_new, a.model);
}

int fu_run_unstable(int device, float* xyz, float* nrm, float* rgb, float* conf, size_t n, int mem, float thresh, size_t* n_out) {
  constexpr const char* F = "fusion_remove_unstable";
  if (const int open = st_open(F, device)) return open;
  DevPool pool;
  StreamGuard st;
  ST_CK(F, st.create());
  hipStream_t s = st.s;
  FuModel m{};
  if (const int rc = fu_stage_model(F, pool, s, mem, xyz, nrm, rgb, conf, n, n, &m)) return rc;
  const unsigned nblocks = ic_blocks(n);
  uint32_t* counts = nullptr;
  ST_CK(F, pool.get(&counts, (size_t)nblocks + 1));
  ST_CK(F, hipMemsetAsync(counts + nblocks, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL((k_fu_unstable<true>), dim3(nblocks), dim3(IC_BLOCK), 0, s, (const float*)m.conf, (uint32_t)n, thresh, counts, (uint32_t*)nullptr);
  ST_CK(F, hipGetLastError());
  ST_CK(F, prim_run(pool, prim_exclusive_sum(counts, counts, (size_t)nblocks + 1, s)));
  uint32_t total = 0;
  ST_CK(F, hipMemcpyAsync(&total, counts + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  const size_t n_new = total >= n ? 0 : n - total;
  *n_out = n_new;
  if (total == 0 || n_new == 0) return CILHIP_OK;      // (nothing leaves / the model is cleared: no row moves)
  uint32_t* S = nullptr;
  ST_CK(F, pool.get(&S, total));
  hipLaunchKernelGGL((k_fu_unstable<false>), dim3(nblocks), dim3(IC_BLOCK), 0, s, (const float*)m.conf, (uint32_t)n, thresh, counts, S);
  ST_CK(F, hipGetLastError());
  if (const int rc = fu_remove_rows(F, pool, s, S, total, true, (uint32_t)n, m)) return rc;
  return fu_model_back(F, s, mem, xyz, nrm, rgb, conf, n_new, m);
}

}  // namespace

}  // namespace cilhip

extern "C" void cilhip_fusion_default_params(cilhip_fusion_params* p) {
  if (!p) return;
  p->fusion_dist_thresh = 0.01f; p->occlusion_dist_thresh = 0.025f; p->radial_factor = -0.5f / (120 * 120);      // fusion.cpp:98-100
  p->fuse_max_angle_deg = 75.0f; p->append_min_angle_deg = 105.0f; p->free_space_max_angle_deg = 45.0f;           // :192, :211, :223
}

extern "C" int cilhip_fuse_frame3f(int device, float* model_xyz, float* model_normals, float* model_rgb, float* model_conf, size_t n_model, size_t capacity,
                                   const float* frame_xyz, const float* frame_normals, const float* frame_rgb, size_t n_frame, int mem, const float* cam_pose,
                                   const float* K, size_t w, size_t h, const cilhip_fusion_params* params, size_t* n_out, cilhip_fusion_counts* counts_or_null) {
  using namespace cilhip;
  constexpr const char* F = "fuse_frame";
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (!n_out) return refuse("n_out is null");
  if (!params) return refuse("params is null");
  if (!K) return refuse("the intrinsic matrix is null");
  if (!cam_pose) return refuse("cam_pose is null");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (n_model > capacity) return refuse("n_model is larger than capacity");
  if ((unsigned long long)n_model >= IC_LIMIT || (unsigned long long)n_frame >= IC_LIMIT) return refuse("n_model and n_frame must be below 2^32 - 16");
  if ((unsigned long long)w >= IC_LIMIT || (unsigned long long)h >= IC_LIMIT || (unsigned long long)w * (unsigned long long)h >= IC_LIMIT) return refuse("w * h must be below 2^32 - 16");
  if (capacity > 0 && (!model_xyz || !model_normals || !model_rgb || !model_conf)) return refuse("a model array is null with capacity > 0");
  if (n_frame > 0 && (!frame_xyz || !frame_normals || !frame_rgb)) return refuse("a frame array is null with n_frame > 0");
  if (!ic_all_finite(K, 9)) return refuse("the intrinsic matrix has a non-finite entry");
  if (!ic_all_finite(cam_pose, 16)) return refuse("cam_pose has a non-finite entry");
  const float prm[6] = {params->fusion_dist_thresh, params->occlusion_dist_thresh, params->radial_factor, params->fuse_max_angle_deg, params->append_min_angle_deg,
                        params->free_space_max_angle_deg};
  if (!ic_all_finite(prm, 6)) return refuse("a parameter is not finite");
  if (prm[0] < 0.0f || prm[1] < 0.0f || prm[3] < 0.0f || prm[4] < 0.0f || prm[5] < 0.0f) return refuse("a distance or angle threshold is negative");
  st_clear();
  if (counts_or_null) *counts_or_null = cilhip_fusion_counts{0, 0, 0, 0, 0};
  if (w * h == 0 || n_frame == 0) { *n_out = n_model; return CILHIP_OK; }      // (no pixel is visited: without touching a device)
  const FuCall c{model_xyz, model_normals, model_rgb, model_conf, n_model, capacity, frame_xyz, frame_normals, frame_rgb, n_frame, mem, cam_pose, K, w, h, *params, n_out, counts_or_null};
  try {
    return fu_run(c, device);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

extern "C" int cilhip_fusion_remove_unstable3f(int device, float* model_xyz, float* model_normals, float* model_rgb, float* model_conf, size_t n_model, int mem,
                                               float conf_thresh, size_t* n_out) {
  using namespace cilhip;
  constexpr const char* F = "fusion_remove_unstable";
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (!n_out) return refuse("n_out is null");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if ((unsigned long long)n_model >= IC_LIMIT) return refuse("n_model must be below 2^32 - 16");
  if (n_model > 0 && (!model_xyz || !model_normals || !model_rgb || !model_conf)) return refuse("a model array is null with n_model > 0");
  st_clear();
  if (n_model == 0) { *n_out = 0; return CILHIP_OK; }
  try {
    return fu_run_unstable(device, model_xyz, model_normals, model_rgb, model_conf, n_model, mem, conf_thresh, n_out);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

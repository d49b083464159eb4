// image_conversions.hip -- depth / RGB-D images to points, normals and colours, and points back to a depth image or an index map:
// cilantro's core/image_point_cloud_conversions.hpp (depthImageToPoints[Normals], RGBDImagesToPoints[Normals]Colors,
// pointsToDepthImage, pointsColorsToRGBDImages, pointsToIndexMap), what the reference's fusion example runs on every frame.
//
// The contract (DESIGN.md section 14 has it in full, rule by rule; tests/_projective_refs.py restates it in numpy):
//   D1  z = inverseScale * (float)raw, inverseScale = 1.0f / scale; truncated: z < max_depth ? z : 0
//   D3  P = Kinv * (z * x, z * y, z), every row the pinned dot3(a, b) = a0 b0 + (a1 b1 + a2 b2), Kinv formed on the host (D2)
//   D4  a pixel is valid iff P_z > 0;  D5  normals at interior pixels whose own and four neighbouring P_z are > 0
//   D6  rows in ascending pixel index;  D7  extrinsics after everything else;  D8  colour = (1.0f / 255.0f) * (float)byte
//   P1  c = to_cam * p;  P2  c_z > 0 and finite projections;  P3  pixel = llround(inv_z * dot3(K_row, c)), ties away from zero
//   P4  the winner of a pixel: smallest c_z, then lowest index;  P5  depth image: smallest raw value, then lowest index
//
// The kernels:
//   k_ic_unproject<COUNT>   one lane per pixel; the four neighbours' points are recomputed from the depth words (same arithmetic, same
//                           bits), nothing like the reference's points_tmp is materialised.  COUNT: kept rows per block of 256 pixels
//                           (ballot / popcount per wave).  One rocPRIM exclusive scan of those counts, then the same kernel again writes
//                           every kept row at its block's offset plus its rank inside the block: rows leave in pixel order.
//   k_ic_splat<MODE>        (image_device.hpp, shared with fusion.hip) one lane per point: one 64-bit atomicMin on (bits(c_z) << 32) | index (index map) or (raw << 32) | index
//                           (depth image) -- c_z and raw are positive, so their f32 bits order as their values do; the minimum is rule
//                           P4 / P5 whatever the arrival order.  No floating-point atomics: two runs give the same bits.
//   k_ic_resolve_*          one lane per pixel: key -> index / u16 / f32 / rgb
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/cilantro_hip/c_api.h"
#include "device_prims.hpp"
#include "image_device.hpp"
#include "internal.hpp"
#include "stateless.hpp"

namespace cilhip {

namespace {

// (IcConv, IcRigid, ic_dot3, ic_apply, ic_normalized, ic_pixel, k_ic_splat, ic_rigid, ic_to_cam: image_device.hpp, shared with fusion.hip)

struct IcUnproject {
  const void* depth;            // u16 or f32, w * h
  const unsigned char* rgb;     // 3 bytes per pixel, or null
  uint32_t w, h, npix;
  IcConv conv;
  float kinv[9];                // row-major
  int has_e;
  IcRigid e;
  int keep_invalid, want_normals;
  uint32_t* block_counts;       // COUNT: [number of blocks]
  const uint32_t* block_offs;   // write pass without keep_invalid: exclusive scan of block_counts
  F3 *out_p, *out_n, *out_c;    // (null: not wanted)
};

// D1, D3: the camera-frame point of pixel k = y * w + x
__device__ __forceinline__ F3 ic_point(const IcUnproject& a, uint32_t x, uint32_t y) {
  const size_t k = (size_t)y * a.w + x;
  const float raw = a.conv.raw_type == CILHIP_DEPTH_U16 ? (float)static_cast<const uint16_t*>(a.depth)[k] : static_cast<const float*>(a.depth)[k];
  float z = __fmul_rn(a.conv.inv_scale, raw);
  if (a.conv.truncated) z = z < a.conv.max_depth ? z : 0.0f;
  const float v0 = __fmul_rn(z, (float)x), v1 = __fmul_rn(z, (float)y);
  return F3{ic_dot3(a.kinv[0], a.kinv[1], a.kinv[2], v0, v1, z), ic_dot3(a.kinv[3], a.kinv[4], a.kinv[5], v0, v1, z), ic_dot3(a.kinv[6], a.kinv[7], a.kinv[8], v0, v1, z)};
}

// D5: normalized(cross(P[k + w] - P[k - w], P[k + 1] - P[k - 1])); NaN where the rule gives none
__device__ __forceinline__ F3 ic_normal(const IcUnproject& a, uint32_t x, uint32_t y, F3 p) {
  const float nan = __int_as_float(0x7FC00000);
  F3 n{nan, nan, nan};
  if (a.w < 3 || a.h < 3 || x == 0 || y == 0 || x + 1 >= a.w || y + 1 >= a.h || !(p.z > 0.0f)) return n;
  const F3 r = ic_point(a, x + 1, y), l = ic_point(a, x - 1, y), d = ic_point(a, x, y + 1), u = ic_point(a, x, y - 1);
  if (!(r.z > 0.0f && l.z > 0.0f && d.z > 0.0f && u.z > 0.0f)) return n;
  const float ax = __fsub_rn(d.x, u.x), ay = __fsub_rn(d.y, u.y), az = __fsub_rn(d.z, u.z);
  const float bx = __fsub_rn(r.x, l.x), by = __fsub_rn(r.y, l.y), bz = __fsub_rn(r.z, l.z);
  const float cx = __fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by));
  const float cy = __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz));
  const float cz = __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx));
  return ic_normalized(F3{cx, cy, cz});
}

// One block per 256 consecutive pixels.  COUNT: block_counts[block] = kept rows of the block.  Otherwise: write the rows.
template <bool COUNT>
__global__ __launch_bounds__(IC_BLOCK) void k_ic_unproject(IcUnproject a) {
  const size_t k = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  const bool in = k < a.npix;
  const uint32_t y = in ? (uint32_t)(k / a.w) : 0u, x = in ? (uint32_t)(k - (size_t)y * a.w) : 0u;
  F3 p{0.f, 0.f, 0.f}, n{0.f, 0.f, 0.f};
  bool keep = false;
  if (in) {
    p = ic_point(a, x, y);
    if (a.want_normals) {
      n = ic_normal(a, x, y, p);
      keep = a.keep_invalid || !(n.x != n.x);      // image_point_cloud_conversions.hpp:232
    } else {
      keep = a.keep_invalid || p.z > 0.0f;         // :93
    }
  }
  size_t row = k;
  if (!a.keep_invalid) {
    uint32_t total;
    const uint32_t before = block_rank<IC_BLOCK>(keep, &total);
    if (COUNT) {
      if (threadIdx.x == 0) a.block_counts[blockIdx.x] = total;
      return;
    }
    row = (size_t)a.block_offs[blockIdx.x] + before;
  }
  if (COUNT || !keep) return;
  if (a.has_e) {      // D7
    p = ic_apply(a.e, p);
    if (a.want_normals) n = ic_linear(a.e, n);
  }
  if (a.out_p) a.out_p[row] = p;
  if (a.out_n) a.out_n[row] = n;
  if (a.out_c) {
    const float s = 1.0f / 255.0f;
    const unsigned char* c = a.rgb + 3 * k;
    a.out_c[row] = F3{__fmul_rn(s, (float)c[0]), __fmul_rn(s, (float)c[1]), __fmul_rn(s, (float)c[2])};
  }
}

__global__ __launch_bounds__(IC_BLOCK) void k_ic_resolve_index(const unsigned long long* __restrict__ keys, size_t npix, uint32_t* __restrict__ out) {
  const size_t k = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  if (k < npix) out[k] = keys[k] == IC_EMPTY ? 0xFFFFFFFFu : (uint32_t)keys[k];
}

// (uchar)(255.0f * colour): truncated, saturated to [0, 255], NaN -> 0
__device__ __forceinline__ unsigned char ic_byte(float c) {
  const float v = __fmul_rn(255.0f, c);
  if (!(v > 0.0f)) return 0;
  return v >= 255.0f ? (unsigned char)255 : (unsigned char)(int)v;
}

__global__ __launch_bounds__(IC_BLOCK) void k_ic_resolve_depth(const unsigned long long* __restrict__ keys, size_t npix, int raw_type, const F3* __restrict__ colours,
                                                               void* __restrict__ depth_out, unsigned char* __restrict__ rgb_out) {
  const size_t k = (size_t)blockIdx.x * IC_BLOCK + threadIdx.x;
  if (k >= npix) return;
  const unsigned long long key = keys[k];
  const bool empty = key == IC_EMPTY;
  const uint32_t hi = empty ? 0u : (uint32_t)(key >> 32);
  if (raw_type == CILHIP_DEPTH_U16) static_cast<uint16_t*>(depth_out)[k] = (uint16_t)hi;
  else static_cast<float*>(depth_out)[k] = __int_as_float((int)hi);
  if (rgb_out) {
    unsigned char r = 0, g = 0, b = 0;
    if (!empty) { const F3 c = colours[(uint32_t)key]; r = ic_byte(c.x); g = ic_byte(c.y); b = ic_byte(c.z); }
    rgb_out[3 * k] = r; rgb_out[3 * k + 1] = g; rgb_out[3 * k + 2] = b;
  }
}

// ---- host side of the rules ------------------------------------------------------------------------------------------
// D2: the inverse of the column-major f32 K, formed in f64, every entry rounded once; row-major out.  false: singular
bool ic_invert(const float* K, float out[9]) {
  double m[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m[r][c] = (double)K[r + 3 * c];
  const double c00 = m[1][1] * m[2][2] - m[1][2] * m[2][1], c01 = m[1][2] * m[2][0] - m[1][0] * m[2][2], c02 = m[1][0] * m[2][1] - m[1][1] * m[2][0];
  const double det = m[0][0] * c00 + m[0][1] * c01 + m[0][2] * c02;
  if (!(std::isfinite(det) && det != 0.0)) return false;
  const double inv[9] = {c00 / det, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) / det, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) / det,
                         c01 / det, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) / det, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) / det,
                         c02 / det, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) / det, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) / det};
  for (int i = 0; i < 9; ++i) { out[i] = (float)inv[i]; if (!std::isfinite(out[i])) return false; }
  return true;
}
// the converter's rules; null: fine
const char* ic_conv_rule(const cilhip_depth_converter* c) {
  if (!c) return "the depth converter is null";
  if (c->raw_type != CILHIP_DEPTH_U16 && c->raw_type != CILHIP_DEPTH_F32) return "raw_type: CILHIP_DEPTH_U16 or CILHIP_DEPTH_F32";
  if (!(c->scale > 0.0f) || !std::isfinite(c->scale)) return "the converter's scale must be a finite positive number";
  if (c->truncated && c->max_depth != c->max_depth) return "a truncated converter needs a max_depth that is not NaN";
  return nullptr;
}
IcConv ic_conv(const cilhip_depth_converter* c) { return IcConv{c->scale, 1.0f / c->scale, c->max_depth, c->truncated ? 1 : 0, c->raw_type}; }
inline size_t ic_raw_bytes(int raw_type) { return raw_type == CILHIP_DEPTH_U16 ? 2 : 4; }

template <class T> hipError_t ic_stage_bytes(DevPool& pool, hipStream_t s, int mem, const void* src, size_t bytes, const T** out) {
  if (mem == CILHIP_MEM_DEVICE) { *out = static_cast<const T*>(src); return hipSuccess; }
  T* d = nullptr;
  const hipError_t e = pool.bytes(&d, bytes);
  *out = d;
  return e != hipSuccess ? e : hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, s);
}

struct IcToPoints {
  const void* depth; const unsigned char* rgb; size_t w, h; int mem; IcConv conv; float kinv[9]; const float* E; int keep_invalid, want_normals;
  float *xyz_out, *nrm_out, *rgb_out; size_t capacity; size_t* n_out;
};

int ic_run_to_points(const IcToPoints& c, int device) {
  constexpr const char* F = "depth_image_to_points";
  if (const int open = st_open(F, device)) return open;
  DevPool pool;
  StreamGuard st;
  ST_CK(F, st.create());
  hipStream_t s = st.s;
  const size_t npix = c.w * c.h;
  const bool host = c.mem == CILHIP_MEM_HOST;
  IcUnproject a{};
  const unsigned char* d_depth = nullptr;
  ST_CK(F, ic_stage_bytes(pool, s, c.mem, c.depth, npix * ic_raw_bytes(c.conv.raw_type), &d_depth));
  a.depth = d_depth;
  const bool colours = c.rgb && c.rgb_out;
  if (colours) ST_CK(F, ic_stage_bytes(pool, s, c.mem, c.rgb, npix * 3, &a.rgb));
  a.w = (uint32_t)c.w; a.h = (uint32_t)c.h; a.npix = (uint32_t)npix; a.conv = c.conv;
  std::memcpy(a.kinv, c.kinv, sizeof(a.kinv));
  a.has_e = c.E != nullptr;
  if (c.E) a.e = ic_rigid(c.E);
  a.keep_invalid = c.keep_invalid; a.want_normals = c.want_normals;
  const unsigned nblocks = ic_blocks(npix);
  const bool want = c.xyz_out || c.nrm_out || c.rgb_out;
  size_t rows = npix;
  if (!c.keep_invalid) {
    uint32_t* counts = nullptr;
    ST_CK(F, pool.get(&counts, (size_t)nblocks + 1));
    ST_CK(F, hipMemsetAsync(counts + nblocks, 0, sizeof(uint32_t), s));
    a.block_counts = counts;
    hipLaunchKernelGGL((k_ic_unproject<true>), dim3(nblocks), dim3(IC_BLOCK), 0, s, a);
    ST_CK(F, hipGetLastError());
    ST_CK(F, prim_run(pool, prim_exclusive_sum(counts, counts, (size_t)nblocks + 1, s)));
    uint32_t total = 0;
    ST_CK(F, hipMemcpyAsync(&total, counts + nblocks, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ST_CK(F, hipStreamSynchronize(s));
    rows = total;
    a.block_offs = counts;
  }
  *c.n_out = rows;
  if (!want && c.capacity == 0) return CILHIP_OK;      // the counting call
  if (rows > c.capacity) return st_fail(CILHIP_ERR_INVALID, F, "capacity is smaller than the number of rows (*n_out has it; capacity = w * h always suffices)");
  if (rows == 0 || !want) return CILHIP_OK;
  const bool normals = c.want_normals && c.nrm_out;
  if (host) {
    if (c.xyz_out) ST_CK(F, pool.get(&a.out_p, rows));
    if (normals) ST_CK(F, pool.get(&a.out_n, rows));
    if (colours) ST_CK(F, pool.get(&a.out_c, rows));
  } else {
    a.out_p = reinterpret_cast<F3*>(c.xyz_out);
    a.out_n = normals ? reinterpret_cast<F3*>(c.nrm_out) : nullptr;
    a.out_c = colours ? reinterpret_cast<F3*>(c.rgb_out) : nullptr;
  }
  hipLaunchKernelGGL((k_ic_unproject<false>), dim3(nblocks), dim3(IC_BLOCK), 0, s, a);
  ST_CK(F, hipGetLastError());
  if (host) {
    if (a.out_p) ST_CK(F, hipMemcpyAsync(c.xyz_out, a.out_p, rows * sizeof(F3), hipMemcpyDeviceToHost, s));
    if (a.out_n) ST_CK(F, hipMemcpyAsync(c.nrm_out, a.out_n, rows * sizeof(F3), hipMemcpyDeviceToHost, s));
    if (a.out_c) ST_CK(F, hipMemcpyAsync(c.rgb_out, a.out_c, rows * sizeof(F3), hipMemcpyDeviceToHost, s));
  }
  ST_CK(F, hipStreamSynchronize(s));
  return CILHIP_OK;
}

struct IcToImage {
  const char* family; int mode; const float *xyz, *rgb; size_t n; int mem; const float *E, *K; IcConv conv; size_t w, h;
  void* out; unsigned char* rgb_out;      // out: uint32 indices (IC_INDEX) or u16 / f32 depth (IC_DEPTH)
};

int ic_run_to_image(const IcToImage& c, int device) {
  const char* F = c.family;
  const size_t npix = c.w * c.h;
  const size_t out_bytes = npix * (c.mode == IC_INDEX ? sizeof(uint32_t) : ic_raw_bytes(c.conv.raw_type));
  const bool host = c.mem == CILHIP_MEM_HOST;
  if (c.n == 0 && host) {      // an empty image, without a device
    std::memset(c.out, c.mode == IC_INDEX ? 0xFF : 0, out_bytes);
    if (c.rgb_out) std::memset(c.rgb_out, 0, npix * 3);
    return CILHIP_OK;
  }
  if (const int open = st_open(F, device)) return open;
  DevPool pool;
  StreamGuard st;
  ST_CK(F, st.create());
  hipStream_t s = st.s;
  IcSplat a{};
  if (c.n) ST_CK(F, st_stage(pool, s, c.mem, c.xyz, c.n, &a.xyz));
  const F3* d_rgb = nullptr;
  const bool colours = c.rgb && c.rgb_out;
  if (colours && c.n) ST_CK(F, st_stage(pool, s, c.mem, c.rgb, c.n, &d_rgb));
  a.n = (uint32_t)c.n;
  a.has_cam = c.E != nullptr;
  if (c.E) a.to_cam = ic_to_cam(c.E);
  for (int j = 0; j < 3; ++j) { a.k0[j] = c.K[0 + 3 * j]; a.k1[j] = c.K[1 + 3 * j]; }
  a.w = (uint32_t)c.w; a.h = (uint32_t)c.h; a.conv = c.conv;
  ST_CK(F, pool.get(&a.keys, npix));
  ST_CK(F, hipMemsetAsync(a.keys, 0xFF, npix * sizeof(unsigned long long), s));
  if (c.n) {
    if (c.mode == IC_INDEX) hipLaunchKernelGGL((k_ic_splat<IC_INDEX>), dim3(ic_blocks(c.n)), dim3(IC_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((k_ic_splat<IC_DEPTH>), dim3(ic_blocks(c.n)), dim3(IC_BLOCK), 0, s, a);
    ST_CK(F, hipGetLastError());
  }
  void* d_out = c.out;
  unsigned char* d_rgb_out = c.rgb_out;
  if (host) {
    ST_CK(F, pool.bytes(&d_out, out_bytes));
    if (c.rgb_out) ST_CK(F, pool.bytes(&d_rgb_out, npix * 3));
  }
  if (c.mode == IC_INDEX) hipLaunchKernelGGL(k_ic_resolve_index, dim3(ic_blocks(npix)), dim3(IC_BLOCK), 0, s, (const unsigned long long*)a.keys, npix, static_cast<uint32_t*>(d_out));
  else hipLaunchKernelGGL(k_ic_resolve_depth, dim3(ic_blocks(npix)), dim3(IC_BLOCK), 0, s, (const unsigned long long*)a.keys, npix, c.conv.raw_type, d_rgb, d_out, colours ? d_rgb_out : (unsigned char*)nullptr);
  ST_CK(F, hipGetLastError());
  if (host) {
    ST_CK(F, hipMemcpyAsync(c.out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    if (colours) ST_CK(F, hipMemcpyAsync(c.rgb_out, d_rgb_out, npix * 3, hipMemcpyDeviceToHost, s));
  }
  ST_CK(F, hipStreamSynchronize(s));
  return CILHIP_OK;
}

// the rules the two points -> image entries share; null: fine
const char* ic_image_rule(const float* xyz, size_t n, int mem, const float* K, size_t w, size_t h, const void* out) {
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return "mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE";
  if ((unsigned long long)n >= IC_LIMIT) return "n must be below 2^32 - 16";
  if ((unsigned long long)w >= IC_LIMIT || (unsigned long long)h >= IC_LIMIT || (unsigned long long)w * (unsigned long long)h >= IC_LIMIT) return "w * h must be below 2^32 - 16";
  if (n && !xyz) return "points is null";
  if (!K) return "the intrinsic matrix is null";
  if (!ic_all_finite(K, 9)) return "the intrinsic matrix has a non-finite entry";
  if (w * h && !out) return "the output image is null";
  return nullptr;
}

}  // namespace

}  // namespace cilhip

extern "C" void cilhip_depth_default_converter(cilhip_depth_converter* c) {
  if (!c) return;
  c->raw_type = CILHIP_DEPTH_U16; c->scale = 1.0f; c->truncated = 0; c->max_depth = 3.402823466e+38f;
}

extern "C" int cilhip_depth_image_to_points3f(int device, const void* depth, const unsigned char* rgb_or_null, size_t w, size_t h, int mem, const cilhip_depth_converter* conv,
                                              const float* K, const float* extrinsics_or_null, int keep_invalid, int want_normals, float* xyz_out, float* normals_out,
                                              float* rgb_out, size_t capacity, size_t* n_out) {
  using namespace cilhip;
  constexpr const char* F = "depth_image_to_points";
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (!n_out) return refuse("n_out is null");
  if (mem != CILHIP_MEM_HOST && mem != CILHIP_MEM_DEVICE) return refuse("mem: CILHIP_MEM_HOST or CILHIP_MEM_DEVICE");
  if (const char* why = ic_conv_rule(conv)) return refuse(why);
  if ((unsigned long long)w >= IC_LIMIT || (unsigned long long)h >= IC_LIMIT || (unsigned long long)w * (unsigned long long)h >= IC_LIMIT) return refuse("w * h must be below 2^32 - 16");
  if (w * h && !depth) return refuse("the depth image is null");
  if (!K) return refuse("the intrinsic matrix is null");
  IcToPoints c{};
  if (!ic_all_finite(K, 9) || !ic_invert(K, c.kinv)) return refuse("the intrinsic matrix must be finite and invertible");
  if (capacity > 0 && !xyz_out) return refuse("xyz_out is null with capacity > 0");
  if (capacity > 0 && want_normals && !normals_out) return refuse("want_normals without normals_out");
  if (capacity > 0 && rgb_or_null && !rgb_out) return refuse("an rgb image without rgb_out");
  st_clear();
  if (w * h == 0) { *n_out = 0; return CILHIP_OK; }      // (without touching a device)
  if (keep_invalid && capacity == 0 && !xyz_out && !normals_out && !rgb_out) { *n_out = w * h; return CILHIP_OK; }      // (the counting call: every pixel is a row)
  c.depth = depth; c.rgb = rgb_or_null; c.w = w; c.h = h; c.mem = mem; c.conv = ic_conv(conv); c.E = extrinsics_or_null;
  c.keep_invalid = keep_invalid ? 1 : 0; c.want_normals = want_normals ? 1 : 0;
  c.xyz_out = xyz_out; c.nrm_out = normals_out; c.rgb_out = rgb_out; c.capacity = capacity; c.n_out = n_out;
  try {
    return ic_run_to_points(c, device);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

extern "C" int cilhip_points_to_depth_image3f(int device, const float* xyz, const float* rgb_or_null, size_t n, int mem, const float* extrinsics_or_null, const float* K,
                                              const cilhip_depth_converter* conv, size_t w, size_t h, void* depth_out, unsigned char* rgb_out_or_null) {
  using namespace cilhip;
  constexpr const char* F = "points_to_depth_image";
  auto refuse = [](const char* why) { return st_fail(CILHIP_ERR_INVALID, F, why); };
  if (const char* why = ic_conv_rule(conv)) return refuse(why);
  if (const char* why = ic_image_rule(xyz, n, mem, K, w, h, depth_out)) return refuse(why);
  if (w * h && rgb_or_null && !rgb_out_or_null) return refuse("colours without an rgb output image");
  st_clear();
  if (w * h == 0) return CILHIP_OK;
  IcToImage c{F, IC_DEPTH, xyz, rgb_or_null, n, mem, extrinsics_or_null, K, ic_conv(conv), w, h, depth_out, rgb_or_null ? rgb_out_or_null : nullptr};
  try {
    return ic_run_to_image(c, device);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

extern "C" int cilhip_points_to_index_map3f(int device, const float* xyz, size_t n, int mem, const float* extrinsics_or_null, const float* K, size_t w, size_t h,
                                            uint32_t* index_out) {
  using namespace cilhip;
  constexpr const char* F = "points_to_index_map";
  if (const char* why = ic_image_rule(xyz, n, mem, K, w, h, index_out)) return st_fail(CILHIP_ERR_INVALID, F, why);
  st_clear();
  if (w * h == 0) return CILHIP_OK;
  IcToImage c{F, IC_INDEX, xyz, nullptr, n, mem, extrinsics_or_null, K, IcConv{1.0f, 1.0f, 0.0f, 0, CILHIP_DEPTH_U16}, w, h, index_out, nullptr};
  try {
    return ic_run_to_image(c, device);
  } catch (...) {
    return st_fail(CILHIP_ERR_HIP, F, "out of host memory");
  }
}

// dev probe: what a read-only streaming kernel reaches on this box, in the access shape of the warm-started iteration
// (k_warm<ACC, 2>: per query 16 B + 12 B + 12 B from three arrays, coalesced, one query per lane and round) -- the practical
// ceiling next to the 8 TB/s spec peak and the device-copy figure on the bench line.
// build: hipcc -O3 -fno-slp-vectorize -ffp-contract=off --offload-arch=gfx950 tools/read_bw_probe.hip -o tools/bin/read_bw_probe
// (warm.hip's flags: the SLP vectoriser pairs the two register sets' arithmetic and the waits then drain both) ; run: tools/bin/read_bw_probe [n] [--stream-only]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <algorithm>
struct F3 { float x, y, z; };
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

// chunked like k_warm: block b owns a contiguous chunk, XCD-aware remap, one element per lane and round, DEPTH rounds in flight
template <int DEPTH, bool XCD>
__global__ __launch_bounds__(256) void k_read3(const float4* __restrict__ a, const F3* __restrict__ b, const F3* __restrict__ c, uint32_t n, float* out) {
  const uint32_t nb = gridDim.x;
  const uint32_t vb = XCD ? (blockIdx.x & 7u) * (nb >> 3) + (blockIdx.x >> 3) : blockIdx.x;
  const uint32_t chunk = (((n + nb - 1) / nb) + 255u) & ~255u;
  const uint64_t beg64 = (uint64_t)vb * chunk;
  const uint32_t beg = beg64 < n ? (uint32_t)beg64 : n, end = beg64 + chunk < n ? (uint32_t)(beg64 + chunk) : n;
  float s = 0.f;
  for (uint32_t i0 = beg + threadIdx.x; i0 < end; i0 += 256u * DEPTH) {
    float4 ra[DEPTH]; F3 rb[DEPTH], rc[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) { const uint32_t i = i0 + 256u * d; if (i < end) { ra[d] = a[i]; rb[d] = b[i]; rc[d] = c[i]; } else { ra[d] = make_float4(0, 0, 0, 0); rb[d] = F3{0, 0, 0}; rc[d] = F3{0, 0, 0}; } }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) s += ra[d].x + ra[d].y + ra[d].z + ra[d].w + rb[d].x + rb[d].y + rb[d].z + rc[d].x + rc[d].y + rc[d].z;
  }
  if (s == 12345.678f) out[0] = s;
}
// one flat array of float4, grid-stride
template <int DEPTH>
__global__ __launch_bounds__(256) void k_read1(const float4* __restrict__ a, size_t n4, float* out) {
  float s = 0.f;
  const size_t stride = (size_t)gridDim.x * 256u;
  for (size_t i0 = (size_t)blockIdx.x * 256u + threadIdx.x; i0 < n4; i0 += stride * DEPTH) {
    float4 r[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) { const size_t i = i0 + stride * d; r[d] = i < n4 ? a[i] : make_float4(0, 0, 0, 0); }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) s += r[d].x + r[d].y + r[d].z + r[d].w;
  }
  if (s == 12345.678f) out[0] = s;
}
// the same sweep from the END of the buffer (rev): what a pass that follows a forward pass finds in the memory-side cache (256 MB
// "infinity cache"): a forward pass over more than the cache leaves its TAIL there, a pass in the same direction starts at the head
// (every line evicted before it is reached again), a pass in the opposite direction starts where the last one ended
template <int DEPTH>
__global__ __launch_bounds__(256) void k_read1_dir(const float4* __restrict__ a, size_t n4, int rev, float* out) {
  float s = 0.f;
  const size_t stride = (size_t)gridDim.x * 256u;
  for (size_t i0 = (size_t)blockIdx.x * 256u + threadIdx.x; i0 < n4; i0 += stride * DEPTH) {
    float4 r[DEPTH];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) { const size_t i = i0 + stride * d; r[d] = i < n4 ? a[rev ? n4 - 1 - i : i] : make_float4(0, 0, 0, 0); }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) s += r[d].x + r[d].y + r[d].z + r[d].w;
  }
  if (s == 12345.678f) out[0] = s;
}

// ---- the warm iteration's stream as k_warm<., 2> really runs it ------------------------------------------------------------------
// SETS register sets per wave (k_warm: 2); a set is requested again only after it was consumed, the loads of a set leave in k_warm's
// order (src3, record, normal).  POL: which arrays are read with __builtin_nontemporal_load (1 = the 16-byte record, 2 = src3,
// 4 = the normals).  WORK: k_warm's non-memory work per round -- transform, one d2, the lane's 8 terms to LDS, eight
// v_mfma_f64_16x16x4_f64 fed by ds_reads -- at k_warm's LDS footprint (34816 B: four blocks per CU).  rev: the same chunks and rows
// taken from the far end of the arrays (what a pass in the opposite direction finds in the memory-side cache).
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f3v __attribute__((ext_vector_type(3), aligned(4)));
template <bool NT> __device__ __forceinline__ float4 ld4(const float4* p) {
  if (NT) { const f4v v = __builtin_nontemporal_load(reinterpret_cast<const f4v*>(p)); return make_float4(v.x, v.y, v.z, v.w); }
  const f4v v = *reinterpret_cast<const f4v*>(p); return make_float4(v.x, v.y, v.z, v.w);      // (the same typed load: the listings differ in the policy bit only)
}
template <bool NT> __device__ __forceinline__ F3 ld3(const F3* p) {
  if (NT) { const f3v v = __builtin_nontemporal_load(reinterpret_cast<const f3v*>(p)); return F3{v.x, v.y, v.z}; }
  const f3v v = *reinterpret_cast<const f3v*>(p); return F3{v.x, v.y, v.z};
}
struct Xf { float T[12]; };
template <int SETS, int POL, bool WORK>
__global__ __launch_bounds__(256, 4) void k_stream(const float4* __restrict__ a, const F3* __restrict__ b, const F3* __restrict__ c, uint32_t n, int rev, Xf xf, float* out) {
  __shared__ __attribute__((aligned(16))) float lds[WORK ? 34816 / 4 : 4];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  float* const zb = lds + (WORK ? wave * 896 : 0);
  const uint32_t nb = gridDim.x;
  const uint32_t vb = (blockIdx.x & 7u) * (nb >> 3) + (blockIdx.x >> 3);
  const uint32_t chunk = (((n + nb - 1) / nb) + 255u) & ~255u;
  const uint64_t beg64 = (uint64_t)vb * chunk;
  const uint32_t beg = beg64 < n ? (uint32_t)beg64 : n, end = beg64 + chunk < n ? (uint32_t)(beg64 + chunk) : n;
  const uint32_t last = end > beg ? end - 1u : 0u;
  typedef double double4_t __attribute__((ext_vector_type(4)));
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  float s = 0.f;
  F3 sv[SETS], nv[SETS]; float4 rv[SETS];
  auto load = [&](int k, uint32_t i) {
    uint32_t ic = i < last ? i : last;      // (unconditional, clamped: as k_warm)
    if (rev) ic = n - 1u - ic;
    __builtin_amdgcn_sched_barrier(0);
    sv[k] = ld3<(POL & 2) != 0>(b + ic);
    __builtin_amdgcn_sched_barrier(0);
    rv[k] = ld4<(POL & 1) != 0>(a + ic);
    __builtin_amdgcn_sched_barrier(0);
    nv[k] = ld3<(POL & 4) != 0>(c + ic);
    __builtin_amdgcn_sched_barrier(0);
  };
  auto consume = [&](int k, bool valid) {
    if (!WORK) { const float t = sv[k].x + sv[k].y + sv[k].z + rv[k].x + rv[k].y + rv[k].z + rv[k].w + nv[k].x + nv[k].y + nv[k].z; s += valid ? t : 0.f; return; }
    const float* T = xf.T;
    const float qx = T[0] * sv[k].x + (T[3] * sv[k].y + T[6] * sv[k].z) + T[9], qy = T[1] * sv[k].x + (T[4] * sv[k].y + T[7] * sv[k].z) + T[10],
                qz = T[2] * sv[k].x + (T[5] * sv[k].y + T[8] * sv[k].z) + T[11];
    const float dx = qx - rv[k].x, dy = qy - rv[k].y, dz = qz - rv[k].z;
    const float e = dx * dx + (dy * dy + dz * dz);
    const bool has = valid && e < rv[k].w * rv[k].w;
    const float nx = has ? nv[k].x : 0.f, ny = has ? nv[k].y : 0.f, nz = has ? nv[k].z : 0.f;
    float4* w4 = reinterpret_cast<float4*>(zb + lane * 8 + (lane >= 32 ? 16 : 0));
    w4[0] = make_float4(qy * nz - qz * ny, qz * nx - qx * nz, qx * ny - qy * nx, nx);
    w4[1] = make_float4(ny, nz, dx * nx + (dy * ny + dz * nz), 0.f);
  };
  auto mfma = [&]() {
    if (!WORK) return;
    __builtin_amdgcn_wave_barrier();
    const int comp = lane & 7, hf = (lane >> 3) & 1, k4 = lane >> 4;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int qi = hf * 32 + 4 * jj + k4;
      const double x = (double)zb[qi * 8 + hf * 16 + comp];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, x, acc, 0, 0, 0);
    }
    __builtin_amdgcn_wave_barrier();
  };
  uint32_t i = beg + threadIdx.x;
#pragma unroll
  for (int k = 0; k < SETS; ++k) load(k, i + 256u * k);
  for (uint32_t base = beg; base < end; base += 256u * SETS) {
#pragma unroll
    for (int k = 0; k < SETS; ++k) {
      consume(k, i + 256u * k < end);
      __builtin_amdgcn_sched_barrier(0);
      load(k, i + 256u * (k + SETS));
      __builtin_amdgcn_sched_barrier(0);
      mfma();
    }
    i += 256u * SETS;
  }
  if (WORK) s = (float)(acc[0] + acc[1] + acc[2] + acc[3]);
  if (s == 12345.678f) out[0] = s;
}
struct Stat { double med, lo, hi; };
template <class F>
static Stat time_stat(F f, int reps = 40) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 4; ++i) f();
  std::vector<float> t;
  for (int i = 0; i < reps; ++i) { CK(hipEventRecord(e0, 0)); f(); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms); }
  CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
  std::sort(t.begin(), t.end());
  return Stat{t[t.size() / 2], t[t.size() / 10], t[t.size() - 1 - t.size() / 10]};
}
template <int SETS, int POL, bool WORK>
static void run_stream(const char* what, const float4* a, const F3* b, const F3* c, uint32_t n, int dir_mode, float* out) {
  // dir_mode 0: every pass forward; 1: passes alternate direction
  Xf xf = {{1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.001f, 0.002f, 0.003f}};
  int flip = 0;
  const Stat st = time_stat([&] { hipLaunchKernelGGL((k_stream<SETS, POL, WORK>), dim3(1024), dim3(256), 0, 0, a, b, c, n, flip, xf, out); if (dir_mode) flip ^= 1; });
  printf("stream %-34s sets %d %s %s: median %7.2f us (p10 %7.2f, p90 %7.2f)  %.2f TB/s\n", what, SETS, WORK ? "work  " : "loads ", dir_mode ? "alternating" : "same-dir   ",
         st.med * 1e3, st.lo * 1e3, st.hi * 1e3, 40.0 * n / st.med / 1e9);
}
template <class F>
static double time_ms(F f, int reps = 20) {
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) f();
  std::vector<float> t;
  for (int i = 0; i < reps; ++i) { CK(hipEventRecord(e0, 0)); f(); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); float ms; CK(hipEventElapsedTime(&ms, e0, e1)); t.push_back(ms); }
  std::sort(t.begin(), t.end());
  return t[t.size() / 2];
}
int main(int argc, char** argv) {
  const uint32_t n = argc > 1 ? (uint32_t)atof(argv[1]) : 10000000u;
  float4* a; F3 *b, *c; float* out; char *x, *y;
  CK(hipMalloc(&a, (size_t)n * 16)); CK(hipMalloc(&b, (size_t)n * 12)); CK(hipMalloc(&c, (size_t)n * 12)); CK(hipMalloc(&out, 4));
  CK(hipMemset(a, 0, (size_t)n * 16)); CK(hipMemset(b, 0, (size_t)n * 12)); CK(hipMemset(c, 0, (size_t)n * 12));
  const size_t G = 1ull << 30;
  CK(hipMalloc(&x, G)); CK(hipMalloc(&y, G)); CK(hipMemset(x, 1, G));
  const double bytes3 = 40.0 * n;
  printf("n = %u: three-array stream %.1f MB per pass\n", n, bytes3 / 1e6);
  // the warm iteration's stream: policy x depth x arithmetic (1024 blocks: k_warm's grid at this size); the plain two-set skeleton
  // is repeated at the start, in the middle and at the end -- the spread of those three is what a difference has to exceed
  CK(hipMemset(a, 0x3c, (size_t)n * 16));      // (finite values: the arithmetic variant is not fed denormals or zeros only)
  CK(hipMemset(b, 0x3c, (size_t)n * 12)); CK(hipMemset(c, 0x3c, (size_t)n * 12));
  run_stream<2, 0, false>("plain (skeleton, repeat 1)", a, b, c, n, 0, out);
  run_stream<2, 7, false>("nt all", a, b, c, n, 0, out);
  run_stream<2, 6, false>("record plain, src3+normal nt", a, b, c, n, 0, out);
  run_stream<2, 1, false>("record nt, src3+normal plain", a, b, c, n, 0, out);
  run_stream<3, 0, false>("plain", a, b, c, n, 0, out);
  run_stream<3, 7, false>("nt all", a, b, c, n, 0, out);
  run_stream<4, 0, false>("plain", a, b, c, n, 0, out);
  run_stream<4, 7, false>("nt all", a, b, c, n, 0, out);
  run_stream<2, 0, false>("plain (skeleton, repeat 2)", a, b, c, n, 0, out);
  run_stream<2, 0, true>("plain", a, b, c, n, 0, out);
  run_stream<2, 7, true>("nt all", a, b, c, n, 0, out);
  run_stream<2, 6, true>("record plain, src3+normal nt", a, b, c, n, 0, out);
  run_stream<3, 0, true>("plain", a, b, c, n, 0, out);
  run_stream<3, 7, true>("nt all", a, b, c, n, 0, out);
  // does an nt stream leave the plain 16-byte record array (16 B x n) in the memory-side cache?  same direction vs alternating
  run_stream<2, 0, false>("plain", a, b, c, n, 1, out);
  run_stream<2, 7, false>("nt all", a, b, c, n, 1, out);
  run_stream<2, 6, false>("record plain, src3+normal nt", a, b, c, n, 1, out);
  run_stream<2, 6, true>("record plain, src3+normal nt", a, b, c, n, 1, out);
  run_stream<2, 0, true>("plain", a, b, c, n, 1, out);
  run_stream<2, 0, false>("plain (skeleton, repeat 3)", a, b, c, n, 0, out);
  if (argc > 2 && !strcmp(argv[2], "--stream-only")) return 0;
  for (int nb : {1024, 2048, 4096, 8192, 16384}) {
    double t1 = time_ms([&] { hipLaunchKernelGGL((k_read3<1, true>), dim3(nb), dim3(256), 0, 0, a, b, c, n, out); });
    double t2 = time_ms([&] { hipLaunchKernelGGL((k_read3<2, true>), dim3(nb), dim3(256), 0, 0, a, b, c, n, out); });
    double t4 = time_ms([&] { hipLaunchKernelGGL((k_read3<4, true>), dim3(nb), dim3(256), 0, 0, a, b, c, n, out); });
    double t2n = time_ms([&] { hipLaunchKernelGGL((k_read3<2, false>), dim3(nb), dim3(256), 0, 0, a, b, c, n, out); });
    printf("read3 chunked blocks=%5d: depth1 %.4f ms %.2f TB/s | depth2 %.4f ms %.2f TB/s | depth4 %.4f ms %.2f TB/s | depth2 no-xcd-map %.4f ms %.2f TB/s\n", nb, t1, bytes3 / t1 / 1e9,
           t2, bytes3 / t2 / 1e9, t4, bytes3 / t4 / 1e9, t2n, bytes3 / t2n / 1e9);
  }
  for (size_t mb : {400ull, 1024ull}) {
    const size_t n4 = mb * (1ull << 20) / 16;
    for (int nb : {2048, 8192, 32768}) {
      double t2 = time_ms([&] { hipLaunchKernelGGL((k_read1<2>), dim3(nb), dim3(256), 0, 0, (const float4*)x, n4, out); });
      double t4 = time_ms([&] { hipLaunchKernelGGL((k_read1<4>), dim3(nb), dim3(256), 0, 0, (const float4*)x, n4, out); });
      printf("read1 %4zu MiB grid-stride blocks=%5d: depth2 %.4f ms %.2f TB/s | depth4 %.4f ms %.2f TB/s\n", mb, nb, t2, n4 * 16.0 / t2 / 1e9, t4, n4 * 16.0 / t4 / 1e9);
    }
  }
  // the memory-side cache: repeated passes over buffers below and above its size, and passes that alternate direction
  for (size_t mb : {64ull, 128ull, 192ull, 256ull, 320ull, 400ull, 800ull}) {
    const size_t n4 = mb * (1ull << 20) / 16;
    const int nb = 8192;
    double tf = time_ms([&] { hipLaunchKernelGGL((k_read1_dir<4>), dim3(nb), dim3(256), 0, 0, (const float4*)x, n4, 0, out); });
    int flip = 0;
    double ta = time_ms([&] { hipLaunchKernelGGL((k_read1_dir<4>), dim3(nb), dim3(256), 0, 0, (const float4*)x, n4, flip, out); flip ^= 1; });
    printf("read1 %4zu MiB repeated: same direction %.4f ms %.2f TB/s | alternating direction %.4f ms %.2f TB/s\n", mb, tf, n4 * 16.0 / tf / 1e9, ta, n4 * 16.0 / ta / 1e9);
  }
  double tc = time_ms([&] { CK(hipMemcpyAsync(y, x, G, hipMemcpyDeviceToDevice, 0)); }, 10);
  printf("device copy 1 GiB: %.4f ms = %.2f TB/s (read + write)\n", tc, 2.0 * G / tc / 1e9);
  return 0;
}

// c_api.hip -- the C ABI of libcilantro_hip.so (declared in include/cilantro_hip/c_api.h): contexts and their stream, the clouds a context
// holds and the buffers built on demand over them (ensure_*), the option entry points, timing and diagnostic getters, a single
// correspondence search and the calls that read the stored set back.  The rest of the ABI by what a call touches: tie_tables.hip,
// estimate.hip, shard_keys.hip, icp_loop.hip (the loop drivers).
// Host-side orchestration only: owns device buffers + stream, enqueues the kernels of kernels.hip /
// grid_build.hip.  No CPU compute fallback exists: without a usable HIP device every call fails.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#include "ctx.hpp"
#include "stateless.hpp"

// (multi.hip -- the C entry of the multi-device loops -- drives contexts through the public entry points; these two are all it reads of one)
namespace cilhip {
hipStream_t ctx_stream(const cilhip_ctx* c) { return c->stream; }
double ctx_wait_us(const cilhip_ctx* c) { return c->wait_us; }
}  // namespace cilhip

// everything a context holds of its target: grid arrays, the tables built on top of them, the per-target buffers of the filters and
// the reverse searches, the colours that were set for it
static void release_target(cilhip_ctx* c) {
  static_cast<TargetBufs&>(*c) = TargetBufs{};
  c->grid.pts = nullptr; c->grid.nrm = nullptr; c->grid.pn = nullptr; c->grid.cell_start = nullptr;
  c->has_target = false; c->dst_rgb_sorted_ok = false;
}

// (the entry points take their C linkage from their declarations in c_api.h)

int cilhip_create(cilhip_ctx** out, int device) {
  if (!out) return CILHIP_ERR_INVALID;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return CILHIP_ERR_NO_DEVICE;
  if (device < 0 || device >= ndev) return CILHIP_ERR_INVALID;
  cilhip_ctx* c = new (std::nothrow) cilhip_ctx();
  if (!c) return CILHIP_ERR_HIP;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || c->own_stream.create() != hipSuccess) {
    delete c;
    return CILHIP_ERR_HIP;
  }
  c->stream = c->own_stream;
  if (c->d_state.alloc(1) != hipSuccess || c->d_count.alloc(1) != hipSuccess ||
      c->d_defer_flag.alloc(1) != hipSuccess || hipMemset(c->d_defer_flag, 0, sizeof(uint32_t)) != hipSuccess ||
      c->d_unproven.alloc(128) != hipSuccess || hipMemset(c->d_unproven, 0, 128 * sizeof(uint32_t)) != hipSuccess ||
      c->d_ticket.alloc(1) != hipSuccess || hipMemset(c->d_ticket, 0, sizeof(unsigned int)) != hipSuccess ||
      hipHostMalloc(&c->h_feedback, sizeof(Feedback), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
      hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_feedback), c->h_feedback, 0) != hipSuccess ||
      c->d_trace.alloc(RUN_TRACE_CAP) != hipSuccess || hipMemset(c->d_trace, 0, RUN_TRACE_CAP * sizeof(uint4)) != hipSuccess ||
      c->d_stage.alloc(REDUCE_STAGE_DOUBLES) != hipSuccess || c->d_sums.alloc(3 * SUMS_MAX) != hipSuccess) {
    delete c;
    return CILHIP_ERR_HIP;
  }
  if (hipMemset(c->d_state, 0, sizeof(IcpState)) != hipSuccess) { delete c; return CILHIP_ERR_HIP; }
  c->d_tie_counters = reinterpret_cast<unsigned int*>(reinterpret_cast<char*>(c->d_state.get()) + offsetof(IcpState, tie_counters));      // (read with the state: read_state)
  memcpy(c->sort_T, kIdentity16, sizeof(kIdentity16));
  memcpy(c->nn_T, kIdentity16, sizeof(kIdentity16));
  *out = c;
  return CILHIP_OK;
}

static void free_source(cilhip_ctx* c) {
  static_cast<SourceBufs&>(*c) = SourceBufs{};      // (d_tiles / d_tile_center pointed into its sort_ws)
  c->src_grid = GridDev{}; c->has_src_grid = false;
  c->rev_tie_valid = false; c->rev_tie_aware = false;      // (the reverse order tables described this source under one transform)
  c->src3_valid = false; c->lb_fresh = false; c->rec_valid = false;
  c->d_tiles = nullptr; c->d_tile_center = nullptr; c->ntiles = 0;
  c->has_source = false; c->src_sorted = false; drop_correspondences(c); c->ns = 0;
  c->policy.far_mode = true;
  c->policy.warm_banned = false;
}

void cilhip_destroy(cilhip_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)cilhip_rank_comm_destroy(c);
  delete c;      // (every buffer is a member; the context's own stream is the last thing to go: ctx.hpp)
}

const char* cilhip_last_error(const cilhip_ctx* c) { return c ? c->err.c_str() : cilhip::stateless_last_error(); }

int cilhip_set_stream(cilhip_ctx* c, void* s) {
  if (!c) return CILHIP_ERR_INVALID;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return CILHIP_OK;
}

int cilhip_synchronize(cilhip_ctx* c) {
  if (!c) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}

// ---- the options of a context: the table a C caller can enumerate and check at compile time (enum cilhip_option in c_api.h) is
// ctx_options.hpp's, one row per option; it is also what tests/test_capi_symbols.py walks (every option documented, accepted with its
// default, readable, exercised by a test).
static const OptionRow* option_row(const char* key) {
  for (const OptionRow& r : kOptionRows) if (!strcmp(key, r.info.key)) return &r;
  return nullptr;
}
// a row's admissible range holds for every key (a mistyped "tiled" = 3 would otherwise run some other form); the row adds what a range cannot say
static int store_option(cilhip_ctx* c, const OptionRow* row, double value) {
  if (value != value) return fail(c, CILHIP_ERR_INVALID, "set_option: the value is not a number");
  if (!row) return fail(c, CILHIP_ERR_INVALID, "set_option: unknown key");
  if (!(value >= row->info.min_value && value <= row->info.max_value))
    return fail(c, CILHIP_ERR_INVALID, "set_option: value outside the option's [min_value, max_value] (cilhip_option_info)");
  unsigned stale = 0;
  if (const char* refusal = row->set(*c, value, &stale)) return fail(c, CILHIP_ERR_INVALID, refusal);
  apply_stale(c, stale);
  return CILHIP_OK;
}

int cilhip_option_count(void) { return N_OPTIONS; }
const cilhip_option_info_t* cilhip_option_info(int id) { return (id >= 0 && id < N_OPTIONS) ? &kOptionRows[id].info : nullptr; }
int cilhip_set_option_id(cilhip_ctx* c, cilhip_option id, double value) {
  if (!c) return CILHIP_ERR_INVALID;
  if ((int)id < 0 || (int)id >= N_OPTIONS) return fail(c, CILHIP_ERR_INVALID, "set_option_id: unknown option");
  return store_option(c, &kOptionRows[(int)id], value);
}
int cilhip_get_option(cilhip_ctx* c, const char* key, double* value) {
  if (!c || !key || !value) return CILHIP_ERR_INVALID;
  const OptionRow* row = option_row(key);
  if (!row) return fail(c, CILHIP_ERR_INVALID, "get_option: unknown key");
  *value = row->get(*c);
  return CILHIP_OK;
}
int cilhip_set_option(cilhip_ctx* c, const char* key, double value) {
  if (!c || !key) return CILHIP_ERR_INVALID;
  return store_option(c, option_row(key), value);
}

int cilhip_debug_counters(cilhip_ctx* c, uint32_t out[2]) {
  if (!c || !out) return CILHIP_ERR_INVALID;
  out[0] = out[1] = 0;
  if (!c->d_defer_mask || !c->ntiles) return CILHIP_OK;
  CK(c, hipSetDevice(c->device));
  if (!c->d_dbg) CK(c, c->d_dbg.alloc(2));
  launch_count_deferred(c->d_defer_mask, c->ntiles, c->d_dbg, c->stream);
  CK(c, hipMemcpyAsync(out, c->d_dbg, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
#ifdef CILHIP_EXP_PHASE_CLOCKS
  cilhip::debug_dump_phase_clocks();
#endif
  return CILHIP_OK;
}

int cilhip_debug_live_allocations(unsigned long long out[2]) {
  if (!out) return CILHIP_ERR_INVALID;
  out[0] = dev_mem_live().count.load(std::memory_order_relaxed);
  out[1] = dev_mem_live().bytes.load(std::memory_order_relaxed);
  return CILHIP_OK;
}

int cilhip_get_last_timing2(cilhip_ctx* c, double* search_ms, double* accumulate_ms) {
  if (!c) return CILHIP_ERR_INVALID;
  if (search_ms) *search_ms = c->last_search_ms;
  if (accumulate_ms) *accumulate_ms = c->last_acc_ms;
  return CILHIP_OK;
}

int cilhip_get_last_iteration_timing(cilhip_ctx* c, int cap, int* n, unsigned int* iteration, float* kernel_ms) {
  if (!c || !n || cap < 0) return CILHIP_ERR_INVALID;
  const size_t m = c->timed_ms.size() < c->timed_iter.size() ? c->timed_ms.size() : c->timed_iter.size();
  *n = (int)m;
  for (size_t k = 0; k < m && k < (size_t)cap; ++k) { if (iteration) iteration[k] = c->timed_iter[k]; if (kernel_ms) kernel_ms[k] = c->timed_ms[k]; }
  return CILHIP_OK;
}

int cilhip_get_last_form_timing(cilhip_ctx* c, int form, double* kernel_ms, int* launches) {
  if (!c || form < 0 || form > 4) return CILHIP_ERR_INVALID;
  if (kernel_ms) *kernel_ms = c->form_ms[form];
  if (launches) *launches = c->form_n[form];
  return CILHIP_OK;
}

int cilhip_get_last_run_trace(cilhip_ctx* c, int cap, int* n_out, unsigned int* unproven, unsigned int* listed, float* step, float* delta, int* form) {
  if (!c || !n_out || cap < 0) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  IcpState hs;
  CK(c, hipMemcpyAsync(&hs, c->d_state, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  uint4 tr[RUN_TRACE_CAP];
  CK(c, hipMemcpyAsync(tr, c->d_trace, sizeof(tr), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  const int n = std::min(std::min(hs.iterations, (int)RUN_TRACE_CAP), cap);
  for (int i = 0; i < n; ++i) {
    if (unproven) unproven[i] = tr[i].x;
    if (listed) listed[i] = tr[i].y;
    if (step) memcpy(&step[i], &tr[i].z, 4);
    if (delta) memcpy(&delta[i], &tr[i].w, 4);
    if (form) form[i] = (size_t)i < c->trace_form.size() ? (int)(c->trace_form[i] & FORM_MASK) : -1;
  }
  *n_out = n;
  return CILHIP_OK;
}

int cilhip_get_last_warm_iterations(cilhip_ctx* c, int* warm_iterations) {
  if (!c || !warm_iterations) return CILHIP_ERR_INVALID;
  *warm_iterations = c->last_warm_iters;
  return CILHIP_OK;
}

int cilhip_get_last_reverse_fused_iterations(cilhip_ctx* c, int* fused_iterations) {
  if (!c || !fused_iterations) return CILHIP_ERR_INVALID;
  *fused_iterations = c->last_rev_fused_iters;
  return CILHIP_OK;
}

int cilhip_get_last_run_forms(cilhip_ctx* c, int* one_pass_iterations, int* two_pass_iterations) {
  if (!c) return CILHIP_ERR_INVALID;
  if (one_pass_iterations) *one_pass_iterations = c->last_fused_iters;
  if (two_pass_iterations) *two_pass_iterations = c->last_two_pass_iters;
  return CILHIP_OK;
}

int cilhip_enable_kernel_timing(cilhip_ctx* c, int on) {
  if (!c) return CILHIP_ERR_INVALID;
  c->kernel_timing = on != 0;
  return CILHIP_OK;
}

static int upload(cilhip_ctx* c, const float* src, size_t count, int mem, DevBuf<float>& d_out) {
  CK(c, d_out.alloc(count));
  if (count)
    CK(c, hipMemcpyAsync(d_out, src, count * sizeof(float), mem == CILHIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
  return CILHIP_OK;
}

int cilhip_set_target(cilhip_ctx* c, const float* xyz, const float* nrm, size_t n, int mem) {
  if (!c) return CILHIP_ERR_INVALID;
  if ((n && !xyz) || n >= 0xFFFFFFF0ull) return fail(c, CILHIP_ERR_INVALID, "set_target: bad cloud (null or >= 2^32-16 points)");
  CK(c, hipSetDevice(c->device));
  auto t0 = std::chrono::steady_clock::now();
  release_target(c);      // (incl. the order tables, the nearest-other-point table, the colours: they describe ONE target; a shared target is only let go of)
  DevBuf<float> d_xyz, d_nrm;
  int rc = upload(c, xyz, 3 * n, mem, d_xyz);
  if (rc) return rc;
  if (nrm) { rc = upload(c, nrm, 3 * n, mem, d_nrm); if (rc) return rc; }
  GridBuildResult r{};
  double mean[3];
  hipError_t e = build_grid(d_xyz, d_nrm, (uint32_t)n, c->stream, &r, mean, c->cell_occupancy, c->refined_occupancy);
  d_xyz.reset(); d_nrm.reset();
  if (e == GRID_RANGE_ERROR) { c->err = std::string("set_target: ") + kGridRangeMessage; return CILHIP_ERR_UNSUPPORTED; }
  if (e != hipSuccess) { c->err = std::string("build_grid: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  c->grid = r.grid; c->grid_store = std::move(r.store); c->grid_occ = r.avg_occupancy; c->grid_cells = r.n_cells;
  c->policy.warm_banned = false;
  c->has_normals = (nrm != nullptr);
  for (int i = 0; i < 3; ++i) c->dst_mean[i] = (float)mean[i];
  c->partial_target = false;      // (a new target stands for itself until cilhip_set_shard_info says otherwise)
  c->has_target = true;
  c->src_sorted = false;  // source order is tied to the target grid
  drop_correspondences(c);
  c->policy.far_mode = true;
  c->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return CILHIP_OK;
}

// CorrespondenceSearchKDTree::getFirstSearchTree / setFirstSearchTree (correspondence_search_kd_tree.hpp:273-296): a second engine
// takes the index another one built instead of building its own.  Here: `c` takes `from`'s target as it stands -- the sorted
// points and normals, the cell table, and whatever has been built on top of them by now (the paired point+normal records, the
// nearest-other-point table, the order tables of the reference's tree, the index -> position map) -- without copying a byte.  Every
// one of those arrays is reference-counted by itself (SharedBuf): either context may be destroyed or given another target first, an
// array goes when its last holder lets go.  What one of them builds LATER (tables a run finds it needs) is its own.
int cilhip_share_target(cilhip_ctx* c, cilhip_ctx* from) {
  if (!c || !from || c == from) return CILHIP_ERR_INVALID;
  if (!from->has_target) return fail(c, CILHIP_ERR_INVALID, "share_target: the other context has no target");
  if (c->device != from->device) return fail(c, CILHIP_ERR_INVALID, "share_target: the two contexts live on different devices");
  CK(c, hipSetDevice(c->device));
  CK(c, hipStreamSynchronize(from->stream));      // (whatever is still building the lender's tables)
  CK(c, hipStreamSynchronize(c->stream));
  release_target(c);
  c->grid = from->grid; c->grid_store = from->grid_store; c->has_target = true; c->has_normals = from->has_normals;
  c->grid_occ = from->grid_occ; c->grid_cells = from->grid_cells; c->build_ms = 0.0;
  for (int i = 0; i < 3; ++i) c->dst_mean[i] = from->dst_mean[i];
  c->index_offset = from->index_offset; c->partial_target = from->partial_target;
  c->d_inv_perm = from->d_inv_perm; c->d_safe2 = from->d_safe2;
  c->d_tie_leaf_slot = from->d_tie_leaf_slot; c->d_tie_nodes = from->d_tie_nodes; c->tie_max_depth = from->tie_max_depth;
  c->policy.warm_banned = false;
  c->src_sorted = false;  // source order is tied to the target grid
  drop_correspondences(c);
  c->policy.far_mode = true;
  return CILHIP_OK;
}

int cilhip_set_source(cilhip_ctx* c, const float* xyz, size_t n, int mem) {
  if (!c) return CILHIP_ERR_INVALID;
  if ((n && !xyz) || n >= 0xFFFFFFF0ull) return fail(c, CILHIP_ERR_INVALID, "set_source: bad cloud");
  CK(c, hipSetDevice(c->device));
  free_source(c);
  int rc = upload(c, xyz, 3 * n, mem, c->d_src_xyz);
  if (rc) return rc;
  CK(c, c->d_src_sorted.alloc(n));
  CK(c, c->d_nn_pos.alloc(n));
  CK(c, c->d_nn_d2.alloc(n));
  c->ns = (uint32_t)n;
  double mean[3];
  float lo[3], hi[3];
  hipError_t e = mean3_device(c->d_src_xyz, c->ns, c->stream, mean, lo, hi);
  if (e != hipSuccess) { c->err = std::string("mean3: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  for (int i = 0; i < 3; ++i) {
    c->src_mean[i] = (float)mean[i];
    // (centre and half extent rounded so that the box holds every point: the half extent is taken from the rounded centre)
    c->src_center[i] = 0.5f * (lo[i] + hi[i]);
    c->src_half[i] = c->ns ? std::max(hi[i] - c->src_center[i], c->src_center[i] - lo[i]) * 1.000001f : 0.0f;
    if (!(c->src_half[i] >= 0.0f) || !std::isfinite(c->src_center[i])) { c->src_center[i] = 0.0f; c->src_half[i] = 1.0e30f; }   // (non-finite coordinates: no bound)
  }
  const int nb = std::max(iter_num_blocks(c->ns), warm_num_blocks(c->ns));      // rows of partial sums: the streaming and the warm-started kernels
  rc = ensure_partial_rows(c, (size_t)nb);
  if (rc) return rc;
  c->has_source = true;
  return CILHIP_OK;
}

int cilhip_set_source_normals(cilhip_ctx* c, const float* nrm, int mem) {
  if (!c) return CILHIP_ERR_INVALID;
  if (!c->has_source) return fail(c, CILHIP_ERR_INVALID, "set_source_normals: set_source first");
  CK(c, hipSetDevice(c->device));
  c->d_src_nrm.reset();
  c->d_src_nrm_sorted.reset();
  c->have_pairs = false;
  drop_src_grid(c);      // (it carries the feature vectors of the reverse searches)
  if (!nrm) return CILHIP_OK;                              // back to the 3-cloud (non-symmetric) form
  int rc = upload(c, nrm, 3 * (size_t)c->ns, mem, c->d_src_nrm);
  if (rc) return rc;
  c->src_nrm0[0] = c->src_nrm0[1] = c->src_nrm0[2] = 0.0f;
  if (c->ns) {
    CK(c, hipMemcpyAsync(c->src_nrm0, c->d_src_nrm, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  }
  CK(c, c->d_src_nrm_sorted.alloc(c->ns));
  c->src_sorted = false;                                   // the sorted copy is (re)built with the next sort
  drop_correspondences(c);
  return CILHIP_OK;
}

int cilhip_set_color_features(cilhip_ctx* c, const float* dst_rgb, const float* src_rgb, int mem) {
  if (!c) return CILHIP_ERR_INVALID;
  if (!c->has_target || !c->has_source) return fail(c, CILHIP_ERR_INVALID, "set_color_features: set_target and set_source first");
  if (!dst_rgb || !src_rgb) return fail(c, CILHIP_ERR_INVALID, "set_color_features: both clouds' colours are needed");
  CK(c, hipSetDevice(c->device));
  c->d_dst_rgb.reset();
  c->d_src_rgb.reset();
  c->d_src_rgb_sorted.reset();
  int rc = upload(c, dst_rgb, 3 * (size_t)c->grid.n, mem, c->d_dst_rgb);
  if (rc) return rc;
  rc = upload(c, src_rgb, 3 * (size_t)c->ns, mem, c->d_src_rgb);
  if (rc) return rc;
  CK(c, c->d_src_rgb_sorted.alloc(c->ns));
  c->dst_rgb_sorted_ok = false;
  c->src_sorted = false;                                   // the source's sorted copy is (re)built with the next sort
  drop_src_grid(c);      // (it carries the features of the reverse searches)
  drop_feat_tie_tables(c);      // (the colours are coordinates of the feature tree)
  drop_correspondences(c);
  return CILHIP_OK;
}

int cilhip_get_means(cilhip_ctx* c, float dm[3], float sm[3]) {
  if (!c) return CILHIP_ERR_INVALID;
  if (dm) memcpy(dm, c->dst_mean, sizeof(c->dst_mean));
  if (sm) memcpy(sm, c->src_mean, sizeof(c->src_mean));
  return CILHIP_OK;
}

// The rows of partial sums the accumulating kernels write (SUMS_MAX doubles each): grown, never shrunk (DevBuf::ensure: a failed
// allocation leaves nothing stale behind).
int cilhip::ensure_partial_rows(cilhip_ctx* c, size_t rows) {
  CK(c, c->d_partials.ensure(rows * SUMS_MAX));
  return CILHIP_OK;
}

// Spatially sort the source under T (once; re-sorted only if the transform moved it by more than a few cells).
int cilhip::ensure_sorted(cilhip_ctx* c, const float T[16]) {
  if (!c->has_target || !c->has_source) return fail(c, CILHIP_ERR_INVALID, "set_target and set_source first");
  bool need = !c->src_sorted;
  if (!need) {
    // displacement of the source bbox centre proxy: compare transforms on the source mean
    float a[3], b[3];
    transform_point(T, c->src_mean[0], c->src_mean[1], c->src_mean[2], a[0], a[1], a[2]);
    transform_point(c->sort_T, c->src_mean[0], c->src_mean[1], c->src_mean[2], b[0], b[1], b[2]);
    float dl = 0.f;
    for (int i = 0; i < 3; ++i) dl = fmaxf(dl, fabsf(a[i] - b[i]));
    float dr = 0.f;
    for (int i = 0; i < 11; ++i) if (i % 4 != 3) dr = fmaxf(dr, fabsf(T[i] - c->sort_T[i]));
    const float ext = fmaxf(c->grid.nx, fmaxf(c->grid.ny, c->grid.nz)) * c->grid.cell;
    if (dl > 4.0f * c->grid.cell || dr * ext > 4.0f * c->grid.cell) need = true;
  }
  if (need) {
    // (scratch, tile table and the per-tile arrays are kept between the sorts of a source: a re-sort costs its kernels only)
    c->d_tiles = nullptr; c->d_tile_center = nullptr; c->ntiles = 0;
    hipError_t e = sort_source(c->d_src_xyz, c->ns, c->grid, T, c->d_src_sorted, c->stream, &c->d_tiles, &c->d_tile_center, c->tile_axes, &c->ntiles, c->sort_ws);
    if (e != hipSuccess) { c->err = std::string("sort_source: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
    if (((size_t)c->ntiles + 1) * 8 > c->d_tile_box.capacity() || !c->d_defer_mask) {      // (sized together, with room to grow)
      c->d_tile_box.reset();
      c->d_defer_mask.reset();
      const size_t cap = (size_t)c->ntiles + 1 + c->ntiles / 8;
      CK(c, c->d_defer_mask.alloc(cap * 2 * (TILE_THREADS / 64)));
      CK(c, c->d_tile_box.alloc(cap * 8));
    }
    CK(c, hipMemsetAsync(c->d_defer_mask, 0, ((size_t)c->ntiles + 1) * 2 * (TILE_THREADS / 64) * sizeof(unsigned long long), c->stream));
    {   // the tiled search with in-tile accumulation leaves one row of partial sums per tile and per block of its clean-up pass
      const int rows = std::max(std::max(iter_num_blocks(c->ns), warm_num_blocks(c->ns)), tiled_partial_rows(c->ntiles));
      const int rc = ensure_partial_rows(c, (size_t)rows);
      if (rc) return rc;
    }
    if (c->d_src_nrm) launch_gather_by_w(c->d_src_sorted, c->d_src_nrm, c->ns, c->d_src_nrm_sorted, c->stream);
    if (c->d_src_rgb) launch_gather_by_w(c->d_src_sorted, c->d_src_rgb, c->ns, c->d_src_rgb_sorted, c->stream);
    c->d_src_inv.reset();
    c->d_grid_to_sorted.reset();
    memcpy(c->sort_T, T, sizeof(c->sort_T));
    c->src_sorted = true;
    c->src3_valid = false; c->rec_valid = false; c->lb_fresh = false;     // (per sorted order)
    drop_matches(c);      // (the matches alone: a pair list carries its own views of the source)
  }
  return CILHIP_OK;
}

int cilhip_prepare_source(cilhip_ctx* c, const float* T, int force, double* ms) {
  if (!c) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  CK(c, hipStreamSynchronize(c->stream));
  const auto t0 = std::chrono::steady_clock::now();
  if (force) c->src_sorted = false;
  const int rc = ensure_sorted(c, T ? T : kIdentity16);
  if (rc) return rc;
  CK(c, hipStreamSynchronize(c->stream));
  if (ms) *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return CILHIP_OK;
}

// the matches records / margin keys / 12-byte source copy of the warm-started iterations: allocated by the first run that can use them
int cilhip::ensure_warm_buffers(cilhip_ctx* c) {
  const size_t cap = c->ns ? c->ns : 1;
  if (!c->d_warm_rec) { CK(c, c->d_warm_rec.alloc((cap * (sizeof(float4) + 2 * sizeof(F3)) + sizeof(float4) - 1) / sizeof(float4))); c->src3_valid = false; }      // (one allocation, three views: set_warm_args)
  if (!c->d_nn_lb) CK(c, c->d_nn_lb.alloc(cap));
  if (!c->src3_valid) {
    launch_copy_src3(c->d_src_sorted, c->ns, reinterpret_cast<F3*>(c->d_warm_rec + cap) + cap, c->stream);
    c->src3_valid = true;
  }
  return CILHIP_OK;
}
// {point, normal} of every target position side by side (GridDev::pn), for the streaming accumulation's gathers: built by the first run
// that streams over stored matches with a metric that reads normals (32 B per target point; without room for it the two arrays serve)
void cilhip::ensure_pair_records(cilhip_ctx* c) {
  if (c->grid.pn || !c->pair_records || !c->grid.nrm || !c->grid.n) return;
  if (c->grid_store.pn.alloc((size_t)c->grid.n * 2) != hipSuccess) { (void)hipGetLastError(); return; }      // (without room for it the two arrays serve)
  launch_interleave_pn(c->grid.pts, c->grid.nrm, c->grid.n, c->grid_store.pn, c->stream);
  c->grid.pn = c->grid_store.pn;
}
void cilhip::set_warm_args(const cilhip_ctx* c, IterArgs& wa) {
  const size_t cap = c->ns ? c->ns : 1;
  wa.warm_extra = c->warm_extra;
  wa.warm_rec = c->d_warm_rec;
  wa.warm_rec_n = reinterpret_cast<F3*>(c->d_warm_rec + cap);
  wa.warm_src3 = wa.warm_rec_n + cap;
}
// k_self_nn's nearest-other-point table (4 B per target point, 0.5 ms at 10M): built by the first warm-capable run on a target
int cilhip::ensure_safe2(cilhip_ctx* c) {
  if (c->d_safe2) return CILHIP_OK;
  CK(c, c->d_safe2.alloc(c->grid.n));
  launch_self_nn(c->grid, c->d_safe2, c->stream);
  return CILHIP_OK;
}

// filterCorrespondencesFraction then filterCorrespondencesOneToOne on the stored matches
int cilhip::apply_filters(cilhip_ctx* c) {
  if (!filters_active(c) || c->ns == 0) return CILHIP_OK;
  if (c->inlier_fraction > 0.0 && c->inlier_fraction < 1.0) {
    if (!c->d_keys) CK(c, c->d_keys.alloc(c->ns));
    if (!c->d_sel_state) CK(c, c->d_sel_state.alloc(filter_state_bytes()));
    launch_filter_fraction(c->d_src_sorted, c->d_nn_pos, c->d_nn_d2, c->ns, c->inlier_fraction, c->d_keys, c->d_sel_state, c->stream);
  }
  if (c->one_to_one && c->grid.n) {
    if (!c->d_winner) CK(c, c->d_winner.alloc(c->grid.n));
    launch_filter_one_to_one(c->d_src_sorted, c->d_nn_pos, c->d_nn_d2, c->ns, c->d_winner, c->grid.n, c->stream);
  }
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

// The 6-D feature search's inputs: vectors (normals or colours), weight, and how the source's part follows the transform being
// searched under (FeatSpec::mode; M = L^-T of that transform is refreshed by cilhip_find_correspondences -- the affine loops are
// host-driven, the device-resident loops are rigid).
FeatSpec cilhip::feat_spec_of(const cilhip_ctx* c) {
  FeatSpec f{};
  f.w = c->normal_weight;
  f.enabled = feat6(c) ? 1 : 0;
  if (c->feature_kind == 1) { f.src = c->d_src_rgb_sorted; f.dst = c->d_dst_rgb_sorted; f.mode = 2; }
  else { f.src = c->d_src_nrm ? c->d_src_nrm_sorted : nullptr; f.dst = c->grid.nrm; f.mode = c->transform_mode == 1 ? 1 : 0; }
  if (c->feature_kind == 2) { f.src2 = c->d_src_rgb_sorted; f.dst2 = c->d_dst_rgb_sorted; f.w2 = c->color_weight; }
  for (int i = 0; i < 9; ++i) f.M[i] = c->feat_M[i];
  // normal_weight = the norm of the FIRST source feature's normal part (adaptors.hpp:113-114), f32
  const float x = c->normal_weight * c->src_nrm0[0], y = c->normal_weight * c->src_nrm0[1], z = c->normal_weight * c->src_nrm0[2];
  f.nw = std::sqrt(x * x + (y * y + z * z));
  return f;
}
// sorted copy of the target's colour features (gathered by the sorted records' original indices), built on first use
int cilhip::ensure_feature_arrays(cilhip_ctx* c) {
  if (c->feature_kind == 0) return CILHIP_OK;
  if (!c->d_dst_rgb || !c->d_src_rgb) return fail(c, CILHIP_ERR_INVALID, "colour features: cilhip_set_color_features first");
  if (!c->dst_rgb_sorted_ok) {
    if (!c->d_dst_rgb_sorted) CK(c, c->d_dst_rgb_sorted.alloc(c->grid.n));
    launch_gather_by_w(c->grid.pts, c->d_dst_rgb, c->grid.n, c->d_dst_rgb_sorted, c->stream);
    c->dst_rgb_sorted_ok = true;
  }
  return CILHIP_OK;
}

IterArgs cilhip::make_iter_args(cilhip_ctx* c, float max_sq) {
  IterArgs a{};
  a.grid = c->grid;
  a.src = c->d_src_sorted;
  a.src_nrm = (c->d_src_nrm && c->symmetric) ? c->d_src_nrm_sorted : nullptr;
  a.feat = feat_spec_of(c);
  a.ns = c->ns;
  a.max_sq = max_sq;
  for (int i = 0; i < 3; ++i) a.dst_mean[i] = c->dst_mean[i];
  for (int i = 0; i < 9; ++i) a.tile_axes[i] = c->tile_axes[i];
  a.state = c->d_state;
  a.nn_pos = c->d_nn_pos;
  a.nn_d2 = c->d_nn_d2;
  a.partials = c->d_partials;
  a.defer_mask = c->d_defer_mask;
  a.tile_partials = c->d_partials;            // (in-tile accumulation: tile rows first, then the clean-up pass's rows)
  a.defer_flag = c->d_defer_flag;
  a.unproven_cnt = c->d_unproven;
  a.store_matches = 1;
  a.skip_if_inner_done = 0;
  a.tie = tie_dev_of(c);
  return a;
}

// The SECOND_TO_FIRST search under the transform held by c->d_state: LDS-tiled or per-lane kernel for point features, the
// 6-D feature search when a normal weight is set.
int cilhip::launch_search(cilhip_ctx* c, const IterArgs& a, int lanes) {
  if (lanes < 0) lanes = c->group_lanes > 0 ? c->group_lanes : 0;
  if (feat6(c)) {
    if (c->feature_kind != 1 && (!c->has_normals || !c->d_src_nrm)) return fail(c, CILHIP_ERR_INVALID, "point+normal features need target and source normals");
    if (c->feature_kind == 1 && (!a.feat.src || !a.feat.dst)) return fail(c, CILHIP_ERR_INVALID, "colour features: cilhip_set_color_features first");
    if (c->feature_kind == 2 && (!a.feat.src2 || !a.feat.dst2)) return fail(c, CILHIP_ERR_INVALID, "point+normal+colour features: cilhip_set_color_features first");
    if (c->index_offset) return fail(c, CILHIP_ERR_UNSUPPORTED, "feature adaptors are not available on target shards");
    if (use_tiled(c)) launch_search_tiled_feat6(a, c->d_tiles, c->d_tile_center, c->d_tile_box, c->ntiles, c->stream);
    else launch_search_feat6(a, c->stream);
    return CILHIP_OK;
  }
  if (use_tiled(c)) launch_search_tiled(a, IM_NONE, c->d_tiles, c->d_tile_center, c->d_tile_box, c->ntiles, c->stream);   // LDS-tiled search kernel
  else if (lanes) launch_search_group(a, lanes, c->stream);                                                    // several lanes per query (a.warm_pos: the previous matches bound the search)
  else launch_iter(a, IM_NONE, true, true, iter_num_blocks(c->ns), c->stream);                                 // per-lane global-memory search
  return CILHIP_OK;
}

// Search directions FIRST_TO_SECOND / BOTH with the transform held by c->d_state: fills c->pairs (post-filters included).
// the source's own grid (source coordinates) and what else the list-free FIRST_TO_SECOND / BOTH loop needs
static int ensure_src_grid(cilhip_ctx* c) {
  if (!c->has_src_grid && c->ns) {
    // the source indexed once, in its own coordinates (the reference builds a kd-tree over T*src per search): the reverse
    // searches go through the inverse transform
    GridBuildResult r{};
    double mean[3];
    // (its per-point attribute = the feature vectors a 6-D reverse search compares by: normals or colours)
    const float* attr = c->feature_kind == 1 ? c->d_src_rgb : c->d_src_nrm;
    const hipError_t eg = build_grid(c->d_src_xyz, attr, c->ns, c->stream, &r, mean, 1.0);
    if (eg == GRID_RANGE_ERROR) { c->err = std::string("source grid: ") + kGridRangeMessage; return CILHIP_ERR_UNSUPPORTED; }
    if (eg != hipSuccess) { c->err = std::string("build_grid (source): ") + hipGetErrorString(eg); return CILHIP_ERR_HIP; }
    c->src_grid = r.grid; c->src_grid_store = std::move(r.store); c->has_src_grid = true;
  }
  if (c->has_src_grid && c->feature_kind == 2 && c->d_src_rgb && !c->d_src_rgb_grid) {      // 9-D: the colours in the same order
    CK(c, c->d_src_rgb_grid.alloc(c->ns));
    launch_gather_by_w(c->src_grid.pts, c->d_src_rgb, c->ns, c->d_src_rgb_grid, c->stream);
  }
  return CILHIP_OK;
}

int cilhip::ensure_reverse_buffers(cilhip_ctx* c) {
  const int rc = ensure_src_grid(c);
  if (rc) return rc;
  if (!c->d_rev_pos) {
    CK(c, c->d_rev_pos.alloc(c->grid.n));
    CK(c, c->d_rev_d2.alloc(c->grid.n));
  }
  if (!c->d_src_safe2 && c->has_src_grid && c->reverse_warm) {      // (lives and dies with the source grid: drop_src_grid)
    CK(c, c->d_src_safe2.alloc(c->ns));
    launch_self_nn(c->src_grid, c->d_src_safe2, c->stream);
  }
  if (!c->d_src_inv) {      // original source index -> position in the cube-sorted source (the forward matches are stored by that)
    CK(c, c->d_src_inv.alloc(c->ns));
    launch_inv_perm(c->d_src_sorted, c->ns, c->d_src_inv, c->stream);
  }
  if (!c->d_grid_to_sorted && c->has_src_grid) {
    CK(c, c->d_grid_to_sorted.alloc(c->ns));
    launch_grid_to_sorted(c->src_grid.pts, c->ns, c->d_src_inv, c->d_grid_to_sorted, c->stream);
  }
  return CILHIP_OK;
}

int cilhip::run_pair_search(cilhip_ctx* c, const IterArgs& a, float max_sq, const float T_host[16]) {
  if (!c->d_state_id) {
    CK(c, c->d_state_id.alloc(1));
    const float zero[3] = {0, 0, 0};
    launch_init_state(c->d_state_id, kIdentity16, zero, c->stream);
  }
  if (c->search_dir == 2 && c->ns && c->grid.n) {   // forward half of BOTH: the usual search, no filters yet
    const int src_rc = launch_search(c, a);
    if (src_rc) return src_rc;
  }
  { const int grc = ensure_src_grid(c); if (grc) return grc; }
  FeatSpec rf = a.feat;                              // the reverse search reads the source's features in the source grid's order
  rf.src = c->has_src_grid ? c->src_grid.nrm : nullptr;
  if (rf.dst2) rf.src2 = c->d_src_rgb_grid;
  if (feat6(c) && (!rf.src || !rf.dst || (rf.dst2 && !rf.src2))) return fail(c, CILHIP_ERR_INVALID, "feature search: both clouds' feature vectors are needed");
  if (!feat6(c)) { rf.w = 0.0f; rf.enabled = 0; }
  if (c->rev_tie_aware && tie_mode_on(c)) { const int trc = build_rev_tie_tables(c, T_host); if (trc) return trc; }
  const TieDev rt = tie_dev_rev(c);
  const hipError_t e = find_pairs(rf, c->grid, c->src_grid, c->d_src_xyz, (c->d_src_nrm && c->symmetric) ? c->d_src_nrm : nullptr, c->d_src_sorted, c->ns, c->d_state,
                                  c->d_state_id, T_host, max_sq, c->search_dir, c->reciprocal, c->inlier_fraction, c->one_to_one, c->d_nn_pos, c->d_nn_d2,
                                  c->pairs, c->stream, &rt);
  if (e == GRID_RANGE_ERROR) { c->err = std::string("find_pairs (grid over the transformed source): ") + kGridRangeMessage; return CILHIP_ERR_UNSUPPORTED; }
  if (e != hipSuccess) { c->err = std::string("find_pairs: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  return CILHIP_OK;
}

const char* cilhip::proj_conflict(const cilhip_ctx* c) {
  if (c->search_dir != 0 || c->reciprocal) return "projective search: SECOND_TO_FIRST only (no other search direction, no reciprocity)";
  if (c->one_to_one) return "projective search: the one-to-one filter is not available";
  if (feat6(c)) return "projective search: feature adaptors are not available";
  if (c->weight_fn) return "projective search: the pair-weight callback is not available";
  if (c->index_offset || c->partial_target || c->guard_axis >= 0) return "projective search: not available on slab or target shards";
  return nullptr;
}

int cilhip::ensure_proj_map(cilhip_ctx* c) {
  if (c->d_proj_map) return CILHIP_OK;
  const size_t npix = (size_t)c->proj.w * c->proj.h;
  CK(c, c->d_proj_keys.alloc(npix));
  CK(c, c->d_proj_map.alloc(npix));
  const hipError_t e = launch_proj_map(c->grid.pts, c->grid.n, c->proj, c->d_proj_keys, c->d_proj_map, c->stream);
  if (e != hipSuccess) { c->d_proj_map.reset(); c->err = std::string("projective index map: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  return CILHIP_OK;
}

int cilhip_set_projection(cilhip_ctx* c, const float* K, size_t w, size_t h, const float* E) {
  if (!c) return CILHIP_ERR_INVALID;
  if (K) {
    for (int i = 0; i < 9; ++i) if (!std::isfinite(K[i])) return fail(c, CILHIP_ERR_INVALID, "set_projection: the intrinsic matrix has a non-finite entry");
    if (w == 0 || h == 0 || w >= 0xFFFFFFF0ull || h >= 0xFFFFFFF0ull || (unsigned long long)w * h >= 0xFFFFFFF0ull)
      return fail(c, CILHIP_ERR_INVALID, "set_projection: w * h must be positive and below 2^32 - 16");
  }
  CK(c, hipSetDevice(c->device));
  CK(c, hipStreamSynchronize(c->stream));      // (a search may still be reading the map)
  c->d_proj_map.reset(); c->d_proj_keys.reset();
  drop_matches(c);      // (the matches alone: a projection never runs with the pair-list directions)
  c->proj_on = K != nullptr;
  if (!K) return CILHIP_OK;
  ProjDev& p = c->proj;
  p = ProjDev{};
  p.has_cam = E != nullptr;
  if (E)      // to_cam = (R^T, -R^T t), formed in f64 from the f32 entries, rounded once (rule P1)
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) p.L[3 * r + k] = E[k + 4 * r];
      p.t[r] = (float)-((double)E[0 + 4 * r] * (double)E[12] + ((double)E[1 + 4 * r] * (double)E[13] + (double)E[2 + 4 * r] * (double)E[14]));
    }
  for (int j = 0; j < 3; ++j) { p.k0[j] = K[0 + 3 * j]; p.k1[j] = K[1 + 3 * j]; }
  p.w = (uint32_t)w; p.h = (uint32_t)h;
  return CILHIP_OK;
}

int cilhip_find_correspondences(cilhip_ctx* c, const float T[16], float max_sq, size_t* n_found) {
  if (!c || !T) return CILHIP_ERR_INVALID;
  if (c->proj_on) { if (const char* why = proj_conflict(c)) return fail(c, CILHIP_ERR_UNSUPPORTED, why); }
  CK(c, hipSetDevice(c->device));
  int rc = ensure_sorted(c, T);
  if (rc) return rc;
  rc = tie_prepare(c, "find_correspondences");
  if (rc) return rc;
  launch_init_state(c->d_state, T, c->src_mean, c->stream, nullptr, 0, nullptr, nullptr, c->d_tie_counters);
  if (feat6(c)) {
    rc = ensure_feature_arrays(c);
    if (rc) return rc;
    linear_inverse_transpose_f32(T, c->feat_M);
  }
  IterArgs a = make_iter_args(c, max_sq);
  if (c->search_dir != 0) {
    if (c->index_offset) return fail(c, CILHIP_ERR_UNSUPPORTED, "search directions other than SECOND_TO_FIRST are not available on target shards");
    rc = run_pair_search(c, a, max_sq, T);
    if (rc) return rc;
    {      // (ties met without tables -- the forward half of BOTH: the target's; the reverse matches: the transformed source's --: once more with them)
      bool again = false;
      rc = tie_check_pending(c, &again);
      if (rc) return rc;
      if (again) { a = make_iter_args(c, max_sq); rc = run_pair_search(c, a, max_sq, T); if (rc) return rc; }
    }
    memcpy(c->nn_T, T, sizeof(c->nn_T));
    drop_matches(c);
    c->have_pairs = true;
    c->matches_origin = 3;
    if (n_found) *n_found = c->pairs.count;
    return CILHIP_OK;
  }
  c->have_pairs = false;
  if (c->proj_on) {
    rc = ensure_proj_map(c);
    if (rc) return rc;
    launch_proj_search(c->d_src_sorted, c->ns, c->d_state, c->grid.pts, c->proj, c->d_proj_map, max_sq, c->d_nn_pos, c->d_nn_d2, c->stream);
  } else if (c->ns) {
    rc = launch_search(c, a);
    if (rc) return rc;
    bool again = false;      // (tie_rule 2: the search met ties and there were no order tables yet -- they exist now: once more)
    rc = tie_check_pending(c, &again);
    if (rc) return rc;
    if (again) { a = make_iter_args(c, max_sq); rc = launch_search(c, a); if (rc) return rc; }
  }
  CK(c, hipGetLastError());
  rc = apply_filters(c);
  if (rc) return rc;
  memcpy(c->nn_T, T, sizeof(c->nn_T));
  c->pending_matches = false;
  c->have_nn = true; c->d2_stale = false;
  c->matches_origin = 3;
  if (n_found) {
    unsigned long long cnt = 0;
    launch_count_found(c->d_nn_pos, c->ns, c->d_count, c->stream);
    CK(c, hipMemcpyAsync(&cnt, c->d_count, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    *n_found = (size_t)cnt;
  }
  return CILHIP_OK;
}

// nn_d2 of the matches a loop left behind (finish_run_matches), with the search's pinned arithmetic under the transform they were found under
static int ensure_d2(cilhip_ctx* c) {
  if (!c->d2_stale || !c->have_nn) return CILHIP_OK;
  CK(c, hipSetDevice(c->device));
  if (c->ns) launch_fill_d2(c->d_src_sorted, c->grid.pts, c->d_nn_pos, c->nn_T, c->ns, c->d_nn_d2, c->stream);
  c->d2_stale = false;
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

static int scatter_to_original(cilhip_ctx* c) {
  { const int drc = ensure_d2(c); if (drc) return drc; }
  const size_t cap = c->ns ? c->ns : 1;
  if (!c->d_out_idx) CK(c, c->d_out_idx.alloc(cap));
  if (!c->d_out_d2) CK(c, c->d_out_d2.alloc(cap));
  launch_scatter_nn(c->d_src_sorted, c->grid.pts, c->d_nn_pos, c->d_nn_d2, c->ns, c->d_out_idx, c->d_out_d2, c->stream);
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

// The correspondence set of the last executed iteration of cilhip_icp_run, when the loop's kernels did not leave it in memory
// (post-filters, pair-list directions, feature search, forms that store no matches): searched again under the transform that
// iteration searched under.  The search is exact and deterministic: the same set.
int cilhip::materialize_pending(cilhip_ctx* c) {
  if (!c->pending_matches) return ensure_d2(c);      // (matches a loop left in place: their distances are formed now, if not yet)
  float T[16];
  memcpy(T, c->nn_T, sizeof(T));
  const float r = c->pending_max_sq;
  c->pending_matches = false;
  // (the search runs through the context's loop state: the finished run's state -- what cilhip_icp_state and
  //  cilhip_get_slab_violation_state report -- is put back afterwards)
  DevBuf<IcpState> keep;
  CK(c, keep.alloc(1));
  hipError_t e = hipMemcpyAsync(keep, c->d_state, sizeof(IcpState), hipMemcpyDeviceToDevice, c->stream);
  int rc = e == hipSuccess ? cilhip_find_correspondences(c, T, r, nullptr) : CILHIP_ERR_HIP;
  if (e == hipSuccess) e = hipMemcpyAsync(c->d_state, keep, sizeof(IcpState), hipMemcpyDeviceToDevice, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess && rc == CILHIP_OK) { c->err = std::string("materialize_pending: ") + hipGetErrorString(e); rc = CILHIP_ERR_HIP; }
  if (rc == CILHIP_OK) c->matches_origin = 2;
  return rc;
}

int cilhip_get_last_matches_origin(cilhip_ctx* c, int* origin) {
  if (!c || !origin) return CILHIP_ERR_INVALID;
  *origin = c->matches_origin;
  return CILHIP_OK;
}

int cilhip_get_matches_transform(cilhip_ctx* c, float T[16]) {
  if (!c || !T) return CILHIP_ERR_INVALID;
  if (!c->have_nn && !c->have_pairs && !c->pending_matches) return fail(c, CILHIP_ERR_INVALID, "get_matches_transform: no search has been run");
  memcpy(T, c->nn_T, sizeof(c->nn_T));
  return CILHIP_OK;
}

int cilhip_get_nn(cilhip_ctx* c, uint32_t* nn_idx, float* nn_d2, int mem) {
  if (!c) return CILHIP_ERR_INVALID;
  { const int prc = materialize_pending(c); if (prc) return prc; }
  if (c->have_pairs) return fail(c, CILHIP_ERR_UNSUPPORTED, "get_nn: the last search ran in a direction whose result is a pair list; use get_correspondences");
  if (!c->have_nn) return fail(c, CILHIP_ERR_INVALID, "get_nn: no search has been run");
  CK(c, hipSetDevice(c->device));
  int rc = scatter_to_original(c);
  if (rc) return rc;
  const hipMemcpyKind k = mem == CILHIP_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  if (nn_idx && c->ns) CK(c, hipMemcpyAsync(nn_idx, c->d_out_idx, (size_t)c->ns * 4, k, c->stream));
  if (nn_d2 && c->ns) CK(c, hipMemcpyAsync(nn_d2, c->d_out_d2, (size_t)c->ns * 4, k, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}

static int get_correspondences_impl(cilhip_ctx* c, uint64_t* i1, uint64_t* i2, float* val, size_t cap, size_t* n_out);
int cilhip_get_correspondences(cilhip_ctx* c, uint64_t* i1, uint64_t* i2, float* val, size_t cap, size_t* n_out) {
  if (!c || !n_out) return CILHIP_ERR_INVALID;
  // (host vectors of the size of the source: an allocation failure must not cross the C boundary)
  try { return get_correspondences_impl(c, i1, i2, val, cap, n_out); }
  catch (const std::bad_alloc&) { return fail(c, CILHIP_ERR_HIP, "get_correspondences: out of host memory"); }
  catch (...) { return fail(c, CILHIP_ERR_HIP, "get_correspondences: unexpected exception"); }
}
static int get_correspondences_impl(cilhip_ctx* c, uint64_t* i1, uint64_t* i2, float* val, size_t cap, size_t* n_out) {
  { const int prc = materialize_pending(c); if (prc) return prc; }
  if (c->have_pairs) {
    // pair list of FIRST_TO_SECOND / BOTH: stored ascending (first, second); the reference leaves the set sorted by
    // value after the fraction filter (correspondence.hpp:61) and by (indexInSecond, value) after the FIRST_TO_SECOND
    // one-to-one filter (:74-82) -- reproduce that (ties keep the stored order)
    const size_t cnt = c->pairs.count;
    *n_out = cnt;
    if (cnt > cap) return fail(c, CILHIP_ERR_INVALID, "get_correspondences: capacity too small");
    if (cnt == 0) return CILHIP_OK;
    CK(c, hipSetDevice(c->device));
    std::vector<uint32_t> f(cnt), sc(cnt);
    std::vector<float> v(cnt);
    CK(c, hipMemcpyAsync(f.data(), c->pairs.first, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipMemcpyAsync(sc.data(), c->pairs.second, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipMemcpyAsync(v.data(), c->pairs.d2, cnt * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    std::vector<size_t> ord(cnt);
    for (size_t k = 0; k < cnt; ++k) ord[k] = k;
    const bool frac = c->inlier_fraction > 0.0 && c->inlier_fraction < 1.0;
    if (c->one_to_one && c->search_dir == 1)
      std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return sc[x] != sc[y] ? sc[x] < sc[y] : v[x] < v[y]; });
    else if (frac)
      std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return v[x] < v[y]; });
    for (size_t k = 0; k < cnt; ++k) {
      if (i1) i1[k] = f[ord[k]];
      if (i2) i2[k] = sc[ord[k]];
      if (val) val[k] = v[ord[k]];
    }
    return CILHIP_OK;
  }
  if (!c->have_nn) return fail(c, CILHIP_ERR_INVALID, "get_correspondences: no search has been run");
  std::vector<uint32_t> idx(c->ns ? c->ns : 1);
  std::vector<float> d2(c->ns ? c->ns : 1);
  int rc = cilhip_get_nn(c, idx.data(), d2.data(), CILHIP_MEM_HOST);
  if (rc) return rc;
  // order-preserving compaction in ascending source index (kd_tree_utilities.hpp:45-50)
  size_t cnt = 0;
  for (uint32_t i = 0; i < c->ns; ++i) {
    if (idx[i] == NONE_U32) continue;
    if (cnt < cap) {
      if (i1) i1[cnt] = idx[i];
      if (i2) i2[cnt] = i;
      if (val) val[cnt] = d2[i];
    }
    ++cnt;
  }
  *n_out = cnt;
  if (cnt > cap) return fail(c, CILHIP_ERR_INVALID, "get_correspondences: capacity too small");
  // the reference's filters leave the set sorted: by value after the fraction filter (correspondence.hpp:61),
  // by indexInFirst after the one-to-one filter (:86-94); reproduce that order (ties: ascending source index)
  if (filters_active(c) && cnt > 1 && i1 && i2 && val) {
    std::vector<size_t> ord(cnt);
    for (size_t k = 0; k < cnt; ++k) ord[k] = k;
    if (c->one_to_one) std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return i1[a] < i1[b]; });
    else std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return val[a] < val[b]; });
    std::vector<uint64_t> t1(cnt), t2(cnt); std::vector<float> tv(cnt);
    for (size_t k = 0; k < cnt; ++k) { t1[k] = i1[ord[k]]; t2[k] = i2[ord[k]]; tv[k] = val[ord[k]]; }
    memcpy(i1, t1.data(), cnt * sizeof(uint64_t)); memcpy(i2, t2.data(), cnt * sizeof(uint64_t)); memcpy(val, tv.data(), cnt * sizeof(float));
  }
  return CILHIP_OK;
}

void cilhip_icp_default_params(cilhip_icp_params* p) {
  if (!p) return;
  p->metric = CILHIP_METRIC_COMBINED;
  p->w_p2p = 0.0f; p->w_p2pl = 1.0f;
  p->max_iter = 15; p->conv_tol = 1e-5f;
  p->max_opt_iter = 1; p->opt_conv_tol = 1e-5f;
  p->max_sq_dist = 0.01f * 0.01f;
}

int cilhip_get_grid_info(cilhip_ctx* c, cilhip_grid_info* o) {
  if (!c || !o) return CILHIP_ERR_INVALID;
  if (!c->has_target) return fail(c, CILHIP_ERR_INVALID, "no target");
  o->nx = c->grid.nx; o->ny = c->grid.ny; o->nz = c->grid.nz;
  o->cell = c->grid.cell;
  o->origin[0] = c->grid.ox; o->origin[1] = c->grid.oy; o->origin[2] = c->grid.oz;
  o->n_cells = c->grid_cells;
  o->avg_occupancy = c->grid_occ;
  o->build_ms = c->build_ms;
  return CILHIP_OK;
}

int cilhip_get_last_timing(cilhip_ctx* c, double* loop_ms, double* search_ms, int* launches) {
  if (!c) return CILHIP_ERR_INVALID;
  if (loop_ms) *loop_ms = c->last_loop_ms;
  if (search_ms) *search_ms = c->last_search_ms;
  if (launches) *launches = c->last_search_launches;
  return CILHIP_OK;
}

// c_api.hip -- the C ABI of libcilantro_hip.so (declared in include/cilantro_hip/c_api.h), but for the ICP loop drivers (icp_loop.hip).
// Host-side orchestration only: owns device buffers + stream, enqueues the kernels of kernels.hip /
// grid_build.hip.  No CPU compute fallback exists: without a usable HIP device every call fails.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <new>

#include "ctx.hpp"
#include "stateless.hpp"

// (multi.hip -- the C entry of the multi-device loops -- drives contexts through the public entry points; these two are all it reads of one)
namespace cilhip {
hipStream_t ctx_stream(const cilhip_ctx* c) { return c->stream; }
double ctx_wait_us(const cilhip_ctx* c) { return c->wait_us; }
}  // namespace cilhip

// ---- what a context lets go of, and when (ctx.hpp: the groups).  A shared target array is only let go of: its last holder frees it.
static void drop_src_grid(cilhip_ctx* c) {
  static_cast<SrcGridBufs&>(*c) = SrcGridBufs{};
  c->src_grid = GridDev{}; c->has_src_grid = false;
}
static void drop_feat_tie_tables(cilhip_ctx* c) {      // (one target under one set of feature options; never shared)
  c->d_tief_leaf_slot.reset(); c->d_tief_nodes.reset();
}
static void drop_tie_tables(cilhip_ctx* c) {      // (they describe ONE target)
  c->d_tie_leaf_slot.reset(); c->d_tie_nodes.reset();
}
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
  c->has_source = false; c->src_sorted = false; drop_matches(c); c->ns = 0;
  c->have_pairs = false; c->pairs.count = 0;   // a pair list refers to the source / target it was found on
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

// ---- the options of a context, as a table a C caller can enumerate and check at compile time (enum cilhip_option in c_api.h):
// id, key, default, admissible range, one line of documentation, how to read the current value back.  cilhip_set_option() below
// validates and applies; the table is what tests/test_capi_symbols.py walks (every option documented, accepted with its default,
// readable, exercised by a test).  Long-form documentation: c_api.h above cilhip_set_option.
namespace {
struct OptionRow { cilhip_option_info_t info; double (*get)(const cilhip_ctx*); };
#define OPT(ID, KEY, DEF, LO, HI, DOC, EXPR) {{ID, KEY, DEF, LO, HI, DOC}, [](const cilhip_ctx* c) -> double { return (double)(EXPR); }}
const OptionRow g_options[] = {
  OPT(CILHIP_OPT_FUSED, "fused", 0, 0, 1, "1 = one per-lane search+accumulate kernel per iteration; 0 = search kernel + streaming accumulation (or the LDS tiles)", c->fused),
  OPT(CILHIP_OPT_INLIER_FRACTION, "inlier_fraction", 1, 0, 1, "CorrespondenceSearchKDTree::setInlierFraction: keep that fraction of the correspondences, nearest first", c->inlier_fraction),
  OPT(CILHIP_OPT_ONE_TO_ONE, "one_to_one", 0, 0, 1, "setOneToOne: a target point keeps only its nearest source point", c->one_to_one),
  OPT(CILHIP_OPT_TILED, "tiled", 1, 0, 2, "LDS-tiled search: 0 = never, 1 = when the cloud fills the chip with full tiles, 2 = always", c->tiled),
  OPT(CILHIP_OPT_WARM_START, "warm_start", 1, 0, 2, "warm-started iterations (margin proof): 0 = never, 1 = when the loop is near alignment, 2 = from the second iteration on", c->warm_start),
  OPT(CILHIP_OPT_WARM_FORECAST, "warm_forecast", 1, 0, 1, "the cold kernels' forecast gates the warm-started form (0: the step alone; tests)", c->warm_forecast),
  OPT(CILHIP_OPT_FUSED_EPILOGUE, "fused_epilogue", 0, 0, 1, "stage-1 reduction + epilogue as one launch behind a device-scope fence (bitwise equal, measured slower; A/B)", c->fused_epilogue),
  OPT(CILHIP_OPT_GROUP_SEARCH, "group_search", -1, -1, 64, "lanes per query of the cooperative global-memory search: -1 = the loop decides, 0 = never, 4 / 8 / 16 / 32 / 64", c->group_lanes),
  OPT(CILHIP_OPT_TIE_RULE, "tie_rule", 2, 0, 2, "exactly equidistant nearest points: 0 = lowest index, 1 = the reference's kd-tree order (tables up front), 2 = the same, tables when a tie is first met", c->tie_rule),
  OPT(CILHIP_OPT_WARM_EXTRA_FRACTION, "warm_extra_fraction", 0.0625, 1e-9, 1, "room (fraction of a cell) of the ball a warm-started iteration searches a listed query in", c->warm_extra),
  OPT(CILHIP_OPT_PAIR_RECORDS, "pair_records", 1, 0, 1, "streaming accumulation gathers a match's point and normal from one 32-byte record (A/B)", c->pair_records),
  OPT(CILHIP_OPT_TILE_RECORDS, "tile_records", 1, 0, 1, "the accumulating tile kernel writes the warm-started form's match records itself (A/B)", c->tile_records),
  OPT(CILHIP_OPT_WARM_ENTER_FRACTION, "warm_enter_fraction", 0.15, 1e-9, 1e9, "the warm-started form is entered once an update moves no source point by more than this fraction of a cell", c->warm_enter),
  OPT(CILHIP_OPT_POINT_WEIGHT_EVALUATOR, "point_weight_evaluator", 0, 0, 2, "combined metric, point-to-point terms: 0 = UnityWeightEvaluator, 1 = DistanceEvaluator, 2 = RBFKernelWeightEvaluator", c->cw_point_kind),
  OPT(CILHIP_OPT_PLANE_WEIGHT_EVALUATOR, "plane_weight_evaluator", 0, 0, 2, "combined metric, point-to-plane terms: 0 = Unity, 1 = Identity (distance), 2 = RBF kernel", c->cw_plane_kind),
  OPT(CILHIP_OPT_POINT_WEIGHT_SIGMA, "point_weight_sigma", 1, 1e-30, 1e30, "sigma of the RBF evaluator of the point-to-point terms", c->cw_point_sigma),
  OPT(CILHIP_OPT_PLANE_WEIGHT_SIGMA, "plane_weight_sigma", 1, 1e-30, 1e30, "sigma of the RBF evaluator of the point-to-plane terms", c->cw_plane_sigma),
  OPT(CILHIP_OPT_TILE_ACCUMULATION, "tile_accumulation", 1, 0, 2, "first Gauss-Newton step accumulated inside the LDS tiles: 0 = never, 1 = unless the source is far from alignment, 2 = always", (c->tile_acc ? (c->tile_acc_adaptive ? 1 : 2) : 0)),
  OPT(CILHIP_OPT_SEARCH_DIRECTION, "search_direction", 0, 0, 2, "CorrespondenceSearchDirection: 0 = SECOND_TO_FIRST, 1 = FIRST_TO_SECOND, 2 = BOTH", c->search_dir),
  OPT(CILHIP_OPT_FEATURE_NORMAL_WEIGHT, "feature_normal_weight", 0, 0, 1e30, "PointNormalFeaturesAdaptor's normal weight (> 0: the search runs on 6-D features)", c->normal_weight),
  OPT(CILHIP_OPT_FEATURE_KIND, "feature_kind", 0, 0, 2, "second feature block: 0 = normals (follow the transform), 1 = colours (do not), 2 = normals + colours (9-D)", c->feature_kind),
  OPT(CILHIP_OPT_FEATURE_COLOR_WEIGHT, "feature_color_weight", 0, 0, 1e30, "PointNormalColorFeaturesAdaptor's colour weight (feature_kind 2)", c->color_weight),
  OPT(CILHIP_OPT_SYMMETRIC_METRIC, "symmetric_metric", 1, 0, 1, "source normals, when set, switch the combined metric to the symmetric objective", c->symmetric),
  OPT(CILHIP_OPT_TRANSFORM_MODE, "transform_mode", 0, 0, 1, "ICP instance family: 0 = rigid, 1 = affine", c->transform_mode),
  OPT(CILHIP_OPT_REQUIRE_RECIPROCALITY, "require_reciprocality", 0, 0, 1, "setRequireReciprocality (search_direction BOTH)", c->reciprocal),
  OPT(CILHIP_OPT_CELL_OCCUPANCY, "cell_occupancy", 1, 1e-3, 1e6, "target points per grid cell the next cilhip_set_target aims at", c->cell_occupancy),
  OPT(CILHIP_OPT_REFINED_OCCUPANCY_FACTOR, "refined_occupancy_factor", 3, 1, 64, "how much denser than that a grid that had to be refined (surface, clusters) may stay", c->refined_occupancy),
  OPT(CILHIP_OPT_KERNEL_TIMING, "kernel_timing", 0, 0, 1, "hipEvents around the search / accumulation kernels (cilhip_enable_kernel_timing)", c->kernel_timing),
  OPT(CILHIP_OPT_KERNEL_TIMING_STRIDE, "kernel_timing_stride", 1, 1, 4096, "with kernel timing on: iterations 0..2 and every stride-th one carry events", c->timing_stride),
  OPT(CILHIP_OPT_REVERSE_WARM_START, "reverse_warm_start", 1, 0, 1, "device-resident FIRST_TO_SECOND / BOTH loops: reverse searches after the first start from the previous reverse matches (margin test over the source; A/B)", c->reverse_warm),
  OPT(CILHIP_OPT_FEATURE_WARM_START, "feature_warm_start", 1, 0, 1, "feature adaptors (SECOND_TO_FIRST loops): searches warm-started from the previous matches once the loop moves little (margin test with the feature distance; A/B)", c->feat_warm),
  OPT(CILHIP_OPT_AFFINE_DEVICE_LOOP, "affine_device_loop", 1, 0, 1, "affine classes: 1 = device-resident loop (one-pass moments, solve in the epilogue kernel), 0 = host-driven loop (three passes + host solve; A/B)", c->affine_device_loop),
};
#undef OPT
constexpr int N_OPTIONS = (int)(sizeof(g_options) / sizeof(g_options[0]));
static_assert(N_OPTIONS == CILHIP_OPT_COUNT, "one table row per enum cilhip_option value, in the enum's order");
}  // namespace

int cilhip_option_count(void) { return N_OPTIONS; }
const cilhip_option_info_t* cilhip_option_info(int id) { return (id >= 0 && id < N_OPTIONS) ? &g_options[id].info : nullptr; }
int cilhip_set_option_id(cilhip_ctx* c, cilhip_option id, double value) {
  if (!c) return CILHIP_ERR_INVALID;
  if ((int)id < 0 || (int)id >= N_OPTIONS) return fail(c, CILHIP_ERR_INVALID, "set_option_id: unknown option");
  return cilhip_set_option(c, g_options[(int)id].info.key, value);
}
int cilhip_get_option(cilhip_ctx* c, const char* key, double* value) {
  if (!c || !key || !value) return CILHIP_ERR_INVALID;
  for (int i = 0; i < N_OPTIONS; ++i)
    if (!strcmp(key, g_options[i].info.key)) { *value = g_options[i].get(c); return CILHIP_OK; }
  return fail(c, CILHIP_ERR_INVALID, "get_option: unknown key");
}

int cilhip_set_option(cilhip_ctx* c, const char* key, double value) {
  if (!c || !key) return CILHIP_ERR_INVALID;
  if (value != value) return fail(c, CILHIP_ERR_INVALID, "set_option: the value is not a number");
  // every row's admissible range holds for every key (a mistyped "tiled" = 3 would otherwise run some other form); the rows
  // below only add what a range cannot say (the discrete values of group_search, tie_rule, ...)
  for (int i = 0; i < N_OPTIONS; ++i)
    if (!strcmp(key, g_options[i].info.key) && !(value >= g_options[i].info.min_value && value <= g_options[i].info.max_value))
      return fail(c, CILHIP_ERR_INVALID, "set_option: value outside the option's [min_value, max_value] (cilhip_option_info)");
  if (!strcmp(key, "fused")) { c->fused = value != 0.0; return CILHIP_OK; }
  // (a finished run's set that has not been searched again yet -- cilhip_get_last_matches_origin 2 -- would be filtered with the
  //  NEW values: a changed post-filter drops it; a set already in memory is what its search left, whatever is set afterwards)
  if (!strcmp(key, "inlier_fraction")) { if (c->inlier_fraction != value && c->pending_matches) drop_matches(c); c->inlier_fraction = value; return CILHIP_OK; }
  if (!strcmp(key, "one_to_one")) { if (c->one_to_one != (value != 0.0) && c->pending_matches) drop_matches(c); c->one_to_one = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "tiled")) { c->tiled = (int)value; return CILHIP_OK; }
  if (!strcmp(key, "warm_start")) { c->warm_start = (int)value; return CILHIP_OK; }
  if (!strcmp(key, "warm_forecast")) { c->warm_forecast = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "fused_epilogue")) { c->fused_epilogue = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "reverse_warm_start")) { c->reverse_warm = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "feature_warm_start")) { c->feat_warm = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "affine_device_loop")) { c->affine_device_loop = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "group_search")) {
    if (value != -1.0 && value != 0.0 && value != 4.0 && value != 8.0 && value != 16.0 && value != 32.0 && value != 64.0)
      return fail(c, CILHIP_ERR_INVALID, "group_search: -1 (the loop decides), 0 (never), or 4, 8, 16, 32, 64 lanes per query");
    c->group_lanes = (int)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "tie_rule")) {
    if (value != 0.0 && value != 1.0 && value != 2.0)
      return fail(c, CILHIP_ERR_INVALID, "tie_rule: 0 (lowest index), 1 (the reference's kd-tree order, tables built up front) or 2 (the same, tables built when a tie is first met)");
    if (((int)value != 0) != (c->tie_rule != 0)) drop_matches(c);
    c->tie_rule = (int)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "warm_extra_fraction")) {
    if (!(value > 0.0 && value <= 1.0)) return fail(c, CILHIP_ERR_INVALID, "warm_extra_fraction: in (0, 1]");
    c->warm_extra = (float)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "pair_records")) { c->pair_records = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "tile_records")) { c->tile_records = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "warm_enter_fraction")) {
    if (!(value > 0.0)) return fail(c, CILHIP_ERR_INVALID, "warm_enter_fraction: > 0 (fraction of a grid cell)");
    c->warm_enter = (float)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "point_weight_evaluator") || !strcmp(key, "plane_weight_evaluator")) {
    if (value != 0.0 && value != 1.0 && value != 2.0) return fail(c, CILHIP_ERR_INVALID, "weight evaluator: 0 = Unity, 1 = Identity, 2 = RBF kernel");
    (key[1] == 'o' ? c->cw_point_kind : c->cw_plane_kind) = (int)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "point_weight_sigma") || !strcmp(key, "plane_weight_sigma")) {
    if (!(value > 0.0)) return fail(c, CILHIP_ERR_INVALID, "weight evaluator sigma must be positive");
    (key[1] == 'o' ? c->cw_point_sigma : c->cw_plane_sigma) = (float)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "tile_accumulation")) { c->tile_acc = value != 0.0; c->tile_acc_adaptive = value != 2.0; return CILHIP_OK; }
  if (!strcmp(key, "search_direction")) {
    if (value != 0.0 && value != 1.0 && value != 2.0) return fail(c, CILHIP_ERR_INVALID, "search_direction: 0 = SECOND_TO_FIRST, 1 = FIRST_TO_SECOND, 2 = BOTH");
    c->search_dir = (int)value; drop_matches(c); c->have_pairs = false;
    return CILHIP_OK;
  }
  if (!strcmp(key, "feature_normal_weight")) {
    if (!(value >= 0.0)) return fail(c, CILHIP_ERR_INVALID, "feature_normal_weight: >= 0 (0 = plain point features)");
    if (c->normal_weight != (float)value) drop_feat_tie_tables(c);
    c->normal_weight = (float)value; drop_matches(c); c->have_pairs = false;
    return CILHIP_OK;
  }
  if (!strcmp(key, "feature_kind")) {
    if (value != 0.0 && value != 1.0 && value != 2.0)
      return fail(c, CILHIP_ERR_INVALID, "feature_kind: 0 = normals (follow the transform), 1 = colours (do not), 2 = normals + colours (9-D)");
    if ((int)value != c->feature_kind) { drop_src_grid(c); drop_feat_tie_tables(c); }      // (the source's grid carries the feature vectors of the reverse searches)
    c->feature_kind = (int)value; drop_matches(c); c->have_pairs = false;
    return CILHIP_OK;
  }
  if (!strcmp(key, "feature_color_weight")) {
    if (!(value >= 0.0)) return fail(c, CILHIP_ERR_INVALID, "feature_color_weight: >= 0");
    if (c->color_weight != (float)value) drop_feat_tie_tables(c);
    c->color_weight = (float)value; drop_matches(c); c->have_pairs = false;
    return CILHIP_OK;
  }
  if (!strcmp(key, "symmetric_metric")) { c->symmetric = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "transform_mode")) {
    if (value != 0.0 && value != 1.0) return fail(c, CILHIP_ERR_INVALID, "transform_mode: 0 = rigid, 1 = affine");
    c->transform_mode = (int)value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "require_reciprocality")) { c->reciprocal = value != 0.0; drop_matches(c); c->have_pairs = false; return CILHIP_OK; }
  if (!strcmp(key, "cell_occupancy")) { c->cell_occupancy = value; return CILHIP_OK; }
  if (!strcmp(key, "refined_occupancy_factor")) {
    if (!(value >= 1.0 && value <= 64.0)) return fail(c, CILHIP_ERR_INVALID, "refined_occupancy_factor: in [1, 64]");
    c->refined_occupancy = value;
    return CILHIP_OK;
  }
  if (!strcmp(key, "kernel_timing")) { c->kernel_timing = value != 0.0; return CILHIP_OK; }
  if (!strcmp(key, "kernel_timing_stride")) {
    if (!(value >= 1.0 && value <= 4096.0)) return fail(c, CILHIP_ERR_INVALID, "kernel_timing_stride: 1 .. 4096");
    c->timing_stride = (int)value;
    return CILHIP_OK;
  }
  return fail(c, CILHIP_ERR_INVALID, "set_option: unknown key");
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
  drop_matches(c);
  c->have_pairs = false; c->pairs.count = 0;
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
  c->d_tie_leaf_slot = from->d_tie_leaf_slot; c->d_tie_nodes = from->d_tie_nodes;
  c->policy.warm_banned = false;
  c->src_sorted = false;  // source order is tied to the target grid
  drop_matches(c);
  c->have_pairs = false; c->pairs.count = 0;
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
  c->have_pairs = false; c->pairs.count = 0;
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
  drop_matches(c);
  c->have_pairs = false; c->pairs.count = 0;
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
  drop_matches(c);
  c->have_pairs = false; c->pairs.count = 0;
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
    drop_matches(c);
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
// The per-pair weights of the combined-metric classes (PointToPoint/PointToPlaneCorrWeightEvaluatorT of
// icp_single_transform_combined_metric.hpp:11-14; the point-to-point class has none): evaluator(corr.value) times the
// metric weight, in f32.  RBF coefficient as common_pair_evaluators.hpp:53.
static CorrWeights corr_weights_of(const cilhip_ctx* c, bool combined_metric, float w_p2p, float w_p2pl) {
  CorrWeights w{};
  w.enabled = (combined_metric && weighted(c)) ? 1 : 0;
  w.point_kind = c->cw_point_kind; w.plane_kind = c->cw_plane_kind;
  w.point_coeff = -0.5f / (c->cw_point_sigma * c->cw_point_sigma);
  w.plane_coeff = -0.5f / (c->cw_plane_sigma * c->cw_plane_sigma);
  w.w_p2p = w_p2p; w.w_p2pl = w_p2pl;
  // (a caller's own evaluators: prepare_pair_weights() has put the weights of the stored correspondences into the tables)
  if (w.enabled && c->weight_fn) { w.point_table = c->d_wtab; w.plane_table = c->d_wtab + c->d_wtab.capacity() / 2; }
  return w;
}
CorrWeights cilhip::corr_weights_of(const cilhip_ctx* c, const cilhip_icp_params* p) {
  return corr_weights_of(c, p->metric == CILHIP_METRIC_COMBINED, p->w_p2p, p->w_p2pl);
}
// k_self_nn's nearest-other-point table (4 B per target point, 0.5 ms at 10M): built by the first warm-capable run on a target
int cilhip::ensure_safe2(cilhip_ctx* c) {
  if (c->d_safe2) return CILHIP_OK;
  CK(c, c->d_safe2.alloc(c->grid.n));
  launch_self_nn(c->grid, c->d_safe2, c->stream);
  return CILHIP_OK;
}

// ---- option "tie_rule": the reference's order among exactly equidistant nearest points ------------------------------------------
// When the option is in force for a context's searches: the order is the reference's kd-tree over the TARGET POINTS: it covers the
// SECOND_TO_FIRST matches (also the forward half of BOTH) under rigid and affine transforms.  Feature adaptors search another
// space (nanoflann's DIM = 6 / 9 tree: tie_feat_on below), the reverse matches of FIRST_TO_SECOND / BOTH a tree over the transformed
// SOURCE that the reference rebuilds every iteration (rev_tie_aware); the feature adaptors' reverse searches keep the lowest index
// (tie_rule 2) or are refused (tie_rule 1, the explicit request).  An
// index shard of a target (cilhip_set_shard_info) notices and counts ties like any context, but never builds tables from its own points:
// the order belongs to the WHOLE target's tree -- whoever owns the shards loads it (cilhip_load_tie_order with the global indices) and
// runs the two-key protocol between them (cilhip_icp_order_keys).  (The predicate itself: tie_mode_on, ctx.hpp.)
// ... and over 6-D / 9-D features: the forward (SECOND_TO_FIRST) search of a whole target follows the reference's DIM = 6 / 9 tree
// (its order tables: tie_order_build_device_features; tie_settle<true> / tie_before_nd on the device)
static bool tie_feat_on(const cilhip_ctx* c) { return c->tie_rule != 0 && feat6(c) && c->search_dir == 0 && !c->partial_target && !c->index_offset; }
static TieDev tie_dev_of(const cilhip_ctx* c) {
  TieDev t{};
  if (feat6(c)) {
    t.mode = tie_feat_on(c) ? 1 : 0;
    t.leaf_slot = t.mode ? c->d_tief_leaf_slot : nullptr;
    t.nodes = c->d_tief_nodes;
    t.counters = c->d_tie_counters;
    return t;
  }
  t.mode = tie_mode_on(c) ? 1 : 0;
  t.leaf_slot = t.mode ? c->d_tie_leaf_slot : nullptr;
  t.nodes = c->d_tie_nodes;
  t.counters = c->d_tie_counters;
  return t;
}
// Order tables by this target's ORIGINAL (local) index -> device, by sorted position.
static int load_tie_tables(cilhip_ctx* c, const uint32_t* leaf_by_index, const uint32_t* slot_by_index, const cilhip::TieNode* nodes, size_t n_nodes) {
  static_assert(sizeof(cilhip::TieNode) == sizeof(uint4), "TieNode is read as one 16-byte record");
  CK(c, hipSetDevice(c->device));
  drop_tie_tables(c);
  const size_t n = c->grid.n;
  DevBuf<uint32_t> d_leaf, d_slot;
  // (d_tie_leaf_slot != null is the "tables loaded" flag: nothing may be left half set when an allocation fails)
  hipError_t e = c->d_tie_leaf_slot.alloc(n);
  if (e == hipSuccess) e = c->d_tie_nodes.alloc(n_nodes);
  if (e == hipSuccess) e = d_leaf.alloc(n);
  if (e == hipSuccess) e = d_slot.alloc(n);
  if (e == hipSuccess && n) {
    e = hipMemcpyAsync(d_leaf, leaf_by_index, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_slot, slot_by_index, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && n_nodes) e = hipMemcpyAsync(c->d_tie_nodes, nodes, n_nodes * sizeof(uint4), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { launch_tie_tables_by_position(c->grid.pts, c->grid.n, d_leaf, d_slot, c->d_tie_leaf_slot, c->stream); e = hipGetLastError(); }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);      // (the host arrays and the two staging buffers live on this frame)
  if (e != hipSuccess) { drop_tie_tables(c); c->err = std::string("tie_rule: loading the order tables: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  c->tie_max_depth = 0;
  for (size_t k = 0; k < n_nodes; ++k) c->tie_max_depth = std::max(c->tie_max_depth, (int)(nodes[k].info >> 3));
  return CILHIP_OK;
}
// The order tables of a tree over this context's target, built on the device (tie_build.hip): `build` fills leaf and slot by original
// index and the nodes; the tables by sorted position go to *leaf_slot.  On failure the caller drops what *leaf_slot holds.
template <class Build>
static hipError_t build_target_order_tables(cilhip_ctx* c, SharedBuf<uint2>& leaf_slot, SharedBuf<uint4>& nodes, Build build) {
  const uint32_t n = c->grid.n;
  DevBuf<uint32_t> d_leaf, d_slot;
  DevBuf<uint4> d_nodes;
  hipError_t e = d_leaf.alloc(n);
  if (e == hipSuccess) e = d_slot.alloc(n);
  if (e == hipSuccess) e = leaf_slot.alloc(n);
  if (e == hipSuccess) e = build(d_leaf.get(), d_slot.get(), &d_nodes);
  if (e == hipSuccess && !d_nodes) e = d_nodes.alloc(1);      // (an empty target)
  if (e == hipSuccess && n) { launch_tie_tables_by_position(c->grid.pts, n, d_leaf, d_slot, leaf_slot, c->stream); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = nodes.adopt(std::move(d_nodes));
  return e;
}
// The tables of THIS context's target, from the grid's own records.
static int build_tie_tables(cilhip_ctx* c) {
  if (c->d_tie_leaf_slot || !c->has_target) return CILHIP_OK;
  const auto t0 = std::chrono::steady_clock::now();
  CK(c, hipSetDevice(c->device));
  drop_tie_tables(c);
  size_t n_nodes = 0;
  int depth = 0;
  const hipError_t e = build_target_order_tables(c, c->d_tie_leaf_slot, c->d_tie_nodes, [&](uint32_t* leaf, uint32_t* slot, DevBuf<uint4>* nodes) {
    return tie_order_build_device(nullptr, c->grid.pts, c->grid.n, c->stream, leaf, slot, nodes, &n_nodes, &depth); });
  if (e != hipSuccess) {
    drop_tie_tables(c);
    c->err = std::string("tie_rule: building the order tables: ") + hipGetErrorString(e);
    return CILHIP_ERR_HIP;
  }
  c->tie_max_depth = depth;
  c->tie_build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  ++c->tie_builds;
  return CILHIP_OK;
}
// the counters of the searches since the last launch_init_state (a host round trip)
static int read_tie_counters(cilhip_ctx* c, unsigned int out[4]) {
  CK(c, hipMemcpyAsync(out, c->d_tie_counters, 4 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}
// The reverse matches' order (FIRST_TO_SECOND / BOTH): what k_reverse_search is handed.  Without valid tables it counts the tied target
// points (counters[3]) and keeps the lowest source index.
TieDev cilhip::tie_dev_rev(const cilhip_ctx* c) {
  TieDev t{};
  t.mode = tie_mode_on(c) ? 1 : 0;
  t.leaf_slot = (t.mode && c->rev_tie_valid) ? c->d_rev_tie_leaf_slot : nullptr;
  t.nodes = c->d_rev_tie_nodes;
  t.counters = c->d_tie_counters;
  return t;
}
// The order tables of the tree the reference builds over the source transformed by T (src_points_trans = transform_ * src, the engine's
// pinned f32 expression; correspondence_search_kd_tree.hpp:185-222), by position in the source grid.  Device work per search: the
// transform of the source (its original order) and tie_order_build_device over it (2 ms for a 110k-point frame, 25 ms at 10M).
static int build_rev_tie_tables(cilhip_ctx* c, const float T[16]) {
  if (c->rev_tie_valid && memcmp(c->rev_tie_T, T, sizeof(c->rev_tie_T)) == 0) return CILHIP_OK;
  c->rev_tie_valid = false;
  const uint32_t n = c->ns;
  if (!c->has_src_grid || n == 0) return CILHIP_OK;
  CK(c, hipSetDevice(c->device));
  DevBuf<float> d_q;
  DevBuf<uint32_t> d_leaf, d_slot;
  DevBuf<uint4> d_nodes;
  size_t n_nodes = 0;
  hipError_t e = d_q.alloc((size_t)n * 3);
  if (e == hipSuccess) e = d_leaf.alloc(n);
  if (e == hipSuccess) e = d_slot.alloc(n);
  if (e == hipSuccess && !c->d_rev_tie_leaf_slot) e = c->d_rev_tie_leaf_slot.alloc(n);
  if (e == hipSuccess) { launch_transform_original_host_T(c->d_src_xyz, n, T, d_q, c->stream); e = hipGetLastError(); }      // q = fl(T s), the engine's pinned expression
  if (e == hipSuccess) e = tie_order_build_device(d_q, nullptr, n, c->stream, d_leaf, d_slot, &d_nodes, &n_nodes, nullptr);
  if (e == hipSuccess) {
    c->d_rev_tie_nodes = std::move(d_nodes);
    launch_tie_tables_by_position(c->src_grid.pts, n, d_leaf, d_slot, c->d_rev_tie_leaf_slot, c->stream);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) { c->err = std::string("tie_rule: the transformed source's order tables: ") + hipGetErrorString(e); return CILHIP_ERR_HIP; }
  memcpy(c->rev_tie_T, T, sizeof(c->rev_tie_T));
  c->rev_tie_valid = true;
  ++c->rev_tie_builds;
  return CILHIP_OK;
}
// tie_rule 1: the tables before the first search; refusals of the explicit request (see tie_mode_on)
// The order tables of the tree the reference's feature adaptor searches (DIM = 6: points + weighted normals or colours; 9: + colours), for
// this target under the CURRENT feature options, built on the device (tie_build.hip).
static int build_feat_tie_tables(cilhip_ctx* c) {
  if (c->d_tief_leaf_slot || !c->has_target) return CILHIP_OK;
  CK(c, hipSetDevice(c->device));
  { const int rc = ensure_feature_arrays(c); if (rc) return rc; }
  const FeatSpec f = feat_spec_of(c);
  const int dim = c->feature_kind == 2 ? 9 : 6;
  if (!f.dst || (dim == 9 && !f.dst2)) return fail(c, CILHIP_ERR_INVALID, "tie_rule: the target's feature attributes (normals / colours) are not set");
  size_t n_nodes = 0;
  const hipError_t e = build_target_order_tables(c, c->d_tief_leaf_slot, c->d_tief_nodes, [&](uint32_t* leaf, uint32_t* slot, DevBuf<uint4>* nodes) {
    return tie_order_build_device_features(dim, c->grid.pts, f.dst, f.w, f.dst2, f.w2, c->grid.n, c->stream, leaf, slot, nodes, &n_nodes, nullptr); });
  if (e != hipSuccess) {
    drop_feat_tie_tables(c);
    c->err = std::string("tie_rule: building the feature tree's order tables: ") + hipGetErrorString(e);
    return CILHIP_ERR_HIP;
  }
  ++c->tief_builds;
  return CILHIP_OK;
}
int cilhip::tie_prepare(cilhip_ctx* c, const char* what) {
  c->tie_counters_fresh = false;      // (a new search / run: whatever the host holds of the counters is history)
  if (c->tie_rule == 1 && ((feat6(c) && !tie_feat_on(c)) || (!feat6(c) && c->partial_target && !c->d_tie_leaf_slot))) {
    c->err = std::string(what) + ": tie_rule = 1 covers the SECOND_TO_FIRST search (point features: every direction) on a whole target, or on shards of a point-feature target with the whole target's order loaded (tie_rule = 2 applies the reference's order where it is defined)";
    return CILHIP_ERR_UNSUPPORTED;
  }
  if (c->tie_rule == 1 && tie_feat_on(c) && c->ns && c->grid.n) return build_feat_tie_tables(c);
  if (c->tie_rule == 1 && c->search_dir != 0) c->rev_tie_aware = true;
  if (c->tie_rule == 0) c->rev_tie_aware = false;
  if (c->tie_rule == 1 && tie_mode_on(c) && !c->partial_target && c->search_dir != 1 && c->ns && c->grid.n) return build_tie_tables(c);
  return CILHIP_OK;
}
// After a search / run: did it meet ties without tables (tie_rule 2)?  Then the tables are built and *again says: run it once more.
int cilhip::tie_check_pending(cilhip_ctx* c, bool* again) {
  *again = false;
  if (tie_feat_on(c)) {      // a feature search: its forward matches counted tied queries while the feature tree's tables were not there
    if (c->d_tief_leaf_slot || !c->ns || !c->grid.n) return CILHIP_OK;
    unsigned int cnt[4];
    if (c->tie_counters_fresh) memcpy(cnt, c->tie_counters_host, sizeof(cnt));
    else { const int rc = read_tie_counters(c, cnt); if (rc) return rc; }
    c->tie_counters_fresh = false;
    if (cnt[0] == 0u) return CILHIP_OK;
    *again = true;
    CK(c, hipMemsetAsync(c->d_tie_counters, 0, 4 * sizeof(unsigned int), c->stream));
    return build_feat_tie_tables(c);
  }
  if (!tie_mode_on(c) || c->partial_target || !c->ns || !c->grid.n) return CILHIP_OK;      // (a part of a target: its caller loads the whole cloud's order)
  const bool fwd_open = !c->d_tie_leaf_slot && c->search_dir != 1;      // (forward matches: SECOND_TO_FIRST, the forward half of BOTH)
  const bool rev_open = !c->rev_tie_aware && c->search_dir != 0;
  if (!fwd_open && !rev_open) return CILHIP_OK;
  unsigned int cnt[4];
  if (c->tie_counters_fresh) {      // (a run's read_state has just brought them over with the loop state: no second round trip)
    memcpy(cnt, c->tie_counters_host, sizeof(cnt));
  } else {
    const int rc = read_tie_counters(c, cnt);
    if (rc) return rc;
  }
  c->tie_counters_fresh = false;
  // Forward matches: any tie, the tables are built once per target.  Reverse matches: the tables cost a host tree build PER SEARCH (0.25 s
  // at 10M points against an iteration of a millisecond), so the automatic rule pays it for clouds that tie systematically -- duplicated
  // points, lattices: at least 16 tied target points and one in 100 000 -- and not for the isolated coincidence of two f32 distances in a
  // large random cloud (about one target point in ten million): those keep the lowest source index and stay counted
  // (cilhip_get_tie_rule_stats); tie_rule 1 follows the reference for every one of them.
  const bool fwd = fwd_open && cnt[0] != 0u, rev = rev_open && cnt[3] >= 16u && (unsigned long long)cnt[3] * 100000ull >= (unsigned long long)c->grid.n;
  if (!fwd && !rev) return CILHIP_OK;
  *again = true;
  CK(c, hipMemsetAsync(c->d_tie_counters, 0, 4 * sizeof(unsigned int), c->stream));      // (the repeated search counts afresh)
  if (rev) c->rev_tie_aware = true;      // (the tables themselves: per search, under its transform -- run_pair_search)
  return fwd ? build_tie_tables(c) : CILHIP_OK;
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
  drop_matches(c);
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
static int materialize_pending(cilhip_ctx* c) {
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

int cilhip_get_tie_count(cilhip_ctx* c, const float T[16], float max_sq, size_t* n_ties) {
  if (!c || !T || !n_ties) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  const int rc = ensure_sorted(c, T);
  if (rc) return rc;
  launch_count_ties(c->grid, c->d_src_sorted, c->ns, T, max_sq, c->d_count, c->stream);
  unsigned long long v = 0;
  CK(c, hipMemcpyAsync(&v, c->d_count, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  CK(c, hipGetLastError());
  *n_ties = (size_t)v;
  return CILHIP_OK;
}

struct cilhip_tie_order { std::vector<uint32_t> leaf, slot; std::vector<cilhip::TieNode> nodes; uint32_t n = 0; int max_depth = 0; };
int cilhip_tie_order_create(const float* xyz, size_t n, cilhip_tie_order** out) {
  if (!out || (n && !xyz) || n >= 0xFFFFFFF0ull) return CILHIP_ERR_INVALID;
  *out = nullptr;
  int ndev = 0, dev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hipGetDevice(&dev) != hipSuccess) return CILHIP_ERR_NO_DEVICE;      // (built on the device: no CPU fallback)
  cilhip_tie_order* o = nullptr;
  DevBuf<float> d_xyz;
  DevBuf<uint32_t> d_leaf, d_slot;
  DevBuf<uint4> d_nodes;
  size_t n_nodes = 0;
  StreamGuard s;      // (declared last: drained and destroyed before the buffers go)
  hipError_t e = hipSuccess;
  int rc = CILHIP_OK;
  try {
    o = new cilhip_tie_order();
    o->n = (uint32_t)n;
    o->leaf.assign(n, 0u); o->slot.assign(n, 0u);
    if (n) {
      e = s.create();
      if (e == hipSuccess) e = d_xyz.alloc(n * 3);
      if (e == hipSuccess) e = d_leaf.alloc(n);
      if (e == hipSuccess) e = d_slot.alloc(n);
      if (e == hipSuccess) e = hipMemcpyAsync(d_xyz, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, s);
      if (e == hipSuccess) e = tie_order_build_device(d_xyz, nullptr, (uint32_t)n, s, d_leaf, d_slot, &d_nodes, &n_nodes, &o->max_depth);
      if (e == hipSuccess) { o->nodes.resize(n_nodes); e = hipMemcpyAsync(o->nodes.data(), d_nodes, n_nodes * sizeof(uint4), hipMemcpyDeviceToHost, s); }
      if (e == hipSuccess) e = hipMemcpyAsync(o->leaf.data(), d_leaf, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipMemcpyAsync(o->slot.data(), d_slot, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
      if (e == hipSuccess) e = hipStreamSynchronize(s);
    }
  } catch (...) { rc = CILHIP_ERR_HIP; }      // (out of host memory: never across the C boundary)
  if (e != hipSuccess) rc = CILHIP_ERR_HIP;
  if (rc != CILHIP_OK) { delete o; return rc; }
  *out = o;
  return CILHIP_OK;
}
void cilhip_tie_order_destroy(cilhip_tie_order* order) { delete order; }
int cilhip_tie_order_tables(const cilhip_tie_order* o, uint32_t* leaf_by_index, uint32_t* slot_by_index, void* nodes_out, size_t nodes_cap, size_t* n_nodes, int* max_depth) {
  if (!o) return CILHIP_ERR_INVALID;
  if (leaf_by_index && o->n) memcpy(leaf_by_index, o->leaf.data(), (size_t)o->n * sizeof(uint32_t));
  if (slot_by_index && o->n) memcpy(slot_by_index, o->slot.data(), (size_t)o->n * sizeof(uint32_t));
  if (nodes_out && nodes_cap) memcpy(nodes_out, o->nodes.data(), std::min(nodes_cap, o->nodes.size()) * sizeof(cilhip::TieNode));
  if (n_nodes) *n_nodes = o->nodes.size();
  if (max_depth) *max_depth = o->max_depth;
  return CILHIP_OK;
}
int cilhip_load_tie_order(cilhip_ctx* c, const cilhip_tie_order* order, const uint32_t* global_index) {
  if (!c || !order) return CILHIP_ERR_INVALID;
  if (!c->has_target) return fail(c, CILHIP_ERR_INVALID, "load_tie_order: set_target first");
  const uint32_t n = c->grid.n, N = order->n;
  if (n == 0) return load_tie_tables(c, nullptr, nullptr, order->nodes.data(), order->nodes.size());      // (a shard without target points)
  if (!global_index) {
    if (n != N) return fail(c, CILHIP_ERR_INVALID, "load_tie_order: the order was built for a cloud of another size (pass global_index for a part of it)");
    return load_tie_tables(c, order->leaf.data(), order->slot.data(), order->nodes.data(), order->nodes.size());
  }
  try {
    std::vector<uint32_t> leaf(n ? n : 1), slot(n ? n : 1);
    for (uint32_t i = 0; i < n; ++i) {
      if (global_index[i] >= N) return fail(c, CILHIP_ERR_INVALID, "load_tie_order: global index out of range");
      leaf[i] = order->leaf[global_index[i]]; slot[i] = order->slot[global_index[i]];
    }
    return load_tie_tables(c, leaf.data(), slot.data(), order->nodes.data(), order->nodes.size());
  } catch (...) { return fail(c, CILHIP_ERR_HIP, "load_tie_order: out of host memory"); }
}
int cilhip_build_tie_order(cilhip_ctx* c) {
  if (!c) return CILHIP_ERR_INVALID;
  if (!c->has_target) return fail(c, CILHIP_ERR_INVALID, "build_tie_order: set_target first");
  if (c->partial_target) return fail(c, CILHIP_ERR_INVALID, "build_tie_order: this context holds a PART of a target (cilhip_set_shard_info): the order is the whole cloud's -- cilhip_tie_order_create + cilhip_load_tie_order");
  return build_tie_tables(c);
}
int cilhip_get_tie_order_info(cilhip_ctx* c, cilhip_tie_order_info* out) {
  if (!c || !out) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  unsigned int cnt[4];
  { const int rc = read_tie_counters(c, cnt); if (rc) return rc; }
  out->loaded = (feat6(c) ? c->d_tief_leaf_slot != nullptr : c->d_tie_leaf_slot != nullptr) ? 1 : 0; out->builds = c->tie_builds + c->tief_builds; out->build_ms = c->tie_build_ms; out->pending = cnt[0];
  return CILHIP_OK;
}

int cilhip_get_tie_rule_stats(cilhip_ctx* c, size_t* tied_queries, size_t* repointed) {
  if (!c) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  unsigned int cnt[4];
  { const int rc = read_tie_counters(c, cnt); if (rc) return rc; }
  if (tied_queries) *tied_queries = (size_t)cnt[1] + (size_t)cnt[0] + (size_t)cnt[3];      // (settled from tables + met without them, forward and reverse)
  if (repointed) *repointed = (size_t)cnt[2];
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

static void pack_T(const double L[9], const double t[3], float T[16]) {
  for (int i = 0; i < 16; ++i) T[i] = 0.f;
  T[15] = 1.f;
  for (int r = 0; r < 3; ++r) { for (int cc = 0; cc < 3; ++cc) T[cc * 4 + r] = (float)L[r * 3 + cc]; T[12 + r] = (float)t[r]; }
}

// ---- a caller's own weight evaluators -----------------------------------------------------------------------------------------
// The reference's combined-metric classes take their evaluators as template arguments (icp_single_transform_combined_metric.hpp:10-14)
// and the estimators call them per correspondence: evaluator(corr.indexInFirst, corr.indexInSecond, corr.value)
// (transform_estimation.hpp:303, :332, :432, :453).  A functor cannot cross a C boundary onto the device; with a callback set, every
// estimate brings the stored correspondence set to the host, lets the callback fill both weights of every pair, and the accumulation
// pass reads them from tables (CorrWeights::point_table) instead of evaluating a kind.  Stored order: ascending source index
// (SECOND_TO_FIRST), or the pair list's (first, second).
static int prepare_pair_weights_impl(cilhip_ctx* c);
static int prepare_pair_weights(cilhip_ctx* c) {
  if (!c->weight_fn) return CILHIP_OK;
  // (host vectors of the size of the correspondence set: an allocation failure must not cross the C boundary; neither may whatever a
  //  C++ callback lets escape)
  try {
    return prepare_pair_weights_impl(c);
  } catch (const std::bad_alloc&) {
    return fail(c, CILHIP_ERR_HIP, "pair-weight callback: out of host memory for the correspondence set");
  } catch (...) {
    return fail(c, CILHIP_ERR_INVALID, "pair-weight callback: an exception escaped the callback");
  }
}
static int prepare_pair_weights_impl(cilhip_ctx* c) {
  const bool pairs = c->have_pairs;
  const size_t slots = pairs ? c->pairs.count : c->ns;      // stream positions
  if (2 * slots > c->d_wtab.capacity() || !c->d_wtab || !c->d_wtab_in) {
    c->d_wtab.reset(); c->d_wtab_in.reset();
    const size_t cap = slots ? slots : 1;
    CK(c, c->d_wtab.alloc(2 * cap));
    CK(c, c->d_wtab_in.alloc(2 * cap));
  }
  const size_t half = c->d_wtab.capacity() / 2;      // the plane weights' table follows the point weights' (corr_weights_of)
  if (slots == 0) return CILHIP_OK;
  std::vector<uint64_t> i1(slots), i2(slots);
  std::vector<float> val(slots), wq(slots, 0.0f), wl(slots, 0.0f);
  size_t cnt = 0;
  if (pairs) {
    std::vector<uint32_t> f(slots), sc(slots);
    CK(c, hipMemcpyAsync(f.data(), c->pairs.first, slots * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipMemcpyAsync(sc.data(), c->pairs.second, slots * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipMemcpyAsync(val.data(), c->pairs.d2, slots * 4, hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < slots; ++k) { i1[k] = f[k]; i2[k] = sc[k]; }
    cnt = slots;
  } else {
    std::vector<uint32_t> idx(slots);
    std::vector<float> d2(slots);
    const int rc = cilhip_get_nn(c, idx.data(), d2.data(), CILHIP_MEM_HOST);
    if (rc) return rc;
    for (size_t i = 0; i < slots; ++i)
      if (idx[i] != NONE_U32) { i1[cnt] = idx[i]; i2[cnt] = i; val[cnt] = d2[i]; ++cnt; }
  }
  if (cnt) c->weight_fn(c->weight_user, i1.data(), i2.data(), val.data(), cnt, wq.data(), wl.data());
  if (pairs) {
    CK(c, hipMemcpyAsync(c->d_wtab, wq.data(), slots * 4, hipMemcpyHostToDevice, c->stream));
    CK(c, hipMemcpyAsync(c->d_wtab + half, wl.data(), slots * 4, hipMemcpyHostToDevice, c->stream));
  } else {
    // by original source index (unmatched: 0, never read), then into the sorted order the pass streams over
    std::vector<float> oq(slots, 0.0f), ol(slots, 0.0f);
    for (size_t k = 0; k < cnt; ++k) { oq[i2[k]] = wq[k]; ol[i2[k]] = wl[k]; }
    CK(c, hipMemcpyAsync(c->d_wtab_in, oq.data(), slots * 4, hipMemcpyHostToDevice, c->stream));
    CK(c, hipMemcpyAsync(c->d_wtab_in + half, ol.data(), slots * 4, hipMemcpyHostToDevice, c->stream));
    launch_gather1_by_w(c->d_src_sorted, c->d_wtab_in, (uint32_t)slots, c->d_wtab, c->stream);
    launch_gather1_by_w(c->d_src_sorted, c->d_wtab_in + half, (uint32_t)slots, c->d_wtab + half, c->stream);
  }
  CK(c, hipStreamSynchronize(c->stream));      // (the host vectors go out of scope)
  return CILHIP_OK;
}

// Accumulate over the stored matches (transform = nn_T) and bring the reduced sums to the host.
static int accumulate_stored(cilhip_ctx* c, int metric, const double innerL[9], const double innert[3], double sums[SUMS_MAX],
                             const CorrWeights* cw = nullptr) {
  IcpState hs;
  launch_init_state(c->d_state, c->nn_T, c->src_mean, c->stream);
  if (innerL) {
    CK(c, hipMemcpyAsync(&hs, c->d_state, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 9; ++i) { hs.innerL[i] = (float)innerL[i]; hs.dLd[i] = innerL[i]; }
    for (int i = 0; i < 3; ++i) { hs.innert[i] = (float)innert[i]; hs.dtd[i] = innert[i]; }
    CK(c, hipMemcpyAsync(c->d_state, &hs, sizeof(hs), hipMemcpyHostToDevice, c->stream));
  }
  IterArgs a = make_iter_args(c, 0.0f);
  if (cw) a.cw = *cw;
  // (a pair list -- FIRST_TO_SECOND / BOTH -- carries its own view of the source, per pair)
  if (c->have_pairs) {
    a.src = c->pairs.src_view; a.ns = c->pairs.count; a.nn_pos = c->pairs.posd; a.nn_d2 = c->pairs.d2;
    a.src_nrm = (c->d_src_nrm && c->symmetric) ? c->pairs.nrm_view : nullptr;
  }
  const int nb = iter_num_blocks(a.ns);
  for (int i = 0; i < SUMS_MAX; ++i) sums[i] = 0.0;
  if (a.ns == 0) return CILHIP_OK;
  const int grc = ensure_partial_rows(c, (size_t)nb);
  if (grc) return grc;
  a.partials = c->d_partials;
  launch_iter(a, metric, false, false, nb, c->stream);
  launch_reduce_partials(c->d_partials, nb, c->d_stage, c->d_sums, c->stream);
  CK(c, hipGetLastError());
  CK(c, hipMemcpyAsync(sums, c->d_sums, SUMS_MAX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}

int cilhip_estimate_point_to_point(cilhip_ctx* c, float dT[16], double* sums_out, int* ok) {
  if (!c || !dT) return CILHIP_ERR_INVALID;
  { const int prc = materialize_pending(c); if (prc) return prc; }
  if (!c->have_nn) return fail(c, CILHIP_ERR_INVALID, "estimate: run find_correspondences first");
  CK(c, hipSetDevice(c->device));
  double sums[SUMS_MAX];
  int rc = accumulate_stored(c, IM_KABSCH, nullptr, nullptr, sums);
  if (rc) return rc;
  double L[9], t[3];
  kabsch_from_sums(sums, L, t);
  pack_T(L, t, dT);
  if (sums_out) memcpy(sums_out, sums, 16 * sizeof(double));
  if (ok) *ok = sums[0] >= 3.0;
  return CILHIP_OK;
}

int cilhip_estimate_combined(cilhip_ctx* c, float w_p2p, float w_p2pl, size_t max_iter, float conv_tol, float dT[16],
                             double* AtA_out, double* Atb_out, int* converged) {
  if (!c || !dT) return CILHIP_ERR_INVALID;
  { const int prc = materialize_pending(c); if (prc) return prc; }
  if (!c->have_nn && !c->have_pairs) return fail(c, CILHIP_ERR_INVALID, "estimate: run find_correspondences first");
  CK(c, hipSetDevice(c->device));
  { const int wrc = prepare_pair_weights(c); if (wrc) return wrc; }
  double L[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  memcpy(dT, kIdentity16, sizeof(kIdentity16));
  if (converged) *converged = 0;
  if (AtA_out) for (int i = 0; i < 36; ++i) AtA_out[i] = 0.0;
  if (Atb_out) for (int i = 0; i < 6; ++i) Atb_out[i] = 0.0;
  const bool wp = w_p2p > 0.0f, wl = w_p2pl > 0.0f;
  if (!wp && !wl) return CILHIP_OK;                      // transform_estimation.hpp:264-272
  if (wl && !c->has_normals) return CILHIP_OK;           // dst_p.cols() != dst_n.cols() -> identity, false
  const int metric = (wp && wl) ? IM_BOTH : (wl ? IM_PLANE : IM_POINT);
  float smt[3];
  transform_point(c->nn_T, c->src_mean[0], c->src_mean[1], c->src_mean[2], smt[0], smt[1], smt[2]);
  int conv = 0;
  const CorrWeights cw = corr_weights_of(c, true, w_p2p, w_p2pl);
  if (max_iter == 0) {      // the loop body never runs; "no usable terms" (no correspondences) still means identity (:264-272)
    double sums[SUMS_MAX];
    const int rc = accumulate_stored(c, metric, L, t, sums, &cw);
    if (rc) return rc;
    if (!(sums[0] > 0.0)) return CILHIP_OK;
  }
  for (size_t it = 0; it < max_iter; ++it) {
    double sums[SUMS_MAX];
    int rc = accumulate_stored(c, metric, L, t, sums, &cw);
    if (rc) return rc;
    if (!(sums[0] > 0.0)) return CILHIP_OK;              // no correspondences: identity
    double AtA[36], Atb[6], dth[6];
    if (cw.enabled) gn_normal_equations(sums, wp ? 1.0 : 0.0, wl ? 1.0 : 0.0, AtA, Atb, true);   // (metric weights inside the per-pair weights)
    else gn_normal_equations(sums, wp ? (double)w_p2p : 0.0, wl ? (double)w_p2pl : 0.0, AtA, Atb);
    if (it == 0) {
      if (AtA_out) memcpy(AtA_out, AtA, sizeof(AtA));
      if (Atb_out) memcpy(Atb_out, Atb, sizeof(Atb));
    }
    ldlt6_solve(AtA, Atb, dth);
    rigid_gn_update(dth, L, t);
    double nrm = 0.0;
    for (int i = 0; i < 6; ++i) nrm += dth[i] * dth[i];
    if (std::sqrt(nrm) < (double)conv_tol) { conv = 1; break; }
  }
  double tt[3];
  for (int r = 0; r < 3; ++r)
    tt[r] = t[r] - (L[r * 3] * (double)smt[0] + L[r * 3 + 1] * (double)smt[1] + L[r * 3 + 2] * (double)smt[2]) + (double)c->dst_mean[r];
  pack_T(L, tt, dT);
  if (converged) *converged = conv;
  return CILHIP_OK;
}

// ---- two correspondence sets in one combined-metric estimate: CorrespondenceSearchCombinedMetricCombiner -------------
// (registration/correspondence_search_combined_metric_combiner.hpp:8-81: the point-to-point terms read one engine's
//  correspondences, the point-to-plane terms another's -- other radius, features, filters -- over the same two clouds.)
// Each context accumulates its own block of the sums over its own stored matches (the point block, slots [28, 44), on
// c_point; the plane block, slots [0, 28), on c_plane); the normal equations are assembled from the two.
static int combined_two_sets_step(cilhip_ctx* cp, cilhip_ctx* cl, bool wp, bool wl, float w_p2p, float w_p2pl, const double L[9], const double t[3],
                                  double sums[SUMS_MAX], bool* weighted_out) {
  CorrWeights cwp = corr_weights_of(cp, true, w_p2p, w_p2pl), cwl = corr_weights_of(cl, true, w_p2p, w_p2pl);
  const bool any = cwp.enabled || cwl.enabled;      // (some evaluator is not Unity: both blocks then carry their metric weight per pair)
  cwp.enabled = cwl.enabled = any ? 1 : 0;
  *weighted_out = any;
  for (int i = 0; i < SUMS_MAX; ++i) sums[i] = 0.0;
  double s1[SUMS_MAX], s2[SUMS_MAX];
  if (wp) {
    CK(cp, hipSetDevice(cp->device));
    const int rc = accumulate_stored(cp, IM_POINT, L, t, s1, &cwp);
    if (rc) return rc;
    for (int i = 28; i < 44; ++i) sums[i] = s1[i];
    if (!(s1[0] > 0.0)) sums[43] = 0.0;
  }
  if (wl) {
    CK(cl, hipSetDevice(cl->device));
    const int rc = accumulate_stored(cl, IM_PLANE, L, t, s2, &cwl);
    if (rc) { if (cl != cp) cp->err = cl->err; return rc; }
    for (int i = 0; i < 28; ++i) sums[i] = s2[i];
  }
  // slot 0 = the plane set's count; the point set's count travels in slot 43 (sum of the unit weights) -- keep a copy where
  // the caller can tell "no point correspondences" from "no plane correspondences"
  sums[44] = wp ? s1[0] : 0.0;
  return CILHIP_OK;
}

int cilhip_estimate_combined_two_sets(cilhip_ctx* cp, cilhip_ctx* cl, float w_p2p, float w_p2pl, size_t max_iter, float conv_tol, float dT[16],
                                      int* converged) {
  if (!cp || !cl || !dT) return CILHIP_ERR_INVALID;
  static_assert(SUMS_MAX >= 45, "slot 44 carries the point set's count");
  { int prc = materialize_pending(cp); if (prc) return prc; prc = materialize_pending(cl); if (prc) { cp->err = cl->err; return prc; } }
  if (!cp->have_nn || !cl->have_nn)
    return fail(cp, CILHIP_ERR_INVALID, "estimate (two sets): both engines need stored SECOND_TO_FIRST correspondences (find_correspondences first)");
  if (memcmp(cp->nn_T, cl->nn_T, sizeof(cp->nn_T)) != 0) return fail(cp, CILHIP_ERR_INVALID, "estimate (two sets): the two engines searched under different transforms");
  if (cp->ns != cl->ns || cp->grid.n != cl->grid.n) return fail(cp, CILHIP_ERR_INVALID, "estimate (two sets): the two engines hold different clouds");
  { int wrc = prepare_pair_weights(cp); if (wrc) return wrc; if (cl != cp) { wrc = prepare_pair_weights(cl); if (wrc) { cp->err = cl->err; return wrc; } } }
  double L[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  memcpy(dT, kIdentity16, sizeof(kIdentity16));
  if (converged) *converged = 0;
  bool wp = w_p2p > 0.0f, wl = w_p2pl > 0.0f;
  if (!wp && !wl) return CILHIP_OK;                      // transform_estimation.hpp:264-272
  float smt[3];
  transform_point(cp->nn_T, cp->src_mean[0], cp->src_mean[1], cp->src_mean[2], smt[0], smt[1], smt[2]);
  int conv = 0;
  const size_t steps = max_iter ? max_iter : 1;          // (max_iter 0: one pass for the "no usable terms" test only)
  for (size_t it = 0; it < steps; ++it) {
    double sums[SUMS_MAX];
    bool weighted_sums = false;
    const int rc = combined_two_sets_step(cp, cl, wp, wl, w_p2p, w_p2pl, L, t, sums, &weighted_sums);
    if (rc) return rc;
    const bool has_p2p = wp && sums[44] > 0.0, has_p2pl = wl && sums[0] > 0.0;     // :264-267
    if ((!has_p2p && !has_p2pl) || (has_p2pl && !cl->has_normals)) return CILHIP_OK;   // :269-272: identity, false
    if (max_iter == 0) break;
    double AtA[36], Atb[6], dth[6];
    if (weighted_sums) gn_normal_equations(sums, has_p2p ? 1.0 : 0.0, has_p2pl ? 1.0 : 0.0, AtA, Atb, true);
    else gn_normal_equations(sums, has_p2p ? (double)w_p2p : 0.0, has_p2pl ? (double)w_p2pl : 0.0, AtA, Atb, true);
    ldlt6_solve(AtA, Atb, dth);
    rigid_gn_update(dth, L, t);
    double nrm = 0.0;
    for (int i = 0; i < 6; ++i) nrm += dth[i] * dth[i];
    if (std::sqrt(nrm) < (double)conv_tol) { conv = 1; break; }
  }
  double tt[3];
  for (int r = 0; r < 3; ++r)
    tt[r] = t[r] - (L[r * 3] * (double)smt[0] + L[r * 3 + 1] * (double)smt[1] + L[r * 3 + 2] * (double)smt[2]) + (double)cp->dst_mean[r];
  pack_T(L, tt, dT);
  if (converged) *converged = conv;
  return CILHIP_OK;
}

// CombinedMetricSingleTransformICP over a Combiner (icp_single_transform_combined_metric.hpp:169-217 with the engine of
// correspondence_search_combined_metric_combiner.hpp): per iteration both engines search under the current transform (each with
// its own radius and options), the estimator reads the two sets, the instance class composes and tests the update norm.
// Host-driven: a few synchronisations per iteration -- this is the reference's thin combination class, not the hot path.
int cilhip_icp_run_two_sets(cilhip_ctx* cp, float max_sq_point, cilhip_ctx* cl, float max_sq_plane, const cilhip_icp_params* p, const float* T0,
                            cilhip_icp_result* out) {
  if (!cp || !cl || !p || !out) return CILHIP_ERR_INVALID;
  if (p->metric != CILHIP_METRIC_COMBINED) return fail(cp, CILHIP_ERR_INVALID, "icp_run (two sets): the combined metric is what takes two correspondence sets");
  if (cp->transform_mode != 0 || cl->transform_mode != 0) return fail(cp, CILHIP_ERR_UNSUPPORTED, "icp_run (two sets): rigid transforms");
  if (cp->search_dir != 0 || cl->search_dir != 0) return fail(cp, CILHIP_ERR_UNSUPPORTED, "icp_run (two sets): SECOND_TO_FIRST engines");
  if (cp->proj_on || cl->proj_on) return fail(cp, CILHIP_ERR_UNSUPPORTED, "projective search: cilhip_icp_run_two_sets is not available");
  float T[16];
  memcpy(T, T0 ? T0 : kIdentity16, sizeof(T));
  memcpy(out->T, T, sizeof(T));
  out->iterations = 0; out->last_delta_norm = INFINITY; out->last_ncorr = 0;
  for (size_t it = 0; it < p->max_iter; ++it) {
    size_t n1 = 0, n2 = 0;
    int rc = cilhip_find_correspondences(cp, T, max_sq_point, &n1);
    if (rc) return rc;
    if (cl != cp) { rc = cilhip_find_correspondences(cl, T, max_sq_plane, &n2); if (rc) { cp->err = cl->err; return rc; } } else n2 = n1;
    float dT[16];
    int conv = 0;
    rc = cilhip_estimate_combined_two_sets(cp, cl, p->w_p2p, p->w_p2pl, p->max_opt_iter, p->opt_conv_tol, dT, &conv);
    if (rc) return rc;
    double L[9], t[3];
    for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) L[r * 3 + k] = (double)dT[k * 4 + r]; t[r] = (double)dT[12 + r]; }
    float Tn[16];
    const float delta = compose_update(L, t, T, Tn);      // rotation() polish, transform_ = tform_iter * transform_, update norm (:207-216)
    memcpy(T, Tn, sizeof(T));
    out->iterations = it + 1; out->last_delta_norm = delta; out->last_ncorr = n1 > n2 ? n1 : n2;
    if (delta < p->conv_tol) break;                       // icp_base.hpp:83
  }
  memcpy(out->T, T, sizeof(T));
  return CILHIP_OK;
}

// ---- affine variants: SimpleCombinedMetricAffineICP3f / SimplePointToPointMetricAffineICP3f ---------------------------
// Moments of the 12-unknown normal equations over the stored correspondences (matches or pair list), three streaming
// passes on the device, one copy to the host.
static int affine_accumulate(cilhip_ctx* c, bool centered, bool plane, double sums[3 * SUMS_MAX], const CorrWeights* cw = nullptr) {
  for (int i = 0; i < 3 * SUMS_MAX; ++i) sums[i] = 0.0;
  launch_init_state(c->d_state, c->nn_T, c->src_mean, c->stream);
  IterArgs a = make_iter_args(c, 0.0f);
  if (cw) a.cw = *cw;
  // (a pair list carries its own values, per pair)
  if (c->have_pairs) { a.src = c->pairs.src_view; a.ns = c->pairs.count; a.nn_pos = c->pairs.posd; a.nn_d2 = c->pairs.d2; }
  a.src_nrm = nullptr;   // (the symmetric metric exists for the rigid classes only)
  a.no_centering = centered ? 0 : 1;
  if (a.ns == 0) return CILHIP_OK;
  const int nb = iter_num_blocks(a.ns);
  const int grc = ensure_partial_rows(c, (size_t)nb);
  if (grc) return grc;
  a.partials = c->d_partials;
  const int passes[3] = {IM_AFF0, IM_AFF1, IM_AFF2};
  const int np = plane ? 3 : 1;
  for (int k = 0; k < np; ++k) {
    launch_iter(a, passes[k], false, false, nb, c->stream);
    launch_reduce_partials(c->d_partials, nb, c->d_stage, c->d_sums + k * SUMS_MAX, c->stream);
  }
  CK(c, hipGetLastError());
  CK(c, hipMemcpyAsync(sums, c->d_sums, (size_t)np * SUMS_MAX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}

int cilhip_estimate_affine(cilhip_ctx* c, float w_p2p, float w_p2pl, int centered, float dT[16], double* AtA_out,
                           double* Atb_out, size_t* n_corr, int* ok) {
  if (!c || !dT) return CILHIP_ERR_INVALID;
  { const int prc = materialize_pending(c); if (prc) return prc; }
  if (!c->have_nn && !c->have_pairs) return fail(c, CILHIP_ERR_INVALID, "estimate: run find_correspondences first");
  CK(c, hipSetDevice(c->device));
  memcpy(dT, kIdentity16, sizeof(kIdentity16));
  if (ok) *ok = 0;
  if (n_corr) *n_corr = 0;
  if (AtA_out) for (int i = 0; i < 144; ++i) AtA_out[i] = 0.0;
  if (Atb_out) for (int i = 0; i < 12; ++i) Atb_out[i] = 0.0;
  const bool wp = w_p2p > 0.0f, wl = w_p2pl > 0.0f;
  if (!wp && !wl) return CILHIP_OK;                      // transform_estimation.hpp:400-409
  if (wl && !c->has_normals) return CILHIP_OK;           // dst_p.cols() != dst_n.cols() -> identity, false
  double sums[3 * SUMS_MAX];
  // weight evaluators (the combined-metric class only: `centered` distinguishes it from the point-to-point class here)
  if (centered) { const int wrc = prepare_pair_weights(c); if (wrc) return wrc; }
  const CorrWeights cw = corr_weights_of(c, centered != 0, w_p2p, w_p2pl);
  const int rc = affine_accumulate(c, centered != 0, wl, sums, &cw);
  if (rc) return rc;
  const double n = sums[0];
  if (n_corr) *n_corr = (size_t)n;
  if (!(n > 0.0)) return CILHIP_OK;                      // no correspondences: identity, false
  double AtA[144], Atb[12], th[12];
  if (cw.enabled) affine_normal_equations(sums, sums + SUMS_MAX, sums + 2 * SUMS_MAX, wp ? 1.0 : 0.0, wl ? 1.0 : 0.0, AtA, Atb, true);      // (metric weights inside the per-pair weights)
  else affine_normal_equations(sums, sums + SUMS_MAX, sums + 2 * SUMS_MAX, wp ? (double)w_p2p : 0.0, wl ? (double)w_p2pl : 0.0, AtA, Atb);
  if (AtA_out) memcpy(AtA_out, AtA, sizeof(AtA));
  if (Atb_out) memcpy(Atb_out, Atb, sizeof(Atb));
  ldlt_solve_n(12, AtA, Atb, th);                        // :468 AtA.ldlt().solve(Atb)
  double L[9], t[3];
  for (int i = 0; i < 9; ++i) L[i] = th[i];              // :470-472 row-major linear part, then the translation
  for (int i = 0; i < 3; ++i) t[i] = th[9 + i];
  if (centered) {                                        // :473 tform = t_dst * tform * t_src
    float smt[3];
    transform_point(c->nn_T, c->src_mean[0], c->src_mean[1], c->src_mean[2], smt[0], smt[1], smt[2]);
    for (int r = 0; r < 3; ++r)
      t[r] = t[r] - (L[r * 3] * (double)smt[0] + L[r * 3 + 1] * (double)smt[1] + L[r * 3 + 2] * (double)smt[2]) + (double)c->dst_mean[r];
  }
  pack_T(L, t, dT);
  if (ok) *ok = ((wp ? 1.0 : 0.0) + (wl ? 1.0 : 0.0)) * n >= 4.0;
  return CILHIP_OK;
}

// icp_base.hpp:68-87 with the affine updateEstimate() (icp_single_transform_point_to_point_metric.hpp:46-65,
// icp_single_transform_combined_metric.hpp:173-217 without the rotation() polish): host-driven, one 12x12 solve per iteration.
int cilhip::icp_run_affine(cilhip_ctx* c, const cilhip_icp_params* p, const float* T0, cilhip_icp_result* out) {
  float T[16];
  memcpy(T, T0 ? T0 : kIdentity16, sizeof(T));
  float delta = INFINITY;
  size_t it = 0, ncorr = 0;
  hipEvent_t e_beg = event_at(c->ev, 0), e_end = event_at(c->ev, 1);
  CK(c, hipEventRecord(e_beg, c->stream));
  while (it < p->max_iter) {
    int rc = cilhip_find_correspondences(c, T, p->max_sq_dist, nullptr);
    if (rc) return rc;
    float dT[16];
    if (p->metric == CILHIP_METRIC_POINT_TO_POINT) rc = cilhip_estimate_affine(c, 1.0f, 0.0f, 0, dT, nullptr, nullptr, &ncorr, nullptr);
    else rc = cilhip_estimate_affine(c, p->w_p2p, p->w_p2pl, 1, dT, nullptr, nullptr, &ncorr, nullptr);
    if (rc) return rc;
    float Tn[16] = {0};
    Tn[15] = 1.0f;                                       // transform_ = tform_iter * transform_ (f32, Eigen affine product)
    for (int r = 0; r < 3; ++r) {
      for (int cc = 0; cc < 3; ++cc) Tn[cc * 4 + r] = dT[0 * 4 + r] * T[cc * 4 + 0] + dT[1 * 4 + r] * T[cc * 4 + 1] + dT[2 * 4 + r] * T[cc * 4 + 2];
      Tn[12 + r] = (dT[0 * 4 + r] * T[12] + dT[1 * 4 + r] * T[13] + dT[2 * 4 + r] * T[14]) + dT[12 + r];
    }
    memcpy(T, Tn, sizeof(T));
    float dn = 0.0f;
    for (int r = 0; r < 3; ++r)
      for (int cc = 0; cc < 3; ++cc) { const float v = dT[cc * 4 + r] - (r == cc ? 1.0f : 0.0f); dn += v * v; }
    for (int r = 0; r < 3; ++r) dn += dT[12 + r] * dT[12 + r];
    delta = std::sqrt(dn);
    ++it;
    if (delta < p->conv_tol) break;
  }
  CK(c, hipEventRecord(e_end, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  memcpy(out->T, T, sizeof(T));
  out->iterations = it;
  out->last_delta_norm = delta;
  out->last_ncorr = ncorr;
  // (the last iteration's cilhip_find_correspondences left the set it estimated from: what getCorrespondences() returns)
  if (it == 0) { drop_matches(c); c->have_pairs = false; } else c->matches_origin = 1;
  float ms = 0.f;
  CK(c, hipEventElapsedTime(&ms, e_beg, e_end));
  c->last_loop_ms = ms; c->last_search_ms = 0.0; c->last_acc_ms = 0.0; c->last_search_launches = 0;
  return CILHIP_OK;
}

int cilhip_set_pair_weight_callback(cilhip_ctx* c, cilhip_pair_weight_fn fn, void* user) {
  if (!c) return CILHIP_ERR_INVALID;
  c->weight_fn = fn; c->weight_user = fn ? user : nullptr;
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

int cilhip_set_shard_info(cilhip_ctx* c, uint64_t target_index_offset, const float* dst_mean, const float* src_mean) {
  if (!c) return CILHIP_ERR_INVALID;
  if (target_index_offset + (c->has_target ? c->grid.n : 0) > 0xFFFFFFFFull) return fail(c, CILHIP_ERR_INVALID, "global target indices must fit 32 bits");
  c->index_offset = (uint32_t)target_index_offset;
  c->partial_target = target_index_offset != 0 || dst_mean != nullptr;      // (the whole cloud's mean handed in: this target is a part of it)
  if (dst_mean) memcpy(c->dst_mean, dst_mean, sizeof(c->dst_mean));
  if (src_mean) memcpy(c->src_mean, src_mean, sizeof(c->src_mean));
  return CILHIP_OK;
}

int cilhip_set_slab_guard(cilhip_ctx* c, int axis, float slack, const float center[3], const float half_extent[3], const float T_part[16]) {
  if (!c) return CILHIP_ERR_INVALID;
  if (axis < 0) { c->guard_axis = -1; return CILHIP_OK; }
  if (axis > 2 || !center || !half_extent || !T_part || !(slack >= 0.0f)) return fail(c, CILHIP_ERR_INVALID, "set_slab_guard: axis 0..2, slack >= 0, box and transform required");
  c->guard_axis = axis; c->guard_slack = slack;
  memcpy(c->guard_center, center, sizeof(c->guard_center)); memcpy(c->guard_half, half_extent, sizeof(c->guard_half));
  memcpy(c->guard_T, T_part, sizeof(c->guard_T));
  return CILHIP_OK;
}

int cilhip_get_slab_violation(cilhip_ctx* c, int* out) {
  if (!c || !out) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  int v = 0;
  CK(c, hipMemcpyAsync(&v, reinterpret_cast<const char*>(c->d_state.get()) + offsetof(IcpState, slab_violation), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *out = v;
  return CILHIP_OK;
}

int cilhip_get_slab_violation_state(cilhip_ctx* c, int* violated, cilhip_icp_result* at) {
  if (!c || !violated) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  IcpState hs;
  CK(c, hipMemcpyAsync(&hs, c->d_state, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *violated = hs.slab_violation;
  if (at) {
    memcpy(at->T, hs.slab_violation ? hs.violation_T : hs.T, sizeof(hs.T));
    at->iterations = (size_t)(hs.slab_violation ? hs.violation_iter : hs.iterations);
    at->last_delta_norm = hs.slab_violation ? hs.violation_delta : hs.delta;
    at->last_ncorr = (size_t)(hs.slab_violation ? hs.violation_ncorr : hs.ncorr);
  }
  return CILHIP_OK;
}

int cilhip_icp_partial_keys(cilhip_ctx* c, uint64_t* keys_dev) {
  if (!c || !keys_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  IterArgs a = make_iter_args(c, c->run_prm.max_sq_dist);
  if (c->ns) {
    if (c->grid.n == 0) CK(c, hipMemsetAsync(c->d_nn_pos, 0xFF, (size_t)c->ns * sizeof(uint32_t), c->stream));      // (a shard without target points: every key "none")
    else if (use_tiled(c)) launch_search_tiled(a, IM_NONE, c->d_tiles, c->d_tile_center, c->d_tile_box, c->ntiles, c->stream);
    else launch_iter(a, IM_NONE, true, true, iter_num_blocks(c->ns), c->stream);
    launch_pack_keys(c->d_src_sorted, c->grid.pts, c->d_nn_pos, c->d_nn_d2, c->ns, c->index_offset,
                     reinterpret_cast<unsigned long long*>(keys_dev), c->stream);
  }
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

// the sums over the matches a key exchange has just selected into nn_pos / nn_d2 (select: enqueues that selection)
template <class Select>
static int sums_of_selected(cilhip_ctx* c, double* sums_dev, Select select) {
  const int im = iter_metric_of(c, &c->run_prm);
  IterArgs a = make_iter_args(c, c->run_prm.max_sq_dist);
  a.cw = corr_weights_of(c, &c->run_prm);
  const int nb = iter_num_blocks(c->ns);
  if (c->ns && c->grid.n) {
    select();
    launch_iter(a, im, false, false, nb, c->stream);
    launch_reduce_partials(c->d_partials, nb, c->d_stage, sums_dev, c->stream);
  } else {
    CK(c, hipMemsetAsync(sums_dev, 0, SUMS_MAX * sizeof(double), c->stream));
  }
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

int cilhip_icp_sums_from_keys(cilhip_ctx* c, const uint64_t* keys_dev, double* sums_dev) {
  if (!c || !keys_dev || !sums_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  if (!c->d_inv_perm) {
    CK(c, c->d_inv_perm.alloc(c->grid.n));
    launch_inv_perm(c->grid.pts, c->grid.n, c->d_inv_perm, c->stream);
  }
  return sums_of_selected(c, sums_dev, [&] {
    launch_keys_to_pos(c->d_src_sorted, reinterpret_cast<const unsigned long long*>(keys_dev), c->d_inv_perm, c->ns,
                       c->index_offset, c->grid.n, c->d_nn_pos, c->d_nn_d2, c->stream,
                       (tie_mode_on(c) && !c->d_tie_leaf_slot) ? c->d_tie_counters : nullptr); });
}

// The reference's tie order across target shards (extract.hip: tie_rank): after the MIN all-reduce of cilhip_icp_partial_keys' keys,
//   cilhip_icp_order_keys(ctx, win_keys_dev, order_keys_dev)   order_keys_dev[i] = where this shard's match of source point i comes in
//                                                              the query's traversal of the WHOLE target's tree, if it is at the
//                                                              winning distance; 0x7fff...f otherwise
//   all-reduce(MIN, 64-bit) of order_keys_dev                  -> the first-met point of the whole target
//   cilhip_icp_sums_from_ordered_keys(ctx, win_keys_dev, order_keys_dev, sums_dev)   accumulates the pairs whose key came back
// Needs the whole target's order tables on every shard (cilhip_load_tie_order with the shard's global indices).
int cilhip_icp_order_keys(cilhip_ctx* c, const uint64_t* win_keys_dev, uint64_t* order_keys_dev) {
  if (!c || !win_keys_dev || !order_keys_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  if (!c->d_tie_leaf_slot) return fail(c, CILHIP_ERR_INVALID, "icp_order_keys: load the whole target's tie order first (cilhip_load_tie_order)");
  if (c->tie_max_depth > 58) return fail(c, CILHIP_ERR_UNSUPPORTED, "icp_order_keys: the order tree is deeper than the 58 levels a traversal key holds");
  CK(c, hipSetDevice(c->device));
  if (!c->d_own_order) CK(c, c->d_own_order.alloc(c->ns));
  TieDev t = tie_dev_of(c);
  launch_order_keys(c->d_src_sorted, c->d_state, reinterpret_cast<const unsigned long long*>(win_keys_dev), c->d_nn_pos, c->d_nn_d2, c->ns, t,
                    c->d_own_order, reinterpret_cast<unsigned long long*>(order_keys_dev), c->stream);
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

int cilhip_icp_sums_from_ordered_keys(cilhip_ctx* c, const uint64_t* win_keys_dev, const uint64_t* order_keys_dev, double* sums_dev) {
  if (!c || !win_keys_dev || !order_keys_dev || !sums_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  if (!c->d_own_order) return fail(c, CILHIP_ERR_INVALID, "icp_sums_from_ordered_keys: cilhip_icp_order_keys first");
  CK(c, hipSetDevice(c->device));
  return sums_of_selected(c, sums_dev, [&] {
    launch_select_ordered(c->d_src_sorted, c->d_own_order, reinterpret_cast<const unsigned long long*>(order_keys_dev),
                          reinterpret_cast<const unsigned long long*>(win_keys_dev), c->ns, c->d_nn_pos, c->d_nn_d2, c->stream); });
}

int cilhip_compute_residuals(cilhip_ctx* c, int metric, float w_p2p, float w_p2pl, const float T[16], float* out, int mem) {
  if (!c || !T || !out) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  if (metric != 0 && !c->has_normals) return fail(c, CILHIP_ERR_INVALID, "compute_residuals: combined metric needs target normals");
  int rc = ensure_sorted(c, T);
  if (rc) return rc;
  c->tie_counters_fresh = false;
  rc = (c->tie_rule == 1 && tie_mode_on(c) && c->ns && c->grid.n) ? build_tie_tables(c) : CILHIP_OK;
  if (rc) return rc;
  launch_init_state(c->d_state, T, c->src_mean, c->stream, nullptr, 0, nullptr, nullptr, c->d_tie_counters);
  IterArgs a = make_iter_args(c, 3.402823466e+38f);
  DevBuf<float> staging;      // (host output: the residuals are formed on the device first)
  if (mem != CILHIP_MEM_DEVICE) CK(c, staging.alloc(c->ns));
  float* d_out = mem != CILHIP_MEM_DEVICE ? staging.get() : out;
  launch_residuals(a, metric, w_p2p, w_p2pl, d_out, c->stream);
  CK(c, hipGetLastError());
  if (metric != 0) {      // (the point-to-plane term reads the matched point's normal: which of two equidistant points matters)
    bool again = false;
    rc = tie_check_pending(c, &again);
    if (rc) return rc;
    if (again) { a = make_iter_args(c, 3.402823466e+38f); launch_residuals(a, metric, w_p2p, w_p2pl, d_out, c->stream); CK(c, hipGetLastError()); }
  }
  if (mem != CILHIP_MEM_DEVICE) {
    if (c->ns) CK(c, hipMemcpyAsync(out, d_out, (size_t)c->ns * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
  }
  return CILHIP_OK;
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

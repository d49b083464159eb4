// ctx.hpp -- the context behind the C ABI (struct cilhip_ctx) and what the host-only translation units share: c_api.hip (contexts,
// clouds, options, diagnostics, single searches and what they leave), tie_tables.hip (the order tables),
// estimate.hip (the estimates over a stored set), shard_keys.hip (the key exchange of sharded runs) and icp_loop.hip (the ICP loop
// drivers).  No kernel translation unit includes it.
#pragma once

#include "../../include/cilantro_hip/c_api.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "ctx_options.hpp"
#include "internal.hpp"
#include "loop_policy.hpp"

using namespace cilhip;

// What a context owns on the device, grouped by the event that releases it: a group is let go of by assigning an empty one
// (c_api.hip: release_target, free_source; below: drop_src_grid).  Everything else the context owns lives as long as it does.
// (declared first, destroyed last: the context's own stream outlives every buffer its work used)
struct CtxStream { StreamGuard own_stream; };
// ... of the TARGET.  Shareable members are what cilhip_share_target hands to a borrower, buffer by buffer.
struct TargetBufs {
  GridStore grid_store;           // the arrays cilhip_ctx::grid views
  SharedBuf<uint32_t> d_inv_perm;  // [n_target] original local index -> sorted position (built on first use)
  SharedBuf<uint2> d_tief_leaf_slot;  // [grid.n] the order tables of the FEATURE tree (6-D / 9-D adaptors: points + weighted normals / colours), for the
  SharedBuf<uint4> d_tief_nodes;  // feature options they were built under (dropped with any of them); TieNode::info with four dimension bits
  SharedBuf<uint2> d_tie_leaf_slot;  // [grid.n] the order tables by sorted target position (null: not loaded)
  SharedBuf<uint4> d_tie_nodes;
  int tie_max_depth = 0;          // ... and the depth of that order tree (the traversal keys hold 58 levels): set, shared and dropped with the tables
  SharedBuf<float> d_safe2;  // [grid.n] k_self_nn's table for the warm-started iteration; built with the target
  DevBuf<unsigned long long> d_winner;  // [n_target]
  DevBuf<float> d_dst_rgb;        // colour features, original order (they belong to the target they were set for)
  DevBuf<float4> d_dst_rgb_sorted;
  DevBuf<uint32_t> d_rev_pos;     // list-free loops of FIRST_TO_SECOND / BOTH: reverse matches by target position
  DevBuf<float> d_rev_d2;
  DevBuf<unsigned long long> d_proj_keys;  // [w * h] scratch of the index map build
  DevBuf<uint32_t> d_proj_map;    // [w * h] the target's index map under the current projection: sorted positions (null: not built; dropped with the target and by cilhip_set_projection)
};
// ... of the SOURCE's own grid (FIRST_TO_SECOND / BOTH) and what is laid out in its order
struct SrcGridBufs {
  GridStore src_grid_store;       // the arrays cilhip_ctx::src_grid views
  DevBuf<float4> d_src_rgb_grid;  // the source's colours in the order of the source's own grid (9-D reverse search)
  DevBuf<float> d_src_safe2;  // [ns] k_self_nn's table over the SOURCE grid: the margin test of the warm-started reverse search (k_reverse_warm)
  DevBuf<uint32_t> d_grid_to_sorted;  // [ns] source-grid position -> sorted source position (d_src_inv through the source grid's order): the fused reverse pass's duplicate test
};
// ... of the SOURCE
struct SourceBufs : SrcGridBufs {
  DevBuf<float> d_src_xyz;  // original order (kept for re-sorting)
  DevBuf<float4> d_src_sorted;  // sorted cube-major by target-grid cell under sort_T
  SortWorkspace sort_ws;          // scratch + tile table of sort_source, kept between the sorts of a source (d_tiles / d_tile_center point into it)
  DevBuf<int> d_tile_box;  // [8*ntiles] cell range of each tile's cube under the current transform (recomputed per search)
  DevBuf<unsigned long long> d_defer_mask;  // [ntiles * 32] queries the tiles hand to the clean-up pass (bit masks, rewritten by every search)
  DevBuf<float> d_src_nrm;  // optional source normals, original order (4-cloud ctor => symmetric metric)
  DevBuf<float4> d_src_nrm_sorted;
  DevBuf<uint32_t> d_nn_pos;
  DevBuf<float> d_nn_d2;
  DevBuf<float4> d_warm_rec;  // [ns] float4 + 2 x [ns] F3: match records {matched point, margin key} {normal} and the 12-byte source copy of the warm-started iterations
  DevBuf<float> d_nn_lb;  // [ns] margin keys the search-only tile kernel leaves next to nn_pos (IterArgs::nn_lb)
  DevBuf<uint2> d_rev_tie_leaf_slot;  // [ns] by position in the source grid; valid for rev_tie_T only
  DevBuf<uint4> d_rev_tie_nodes;
  DevBuf<uint32_t> d_out_idx;  // [ns] original-order results
  DevBuf<float> d_out_d2;
  DevBuf<unsigned long long> d_keys;  // [ns]
  DevBuf<unsigned long long> d_own_order;  // [ns] this shard's traversal keys of the current iteration (cilhip_icp_order_keys)
  DevBuf<float> d_src_rgb;
  DevBuf<float4> d_src_rgb_sorted;
  DevBuf<uint32_t> d_src_inv;     // ... original -> sorted source position (per sorted order)
};

struct cilhip_ctx : CtxStream, TargetBufs, SourceBufs, CtxOptions {      // (CtxOptions: every field an option sets, ctx_options.hpp)
  ~cilhip_ctx();                  // (below: events and the pinned feedback block)
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;

  // target
  bool has_target = false;
  GridDev grid{};
  bool has_normals = false;
  double grid_occ = 0.0;
  size_t grid_cells = 0;
  double build_ms = 0.0;
  float dst_mean[3] = {0, 0, 0};
  uint32_t index_offset = 0;      // global index of this shard's first target point (target-sharded runs)
  bool partial_target = false;    // this context holds only PART of the cloud the reference would index (an index shard, a spatial slab: cilhip_set_shard_info
                                  // with an offset or the whole cloud's mean): the order tables are the WHOLE cloud's -- loaded (cilhip_load_tie_order), never built here

  // source
  bool has_source = false;
  uint32_t ns = 0;
  uint2* d_tiles = nullptr;       // [ntiles] query ranges of the LDS-tiled search kernel
  float4* d_tile_center = nullptr;  // [ntiles] cube centre of each tile in source space
  float tile_axes[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  DevBuf<uint32_t> d_defer_flag;            // [1] "some tile deferred a query" (reset before, set by, every tiled search)
  DevBuf<uint32_t> d_unproven;              // [128] queries the tiles' first stage did not prove / the warm-started kernel listed (summed / zeroed by the epilogue)
  LoopPolicy policy;                           // the form an ICP iteration takes: warm_banned / far_mode belong to the cloud pair, the rest to one run (loop_policy.hpp)
  Feedback* h_feedback = nullptr;              // pinned, host-coherent: what the epilogue kernel publishes after every iteration (pacing, kernel form)
  Feedback* d_feedback = nullptr;              // the device's address of it
  unsigned int run_tag = 0;
  int last_fused_iters = 0, last_two_pass_iters = 0, last_warm_iters = 0;
  int last_rev_fused_iters = 0;      // run_reverse_loop: iterations whose warm-started reverse search accumulated the sums itself (k_reverse_warm<ACC>)
  int run_calls = 0;              // cilhip_icp_partial_sums calls since cilhip_icp_begin
  std::vector<unsigned char> iter_form;   // form of every timed search / one-pass launch of the last run (FORM_*), in launch order
  std::vector<unsigned char> trace_form;  // form of every iteration enqueued by the last run, timed or not (cilhip_get_last_run_trace)
  double form_ms[5] = {0, 0, 0, 0, 0};    // ... and the kernel time summed per form
  int form_n[5] = {0, 0, 0, 0, 0};
  DevBuf<uint32_t> d_dbg;                   // [2] cilhip_debug_counters scratch
  DevBuf<uint4> d_trace;                    // [RUN_TRACE_CAP] per-iteration loop state of the last run, written by the epilogue (cilhip_get_last_run_trace)
  uint32_t ntiles = 0;
  bool src_sorted = false;
  float sort_T[16];
  float src_mean[3] = {0, 0, 0};
  bool rec_valid = false;         // the records describe the last executed iteration's matches (inside a run)
  bool src3_valid = false;        // the 12-byte source copy matches d_src_sorted (rewritten after a re-sort)
  bool lb_fresh = false;          // ... and they belong to the search that left nn_pos (inside a run)
  int tief_builds = 0;
  unsigned int* d_tie_counters = nullptr;        // [4] TieDev::counters
  DevBuf<unsigned int> d_ticket;              // [1] k_reduce_solve's ticket (zero between launches)
  double wait_us = 0.0;                          // time spent waiting for the device to publish loop state (wait_published), accumulated: not enqueue work
  unsigned int tie_counters_host[4] = {0, 0, 0, 0};      // ... as read together with the loop state at the end of a run (read_state: one synchronisation for both)
  bool tie_counters_fresh = false;
  double tie_build_ms = 0.0;                     // host time of the last table build (tree + upload)
  int tie_builds = 0;                            // table builds on this context (diagnostics)
  // the reverse matches of FIRST_TO_SECOND / BOTH: the reference's tree is over the TRANSFORMED source, a new one per search -- once a
  // reverse search has met exactly equidistant source points (or under tie_rule 1) that tree's order tables are built (on the device) before
  // every reverse search (the loops then run host-driven, one search at a time)
  bool rev_tie_aware = false;
  bool rev_tie_valid = false;
  float rev_tie_T[16];
  int rev_tie_builds = 0;
  void* rank_comm = nullptr; int rank_comm_size = 0; DevBuf<double> d_rank_sums;      // cilhip_rank_comm_*: this process' rank in an RCCL communicator
  float src_center[3] = {0, 0, 0}, src_half[3] = {0, 0, 0};   // bounding box of the source (source coordinates): the epilogue's bound on how far a query moves per update
  cilhip_pair_weight_fn weight_fn = nullptr;    // a caller's own evaluators (cilhip_set_pair_weight_callback): the estimates call them on the host
  void* weight_user = nullptr;
  DevBuf<float> d_wtab;           // [2 * cap]: capacity() / 2 entries per table;  point / plane weights by stream position (CorrWeights::point_table / plane_table)
  DevBuf<float> d_wtab_in;        // [2 * cap] ... by original source index, as the host filled them
  bool have_nn = false;           // nn_pos/nn_d2 hold the result of a search
  bool d2_stale = false;          // ... but nn_d2 has not been formed yet (matches left by a loop whose kernels keep no distances: ensure_d2)
  float nn_T[16];                 // transform used by that search
  // after cilhip_icp_run the engine's correspondence set is the last executed iteration's (correspondence_search_kd_tree.hpp:231 through
  // icp_base.hpp:32-38): either the loop's kernels left it in nn_pos (have_nn, origin 1) or it is searched again on demand under
  // nn_T = the transform that iteration searched under (pending_matches, origin 2) -- the search is exact, so it is the same set
  bool pending_matches = false;
  float pending_max_sq = 0.0f;
  int matches_origin = 0;         // cilhip_get_last_matches_origin

  // loop state / scratch
  DevBuf<IcpState> d_state;
  DevBuf<double> d_partials;      // rows of SUMS_MAX doubles (ensure_partial_rows)
  DevBuf<double> d_stage;      // [REDUCE_STAGE_DOUBLES] stage-1 rows of the cross-block reduction
  DevBuf<double> d_sums;       // [3 * SUMS_MAX] (the affine estimator reduces three passes before one copy to the host)
  DevBuf<unsigned long long> d_count;
  DevBuf<unsigned char> d_sel_state;

  bool dst_rgb_sorted_ok = false;
  float src_nrm0[3] = {0, 0, 0};  // the first source normal (the affine feature adaptor's normal weight is |w n_0|, adaptors.hpp:113-114)
  float feat_M[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};              // L^-T of the transform being searched under (affine adaptor)
  PairSet pairs;
  GridDev src_grid{};             // grid over the source in SOURCE coordinates (built on the first FIRST_TO_SECOND / BOTH search of a source)
  bool has_src_grid = false;
  bool have_pairs = false;        // `pairs` holds the result of the last find_correspondences
  DevBuf<IcpState> d_state_id; // a state holding the identity transform (the reverse search transforms nothing)

  // cilhip_set_projection: while proj_on, searches and cilhip_icp_run associate through the target's index map (projective.hip)
  bool proj_on = false;
  ProjDev proj{};

  // sharded-run state
  cilhip_icp_params run_prm{};
  bool run_active = false;
  int guard_axis = -1;            // slab-sharded runs: see SolveArgs::guard_*
  float guard_slack = 0.0f, guard_center[3] = {0, 0, 0}, guard_half[3] = {0, 0, 0}, guard_T[16] = {0};
  float run_src_mean[3] = {0, 0, 0};

  // timing
  std::vector<unsigned int> timed_iter;      // the iterations of the last run that carried events (options "kernel_timing", "kernel_timing_stride")
  std::vector<float> timed_ms;               // ... and the kernel time of each (cilhip_get_last_iteration_timing)
  double last_loop_ms = 0.0, last_search_ms = 0.0, last_acc_ms = 0.0;
  int last_search_launches = 0;
  size_t run_nev = 0;             // sharded runs: hipEvents recorded by cilhip_icp_partial_sums since cilhip_icp_begin (3 per call)
  std::vector<hipEvent_t> ev, ev_acc;
  std::vector<hipEvent_t> ev_ar;  // ranked loop: event pairs around the sampled all-reduces since cilhip_icp_begin (cilhip_get_last_allreduce_timing)
  size_t run_nar = 0;             // ... how many of them are recorded
  double last_allreduce_ms = 0.0; int last_allreduce_n = 0;
  double run_enqueue_us = 0.0; int run_enqueue_iters = 0;      // ranked loop: host time of its enqueue calls (the paced waits for the device's feedback word excluded)
};

inline cilhip_ctx::~cilhip_ctx() {
  if (h_feedback) (void)hipHostFree(h_feedback);
  for (auto e : ev) (void)hipEventDestroy(e);
  for (auto e : ev_acc) (void)hipEventDestroy(e);
  for (auto e : ev_ar) (void)hipEventDestroy(e);
}

#define CK(ctx, call)                                                                                   \
  do {                                                                                                  \
    hipError_t e_ = (call);                                                                             \
    if (e_ != hipSuccess) {                                                                             \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                                   \
      return CILHIP_ERR_HIP;                                                                            \
    }                                                                                                   \
  } while (0)

namespace cilhip {
inline int fail(cilhip_ctx* c, int code, const char* msg) {
  if (c) c->err = msg;
  return code;
}

// The LDS-tiled kernel runs 1024-thread workgroups, two per CU: below ~2 full rounds of tiles on the
// 256 CUs the per-lane kernel (8x more, smaller workgroups) balances better (measured: per-lane wins at 1M
// points = 580 tiles, tiled wins from 2M = 1160 tiles on).
// It also needs tiles that are reasonably full (a source much sparser than the target leaves most lanes of
// a tile idle: 10M source points against an 80M-point target fill 14 % of the slots) and a target whose
// local density fits the LDS budget of a tile's region (cube + halo + one cell of drift per axis);
// otherwise every tile would be handed to the clean-up pass, which is the per-lane search done worse.
inline bool use_tiled(const cilhip_ctx* c) {
  if (c->ns >= 0x80000000ull) return false;   // the clean-up list keeps a flag in bit 31 of a query index
  if (c->tiled >= 2) return true;
  if (c->tiled != 1 || c->ntiles < 600) return false;   // (measured: 729 tiles / 1M points already favour the tiles by 4 %, 2M by 27 %)
  const double fill = (double)c->ns / ((double)c->ntiles * (double)TILE_QUERIES);
  const double region_cells = (double)(CUBE_EDGE + 3) * (CUBE_EDGE + 3) * (CUBE_EDGE + 3);
  const double density = c->grid_occ > 1.0 ? c->grid_occ - 1.0 : c->grid_occ;   // sum(count^2)/n = lambda + 1 for a Poisson cloud
  return fill >= 0.45 && density * region_cells <= 0.92 * (double)TILE_CAP;
}

inline bool filters_active(const cilhip_ctx* c) {
  return (c->inlier_fraction > 0.0 && c->inlier_fraction < 1.0) || c->one_to_one;
}

inline bool weighted(const cilhip_ctx* c) { return c->weight_fn != nullptr || c->cw_point_kind != CW_UNITY || c->cw_plane_kind != CW_UNITY; }
// a feature adaptor is in force (6-D point+normal or point+colour, 9-D point+normal+colour): correspondences are compared by feature distance
inline bool feat6(const cilhip_ctx* c) { return c->normal_weight > 0.0f || (c->feature_kind == 2 && c->color_weight > 0.0f); }
// The warm-started iteration (k_warm) needs stored matches, unit weights and the first Gauss-Newton step's plain terms -- the
// same engine conditions as the in-tile accumulation, but no tiles: it also serves clouds the tiles do not (a source much
// sparser than the target: BASELINE configs[3]).
inline bool warm_capable(const cilhip_ctx* c) {
  // (the symmetric objective -- source normals set, option symmetric_metric on -- runs warm-started too: k_warm<., ., SYM> streams the source normals)
  return c->warm_start && c->ns >= 65536 && !filters_active(c) && !weighted(c) && !feat6(c) && !c->fused;
}

// The ICP loop's first Gauss-Newton step is accumulated inside the LDS tiles of the search (one pass instead of a search
// pass + a streaming accumulation pass) whenever the plain engine runs tiled: no post-filters (they act on the complete
// match set), point features, the three-cloud metric (the symmetric objective reads source normals per pair), and not
// the A/B option "fused" (per-lane kernel) or "tile_accumulation" = 0.
inline bool tile_accumulation(const cilhip_ctx* c) {
  return c->tile_acc && use_tiled(c) && !filters_active(c) && !weighted(c) && !feat6(c) && !(c->d_src_nrm && c->symmetric) && !c->fused;
}

// option "tie_rule" is in force for this context's point searches (tie_tables.hip: the order tables)
inline bool tie_mode_on(const cilhip_ctx* c) { return c->tie_rule != 0 && !feat6(c); }

// c->fused is honoured as ONE per-lane search+accumulate kernel only by the plain engine (post-filters and feature adaptors need the stored set)
inline bool lane_fused(const cilhip_ctx* c) { return c->fused && !filters_active(c) && !feat6(c); }
// ---- what a context lets go of, and when.  A shared target array is only let go of: its last holder frees it.
// the stored matches no longer describe anything a caller may read
inline void drop_matches(cilhip_ctx* c) { c->have_nn = false; c->d2_stale = false; c->pending_matches = false; c->matches_origin = 0; }
// ... nor does the pair list (it refers to the source / target and the options it was found under).  pairs.count stays as it is: it is
// read behind have_pairs only, or straight after the search that wrote it
inline void drop_correspondences(cilhip_ctx* c) { drop_matches(c); c->have_pairs = false; }
inline void drop_src_grid(cilhip_ctx* c) {
  static_cast<SrcGridBufs&>(*c) = SrcGridBufs{};
  c->src_grid = GridDev{}; c->has_src_grid = false;
}
inline void drop_feat_tie_tables(cilhip_ctx* c) {      // (one target under one set of feature options; never shared)
  c->d_tief_leaf_slot.reset(); c->d_tief_nodes.reset();
}
inline void drop_tie_tables(cilhip_ctx* c) {      // (they describe ONE target)
  c->d_tie_leaf_slot.reset(); c->d_tie_nodes.reset(); c->tie_max_depth = 0;
}
// what a newly stored option value made stale (ctx_options.hpp: the STALE_* events a table row reports)
inline void apply_stale(cilhip_ctx* c, unsigned stale) {
  if (stale & STALE_SRC_GRID) drop_src_grid(c);
  if (stale & STALE_FEAT_ORDER) drop_feat_tie_tables(c);
  if ((stale & STALE_MATCHES) || ((stale & STALE_PENDING_MATCHES) && c->pending_matches)) drop_matches(c);
  if (stale & STALE_CORRESPONDENCES) drop_correspondences(c);
}
// event i of a list that grows on demand (c->ev: run / kernel events, c->ev_acc: the two-pass iterations' accumulation)
inline hipEvent_t event_at(std::vector<hipEvent_t>& v, size_t i) {
  while (v.size() <= i) { hipEvent_t e; (void)hipEventCreate(&e); v.push_back(e); }
  return v[i];
}

// ---- helpers the host units call across files: c_api.hip (ensure_*, set_warm_args, filters, projection, searches,
// materialize_pending), tie_tables.hip (tie_*, build_*tie_tables), estimate.hip (corr_weights_of, use_stored_set,
// icp_run_affine), icp_loop.hip (iter_metric_of)
int ensure_sorted(cilhip_ctx* c, const float T[16]);
int ensure_partial_rows(cilhip_ctx* c, size_t rows);      // d_partials holds at least `rows` rows of SUMS_MAX doubles (callers re-read c->d_partials)
int ensure_warm_buffers(cilhip_ctx* c);
void ensure_pair_records(cilhip_ctx* c);
int ensure_safe2(cilhip_ctx* c);
int ensure_feature_arrays(cilhip_ctx* c);
int ensure_reverse_buffers(cilhip_ctx* c);
void set_warm_args(const cilhip_ctx* c, IterArgs& wa);
CorrWeights corr_weights_of(const cilhip_ctx* c, const cilhip_icp_params* p);
FeatSpec feat_spec_of(const cilhip_ctx* c);
TieDev tie_dev_of(const cilhip_ctx* c);
TieDev tie_dev_rev(const cilhip_ctx* c);
int build_tie_tables(cilhip_ctx* c);
int build_rev_tie_tables(cilhip_ctx* c, const float T[16]);
int tie_prepare(cilhip_ctx* c, const char* what);
int tie_check_pending(cilhip_ctx* c, bool* again);
int apply_filters(cilhip_ctx* c);
const char* proj_conflict(const cilhip_ctx* c);      // what, of the context's settings, a projection does not run with (null: nothing)
int ensure_proj_map(cilhip_ctx* c);
IterArgs make_iter_args(cilhip_ctx* c, float max_sq);
int launch_search(cilhip_ctx* c, const IterArgs& a, int lanes = -1 /* -1: the option's own value when it names a lane count */);
int run_pair_search(cilhip_ctx* c, const IterArgs& a, float max_sq, const float T_host[16]);
int materialize_pending(cilhip_ctx* c);
void use_stored_set(const cilhip_ctx* c, IterArgs& a, bool symmetric_normals);      // the pair list's own views, for the accumulating kernels
int icp_run_affine(cilhip_ctx* c, const cilhip_icp_params* p, const float* T0, cilhip_icp_result* out);
int iter_metric_of(const cilhip_ctx* c, const cilhip_icp_params* p);      // (icp_loop.hip)
}  // namespace cilhip

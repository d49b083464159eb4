// icp_loop.hip -- the ICP loop drivers of the C ABI (c_api.h): cilhip_icp_run, the building blocks of sharded runs (cilhip_icp_begin /
// _partial_sums / _apply_sums / _state) and the ranked loop over an RCCL communicator.  Host control flow only, no kernels; the
// form an iteration takes is decided in loop_policy.hpp, the context and the helpers of the other host units these loops call are in ctx.hpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "ctx.hpp"
#include "rccl_api.hpp"

// What the accumulation kernels sum for one ICP instance.  A plane term without target normals is the reference's
// "dst_p.cols() != dst_n.cols()" case (transform_estimation.hpp:264-272: identity, false): the kernels must then never
// touch grid.nrm (it is null) -- they count the correspondences only (IM_POINT's slot 0) and the epilogue's identity
// branch (k_solve: has_p2pl && !has_normals) does the rest.
int cilhip::iter_metric_of(const cilhip_ctx* c, const cilhip_icp_params* p) {
  if (p->metric == CILHIP_METRIC_POINT_TO_POINT) return IM_KABSCH;
  const bool wp = p->w_p2p > 0.0f, wl = p->w_p2pl > 0.0f;
  if (wl && !c->has_normals) return IM_POINT;
  if (wp && wl) return IM_BOTH;
  if (wl) return IM_PLANE;
  if (wp) return IM_POINT;
  return IM_PLANE;  // no terms: sums unused, the epilogue takes the identity branch
}

static SolveArgs make_solve_args(cilhip_ctx* c, const cilhip_icp_params* p, int im, const float src_mean[3]) {
  SolveArgs sa{};
  sa.state = c->d_state;
  sa.partials = c->d_partials;
  sa.nblocks = iter_num_blocks(c->ns);
  sa.reduced = nullptr;
  sa.metric = im;
  sa.w_p2p = p->w_p2p; sa.w_p2pl = p->w_p2pl;
  if (p->metric == CILHIP_METRIC_COMBINED && weighted(c)) {   // the metric weights are inside the per-pair weights already
    sa.w_p2p = p->w_p2p > 0.0f ? 1.0f : 0.0f; sa.w_p2pl = p->w_p2pl > 0.0f ? 1.0f : 0.0f;
    sa.point_weighted = 1;
  }
  sa.conv_tol = p->conv_tol; sa.opt_conv_tol = p->opt_conv_tol;
  for (int i = 0; i < 3; ++i) { sa.dst_mean[i] = c->dst_mean[i]; sa.src_mean[i] = src_mean[i]; }
  sa.gn_last_step = 1;
  sa.has_normals = c->has_normals ? 1 : 0;
  sa.unproven_cnt = c->d_unproven;
  sa.guard_axis = c->guard_axis; sa.guard_slack = c->guard_slack;
  for (int i = 0; i < 3; ++i) { sa.guard_center[i] = c->guard_center[i]; sa.guard_half[i] = c->guard_half[i]; }
  for (int i = 0; i < 16; ++i) sa.guard_T[i] = c->guard_T[i];
  for (int i = 0; i < 3; ++i) { sa.src_center[i] = c->src_center[i]; sa.src_half[i] = c->src_half[i]; }
  sa.trace = c->d_trace;
  sa.feedback = c->d_feedback; sa.run_tag = c->run_tag;      // (the epilogue publishes the loop state: wait_published)
  return sa;
}

// Waits until iteration `need` of the current run (or its convergence) has been published.  patience_s: how long to spin;
// returns 0 and fills *v, or 1 when nothing came in that time.
static int wait_published(cilhip_ctx* c, unsigned int need, double patience_s, FbView* v) {
  const volatile Feedback* fb = c->h_feedback;
  const auto t0 = std::chrono::steady_clock::now();
  struct Acc { cilhip_ctx* c; std::chrono::steady_clock::time_point t; ~Acc() { c->wait_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t).count(); } } acc{c, t0};
  for (unsigned spins = 0;; ++spins) {
    const unsigned long long lt = fb->latest;
    if ((unsigned int)(lt >> 32) == c->run_tag) {
      const bool done = (lt & 0x80000000ull) != 0ull;
      const unsigned int iters = (unsigned int)lt & 0x7fffffffu;
      if (done || iters >= need) {
        // the slot of the latest published iteration: the device's next write goes to another slot (the host is at most two
        // iterations ahead), so this read cannot be torn; its commit word is checked all the same
        const volatile FeedbackSlot* sl = &fb->slot[iters & 3u];
        v->done = done; v->iterations = iters;
        v->unproven = sl->unproven; v->listed = sl->listed; v->delta = sl->delta; v->prev_delta = sl->prev_delta; v->step = iters ? sl->step : INFINITY;
        if (iters == 0u || sl->commit == (((unsigned long long)c->run_tag << 32) | iters)) return 0;
      }
    }
    cpu_relax(spins);
    if ((spins & 1023u) == 1023u && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > patience_s) return 1;
  }
}
// ... with the long-stall handling of cilhip_icp_run: nothing for 30 s -- a caller-owned stream may have long work of its own
// queued ahead of this run -- wait for the stream (that also surfaces a device fault); everything enqueued has then run and
// must have been published
static int wait_published_or_sync(cilhip_ctx* c, unsigned int need, FbView* v) {
  if (wait_published(c, need, 30.0, v) == 0) return CILHIP_OK;
  CK(c, hipStreamSynchronize(c->stream));
  if (wait_published(c, need, 0.01, v) == 0) return CILHIP_OK;
  return fail(c, CILHIP_ERR_HIP, "icp_run: the device stopped publishing its loop state");
}

static int read_state(cilhip_ctx* c, cilhip_icp_result* out, float* Tprev = nullptr) {
  IcpState hs;
  CK(c, hipMemcpyAsync(&hs, c->d_state, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  memcpy(c->tie_counters_host, hs.tie_counters, sizeof(c->tie_counters_host));
  c->tie_counters_fresh = true;
  memcpy(out->T, hs.T, sizeof(hs.T));
  if (Tprev) memcpy(Tprev, hs.Tprev, sizeof(hs.Tprev));
  out->iterations = (size_t)hs.iterations;
  out->last_delta_norm = hs.delta;
  out->last_ncorr = (size_t)hs.ncorr;
  return CILHIP_OK;
}

// What the engine's getCorrespondences() refers to after a run: the set of the last executed iteration, found under Tprev
// (correspondence_search_kd_tree.hpp:231 keeps it; icp_base.hpp:32-38 hands the engine out).  stored: the loop's kernels left
// it in nn_pos (the squared distances are formed again with the search's pinned arithmetic); pairs: c->pairs holds it;
// otherwise it is searched again when somebody asks (materialize_pending).
static void finish_run_matches(cilhip_ctx* c, const cilhip_icp_params* p, size_t iterations, const float Tprev[16], bool stored, bool pairs) {
  drop_correspondences(c);
  if (iterations == 0) return;
  memcpy(c->nn_T, Tprev, sizeof(c->nn_T));
  if (pairs) { c->have_pairs = true; c->matches_origin = 1; return; }
  if (stored && c->ns) {
    // (the squared distances of the stored matches are formed when somebody asks for them -- ensure_d2: a pass over the source that
    //  a caller who only wants the transform does not pay, 80 us at 10M)
    c->have_nn = true; c->d2_stale = true; c->matches_origin = 1;
  } else {
    c->pending_matches = true; c->pending_max_sq = p->max_sq_dist; c->matches_origin = 2;
  }
}

// ---- cilhip_icp_run: what each of its three loops starts from (the caller's parameters, the kernels' argument blocks, per-run constants)
struct RunSetup {
  const cilhip_icp_params* p;
  const float* Ti;            // the initial transform
  cilhip_icp_result* out;
  IterArgs a;
  SolveArgs sa;
  int im;                     // what the accumulation kernels sum (IM_*)
  bool affine;
  bool gn;                    // Gauss-Newton steps inside an iteration (the rigid combined metric)
  size_t opt_steps;
  int nb, nb_aff;             // rows of the streaming accumulation: the rigid terms' / the affine moments'
  hipEvent_t e_beg, e_end;
};

// grows d_partials and points the argument blocks at it
static int grow_partials(cilhip_ctx* c, RunSetup& r, size_t rows) {
  const int rc = ensure_partial_rows(c, rows);
  if (rc) return rc;
  r.a.partials = c->d_partials; r.a.tile_partials = c->d_partials; r.sa.partials = c->d_partials;
  return CILHIP_OK;
}

// The warm-started iteration (k_warm): search + accumulation from the previous iteration's matches.  The first one after the
// search-only forms gathers through the stored positions, takes the margin keys those searches left (nn_lb) and writes a match
// record per query; after a tile iteration with the accumulation inside -- which writes the records itself -- and from then
// on, the records are streamed instead.  Returns whether this was such a first one.
static bool launch_warm_iteration(cilhip_ctx* c, const IterArgs& a, int im) {
  IterArgs wa = a;
  wa.warm_pos = c->d_nn_pos;
  wa.safe2 = c->d_safe2;
  wa.warm_far_sq = 0.25f * c->grid.cell * c->grid.cell;
  set_warm_args(c, wa);
  wa.nn_lb = c->d_nn_lb; wa.lb_valid = c->lb_fresh ? 1 : 0;
  const bool first = !c->rec_valid;
  launch_warm(wa, im, first ? 1 : 2, warm_num_blocks(c->ns), c->stream);
  c->rec_valid = true; c->lb_fresh = false;
  return first;
}

// Search + accumulation of the first Gauss-Newton step inside the LDS tiles (one pass).  Returns whether the tile also left the
// match records of the warm-started form (records: wanted), having counted the queries a warm-started iteration would search.
static bool launch_tile_one_pass(cilhip_ctx* c, const IterArgs& a, int im, bool store_matches, bool records) {
  IterArgs fa = a;
  fa.store_matches = store_matches ? 1 : 0;
  fa.partials = c->d_partials + (size_t)c->ntiles * SUMS_MAX;
  const bool recs = records && c->tile_records && store_matches;
  if (recs) set_warm_args(c, fa);
  launch_search_tiled(fa, im, c->d_tiles, c->d_tile_center, c->d_tile_box, c->ntiles, c->stream);
  c->rec_valid = recs; c->lb_fresh = false;
  return recs;
}

// Long runs ("iterate until converged" with a large max_iter): the kernels of a converged run return at once, but the
// post-filter / reduction launches do not look at the flag, so look at it from the host every 32nd iteration and stop
// enqueueing.  Short runs (the reference's default is 15) stay free of host round trips.
static int stop_when_done(cilhip_ctx* c, size_t it, size_t max_iter, bool* stop) {
  *stop = false;
  if (!(max_iter > 64 && (it + 1) % 32 == 0 && it + 1 < max_iter)) return CILHIP_OK;
  int done = 0;
  CK(c, hipMemcpyAsync(&done, reinterpret_cast<const char*>(c->d_state.get()) + offsetof(IcpState, done), sizeof(int), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  *stop = done != 0;
  return CILHIP_OK;
}

// The end of every loop: the result, what getCorrespondences() refers to from now on, the loop's time (last_acc_ms: the caller's)
static int finish_run(cilhip_ctx* c, const RunSetup& r, bool stored, bool pairs) {
  CK(c, hipEventRecord(r.e_end, c->stream));
  CK(c, hipGetLastError());
  float Tprev[16];
  const int rc = read_state(c, r.out, Tprev);
  if (rc) return rc;
  finish_run_matches(c, r.p, r.out->iterations, Tprev, stored, pairs && r.out->iterations > 0);
  float ms = 0.f;
  CK(c, hipEventElapsedTime(&ms, r.e_beg, r.e_end));
  c->last_loop_ms = ms; c->last_search_ms = 0.0; c->last_search_launches = 0;
  return CILHIP_OK;
}

// FIRST_TO_SECOND / BOTH without post-filters: the loop needs the SUMS over the correspondence set, not the sorted list: the
// reverse matches are found through the inverse of the (rigid) transform against a grid over the source built once, and
// accumulated where they are found (BOTH: forward pass + the reverse matches that are not reciprocal duplicates; reciprocal:
// the duplicates alone) -- no per-iteration index, no sort, no host round trip: every iteration is enqueued back to back.
static int run_reverse_loop(cilhip_ctx* c, RunSetup& r) {
  const cilhip_icp_params* p = r.p;
  IterArgs& a = r.a;
  SolveArgs& sa = r.sa;
  const int im = r.im;
  int rc = ensure_reverse_buffers(c);
  if (rc) return rc;
  FeatSpec rf = a.feat;
  rf.src = c->src_grid.nrm;
  if (rf.dst2) rf.src2 = c->d_src_rgb_grid;
  if (feat6(c) && (!rf.src || !rf.dst || (rf.dst2 && !rf.src2))) return fail(c, CILHIP_ERR_INVALID, "feature search: both clouds' feature vectors are needed");
  const int nb_f = iter_num_blocks(c->ns), nb_r = iter_num_blocks(c->grid.n);
  // BOTH: the forward half runs warm-started from its third iteration on (search + accumulation in k_warm, like the plain loop's
  // steady state: exact whatever the source's distance, and these loops have no cheaper forward form to go back to)
  const bool fwd_wcap = c->search_dir == 2 && warm_capable(c);
  if (fwd_wcap) { rc = ensure_safe2(c); if (rc) return rc; rc = ensure_warm_buffers(c); if (rc) return rc; }
  const int nb_w = fwd_wcap ? warm_num_blocks(c->ns) : 0;
  const int nb_fmax = std::max(nb_f, nb_w);
  // the warm-started reverse search accumulates the first step's sums itself (one pass over the target; per-pair weights keep the separate pass)
  const bool rev_fusable = c->reverse_warm && !feat6(c) && !a.cw.enabled && c->d_src_safe2 != nullptr;
  const int nb_rw = rev_fusable ? reverse_warm_blocks(c->grid.n) : 0;
  const int nb_rmax = std::max(nb_r, nb_rw);
  rc = ensure_partial_rows(c, (size_t)(nb_fmax + nb_rmax));
  if (rc) return rc;
  const bool both_union = c->search_dir == 2 && !c->reciprocal;
  const int rmode = c->search_dir == 1 ? 1 : (c->reciprocal ? 3 : 2);
  // rows: the reverse matches' first, the forward half's (streaming pass or warm-started kernel) right behind them
  IterArgs ar = a;
  ar.partials = c->d_partials;
  a.nn_d2 = nullptr;
  c->rec_valid = false; c->lb_fresh = false;
  c->policy.begin_run(c->warm_enter * c->grid.cell);
  c->last_fused_iters = c->last_two_pass_iters = c->last_warm_iters = c->last_rev_fused_iters = 0;
  for (size_t it = 0; it < p->max_iter; ++it) {
    bool fwd_warm = false;
    const bool rev_fused = rev_fusable && it >= 1;      // (this iteration's reverse search starts from the previous matches and accumulates)
    for (size_t st = 0; st < r.opt_steps; ++st) {
      a.skip_if_inner_done = ar.skip_if_inner_done = (st > 0);
      const int rev_rows = (rev_fused && st == 0) ? nb_rw : nb_r;
      a.partials = c->d_partials + (size_t)rev_rows * SUMS_MAX; a.tile_partials = a.partials;
      if (st == 0) {
        if (c->search_dir == 2) {
          fwd_warm = fwd_wcap && it >= 2;
          if (fwd_warm) {
            launch_warm_iteration(c, a, im);
            ++c->last_warm_iters;
          } else {
            IterArgs sa2 = a;
            if (fwd_wcap) { sa2.nn_lb = c->d_nn_lb; c->lb_fresh = true; }      // (the margin keys the first warm-started iteration starts from)
            c->rec_valid = false;
            const int src_rc = launch_search(c, sa2);
            if (src_rc) return src_rc;
          }
        }
        // (from the second iteration on d_rev_pos holds the previous reverse matches: the search starts from them)
        const float* warm_tab = (it >= 1 && c->reverse_warm && !feat6(c)) ? c->d_src_safe2 : nullptr;
        RevFused rfu{};
        rfu.metric = im; rfu.mode = rmode; rfu.fwd_pos = c->d_nn_pos; rfu.src_inv = c->d_src_inv; rfu.grid_to_sorted = c->d_grid_to_sorted; rfu.partials = c->d_partials;
        for (int k = 0; k < 3; ++k) rfu.dst_mean[k] = a.dst_mean[k];
        if (rev_fused) ++c->last_rev_fused_iters;
        { const TieDev rt = tie_dev_rev(c); launch_reverse_search_rigid(c->grid, c->src_grid, c->d_state, p->max_sq_dist, c->d_rev_pos, c->d_rev_d2, c->stream, feat6(c) ? &rf : nullptr, &rt, warm_tab, rev_fused ? &rfu : nullptr); }
      }
      const bool fwd_in_kernel = fwd_warm && st == 0;      // (the warm-started kernel accumulated the first step's terms itself)
      if (both_union && !fwd_in_kernel) launch_iter(a, im, false, false, nb_f, c->stream);
      if (!(rev_fused && st == 0)) launch_acc_reverse(ar, im, c->src_grid.pts, c->d_rev_pos, c->grid.n, rmode, c->d_nn_pos, c->d_src_inv, nb_r, c->stream);
      sa.gn_last_step = (st + 1 == r.opt_steps);
      const int rows_total = rev_rows + (both_union ? (fwd_in_kernel ? nb_w : nb_f) : 0);
      const int rows = launch_reduce_stage1(c->d_partials, rows_total, c->d_stage, c->stream);
      sa.partials = rows ? c->d_stage : c->d_partials;
      sa.nblocks = rows ? rows : rows_total;
      sa.reduced = nullptr;
      launch_solve(sa, c->stream);
    }
    bool stop = false;
    rc = stop_when_done(c, it, p->max_iter, &stop);
    if (rc) return rc;
    if (stop) break;
  }
  c->last_acc_ms = 0.0;
  return finish_run(c, r, false, false);      // (nothing was listed: searched again on demand)
}

// FIRST_TO_SECOND / BOTH otherwise: the correspondence set is a pair list rebuilt every iteration (a grid over the transformed
// source, like the reference's per-iteration kd-tree); host-driven loop, the accumulation kernels stream over the pairs
static int run_pair_list_loop(cilhip_ctx* c, RunSetup& r) {
  const cilhip_icp_params* p = r.p;
  SolveArgs& sa = r.sa;
  for (size_t it = 0; it < p->max_iter; ++it) {
    int rc = run_pair_search(c, r.a, p->max_sq_dist, it == 0 ? r.Ti : r.out->T);
    if (rc) return rc;
    IterArgs pa = r.a;
    use_stored_set(c, pa, true);  // (nn_d2 per pair: corr.value -- the 6-D distance under a feature adaptor -- for the weight evaluators)
    const int pnb = iter_num_blocks(pa.ns);
    rc = ensure_partial_rows(c, (size_t)pnb);
    if (rc) return rc;
    pa.partials = c->d_partials;
    for (size_t st = 0; st < r.opt_steps; ++st) {
      pa.skip_if_inner_done = (st > 0);
      sa.gn_last_step = (st + 1 == r.opt_steps);
      if (pa.ns) {
        launch_iter(pa, r.im, false, false, pnb, c->stream);
        const int rows = launch_reduce_stage1(c->d_partials, pnb, c->d_stage, c->stream);
        sa.partials = rows ? c->d_stage : c->d_partials;
        sa.nblocks = rows ? rows : pnb;
        sa.reduced = nullptr;
      } else {
        CK(c, hipMemsetAsync(c->d_sums, 0, SUMS_MAX * sizeof(double), c->stream));
        sa.nblocks = 0;
        sa.reduced = c->d_sums;
      }
      launch_solve(sa, c->stream);
    }
    rc = read_state(c, r.out);
    if (rc) return rc;
    if (r.out->last_delta_norm < p->conv_tol) break;   // the device sets `done` by the same test (icp_base.hpp:83)
  }
  c->last_acc_ms = 0.0;
  return finish_run(c, r, false, true);      // c->pairs: the last iteration's list
}

// A projection is set (cilhip_set_projection): host-paced like run_pair_list_loop -- the projective search over the target's index map
// leaves its matches in nn_pos, the post-filter and the streaming accumulation run over them as after any search-only form, the
// epilogue solves, and the host reads the loop state after every iteration.  No tiled or warm forms.
static int run_projective_loop(cilhip_ctx* c, RunSetup& r) {
  const cilhip_icp_params* p = r.p;
  IterArgs& a = r.a;
  SolveArgs& sa = r.sa;
  CK(c, hipEventRecord(r.e_beg, c->stream));
  int rc = ensure_proj_map(c);
  if (rc) return rc;
  c->rec_valid = false; c->lb_fresh = false;
  c->last_fused_iters = c->last_two_pass_iters = c->last_warm_iters = c->last_rev_fused_iters = 0;
  c->iter_form.clear(); c->trace_form.clear(); c->timed_iter.clear();
  for (int k = 0; k < 5; ++k) { c->form_ms[k] = 0.0; c->form_n[k] = 0; }
  for (size_t it = 0; it < p->max_iter; ++it) {
    if (c->ns) {
      launch_proj_search(c->d_src_sorted, c->ns, c->d_state, c->grid.pts, c->proj, c->d_proj_map, p->max_sq_dist, c->d_nn_pos, c->d_nn_d2, c->stream);
      rc = apply_filters(c);
      if (rc) return rc;
    }
    ++c->last_two_pass_iters;
    for (size_t st = 0; st < r.opt_steps; ++st) {
      a.skip_if_inner_done = (st > 0);
      sa.gn_last_step = (st + 1 == r.opt_steps);
      if (c->ns) {
        launch_iter(a, r.im, false, false, r.nb, c->stream);
        launch_reduce_and_solve(c->d_partials, r.nb, c->d_stage, nullptr, sa, c->stream);
      } else {
        launch_solve(sa, c->stream);
      }
    }
    rc = read_state(c, r.out);
    if (rc) return rc;
    if (r.out->last_delta_norm < p->conv_tol) break;   // the device sets `done` by the same test (icp_base.hpp:83)
  }
  c->last_acc_ms = 0.0;
  // the last iteration's matches are in nn_pos, with the values its search formed (a post-filtered set is searched again on demand, as after the grid loop)
  rc = finish_run(c, r, !filters_active(c), false);
  if (rc == CILHIP_OK && c->have_nn) c->d2_stale = false;
  return rc;
}

// FIRST_TO_SECOND / BOTH: which of the two loops
static int run_other_directions(cilhip_ctx* c, RunSetup& r) {
  if (c->index_offset) return fail(c, CILHIP_ERR_UNSUPPORTED, "search directions other than SECOND_TO_FIRST are not available on target shards");
  if (feat6(c)) { const int rc = ensure_feature_arrays(c); if (rc) return rc; r.a.feat = feat_spec_of(c); }
  // (a weight evaluator over FEATURE distances reads them per pair: those loops go through the pair list)
  const bool feat_weights = feat6(c) && r.a.cw.enabled;
  CK(c, hipEventRecord(r.e_beg, c->stream));
  bool t0_rigid = true;
  for (int i = 0; i < 3 && t0_rigid; ++i)
    for (int j = 0; j < 3; ++j) {
      const double dot = (double)r.Ti[i * 4] * r.Ti[j * 4] + (double)r.Ti[i * 4 + 1] * r.Ti[j * 4 + 1] + (double)r.Ti[i * 4 + 2] * r.Ti[j * 4 + 2];
      if (std::fabs(dot - (i == j ? 1.0 : 0.0)) > 1e-5) t0_rigid = false;
    }
  const bool list_free = !filters_active(c) && !(c->d_src_nrm && c->symmetric) && t0_rigid && c->ns && c->grid.n && !feat_weights && !(c->rev_tie_aware && tie_mode_on(c));
  return list_free ? run_reverse_loop(c, r) : run_pair_list_loop(c, r);
}

// ---- the forward (SECOND_TO_FIRST) loop
// Tiled runs are PACED: the host stays at most two iterations ahead of the device and looks at the loop state of
// iteration it - 2 before it enqueues iteration it (a pinned copy + an event per iteration; the device never waits: an
// iteration takes hundreds of microseconds, the look a few).  That buys (1) no launches after convergence and (2) the
// choice of the kernel FORM per iteration: while the octant stage leaves many queries unproven (source far from
// alignment: first iterations of a registration) the search runs with its in-LDS 3x3x3 second pass and a separate
// streaming accumulation; once nearly all are proven, search + accumulation run as one pass inside the tiles.
struct ForwardRun {
  // per-run constants
  bool tile_acc;              // the tiles may accumulate (the rigid classes' terms only)
  bool timing;
  bool wcap;                  // the warm-started form is available
  bool fwcap;                 // ... the feature adaptors' (feat_warm.hip)
  bool paced;
  int glanes;                 // lanes per query of the cooperative search's cold iterations (0: none)
  // what the loop has seen and done so far
  bool group_now = false;
  size_t next_probe = 0, probe_gap = 8;
  bool feat_warm_now = false;
  unsigned int feat_judged = 0;
  bool all_stored = true;     // every iteration enqueued left its matches in nn_pos (finish_run_matches)
  bool prev_stored = false;   // ... the previous one did
  size_t nev = 2, nacc = 0;   // events used (c->ev / c->ev_acc)
};

// Before iteration `it` is enqueued: from what the device has published, the forms of the iterations to come (c->policy.on /
// far_mode, f.group_now, f.feat_warm_now).  *stop: the run has converged.
static int pace_forward(cilhip_ctx* c, ForwardRun& f, size_t it, bool* stop) {
  LoopPolicy& pol = c->policy;
  const bool auto_lanes = f.glanes && c->group_lanes < 0;      // the loop decides between the cooperative and the one-lane search
  const bool warm_auto = f.wcap && c->warm_start == 1;
  *stop = true;
  if (it == 1 && warm_auto && !pol.warm_banned && form_counted(form_of(c->trace_form, 1u))) {
    // The SECOND iteration can already run warm-started when the first one moved the source by a small fraction of a cell (a
    // source that starts aligned: tracking, a refinement pass) and its kernels' own forecast agrees: worth one look at the
    // first iteration's result before the second is enqueued (the device idles for the host's reaction once per run; a cold
    // iteration costs three times a warm one).
    FbView fv;
    const int rc = wait_published_or_sync(c, 1u, &fv);
    if (rc) return rc;
    if (fv.done) return CILHIP_OK;
    const int fo = form_of(c->trace_form, 1u);
    pol.note_unproven(fo, fv.unproven, c->ns);
    if (auto_lanes && fv.iterations == 1u) f.group_now = (unsigned long long)fv.listed * 2ull > (unsigned long long)c->ns;
    pol.on = fv.iterations == 1u && pol.cold_admits(fv, fo, c->ns, c->warm_forecast, f.group_now);
  }
  if (it >= 2) {
    // wait (briefly, if at all) until iteration it - 2 has been published
    FbView fv;
    int rc = wait_published_or_sync(c, (unsigned int)(it - 1), &fv);
    if (rc) return rc;
    if (fv.done) return CILHIP_OK;
    const int fo = form_of(c->trace_form, fv.iterations);
    if (f.fwcap && !pol.warm_banned) {
      // (a warm-started feature search reports the queries it had to search in full: more than a quarter of them = a cold tile search's price)
      if (form_is(fo, FORM_WARM) && fv.iterations > f.feat_judged) { f.feat_judged = fv.iterations; if (!pol.warm_keeps_paying(fv.listed, c->ns)) f.feat_warm_now = false; }
      else if (!f.feat_warm_now) f.feat_warm_now = pol.warm_worthwhile(fv.step);
    }
    pol.note_unproven(fo, fv.unproven, c->ns);
    // a cold iteration that counted: its forecast decides (every eighth iteration of a stretch of cooperative searches is such a
    // one: enqueue_forward_iteration)
    if (auto_lanes && f.wcap && form_counted(fo)) f.group_now = (unsigned long long)fv.listed * 2ull > (unsigned long long)c->ns;
    const bool fell = warm_auto && pol.judge(fv, fo, c->ns);
    if (warm_auto && pol.candidate(fell, fv.step)) {
      // Candidate for the warm-started form.  Decided on the step the loop made LAST -- it is the distance between
      // the queries the margins were left for and the queries about to be searched -- so wait for iteration it - 1 itself
      // (a bubble of some tens of microseconds, only while this decision is pending and the loop is within reach of it).
      rc = wait_published_or_sync(c, (unsigned int)it, &fv);
      if (rc) return rc;
      if (fv.done) return CILHIP_OK;
      // (never out of a stretch of cooperative searches: they leave no keys; its next one-lane iteration's forecast ends the stretch first)
      pol.decide(fv, form_of(c->trace_form, fv.iterations), c->ns, c->warm_forecast, auto_lanes && f.group_now);
    }
  }
  *stop = false;
  return CILHIP_OK;
}

// Enqueues iteration `it` in the form decided for it (timing_it: it carries events): search / accumulation, then per Gauss-Newton step reduction + epilogue.
static int enqueue_forward_iteration(cilhip_ctx* c, RunSetup& r, ForwardRun& f, size_t it, bool one_pass, bool warm, bool timing_it) {
  IterArgs& a = r.a;
  SolveArgs& sa = r.sa;
  const int im = r.im, nb = r.nb;
  const size_t opt_steps = r.opt_steps;
  const bool single = one_pass || warm;        // search + accumulation in one kernel
  const bool fused = lane_fused(c);
  bool warm_first = false;
  bool stored_now = true;    // this iteration leaves its matches in nn_pos
  bool counted = false;      // a cold iteration whose kernels count the queries a warm-started iteration after it would have to search
  bool feat_warm_it = false; // this iteration's feature search ran warm-started
  bool feat_fused_it = false; // ... and accumulated the first step's sums itself
  for (size_t st = 0; st < opt_steps; ++st) {
    a.skip_if_inner_done = (st > 0);
    // (the one-kernel forms are timed through their own dispatch packets: no event packets between dependent kernels)
    const bool ext_ev = timing_it && st == 0 && c->ns && !fused && (warm || one_pass);
    if (timing_it && st == 0 && !ext_ev) CK(c, hipEventRecord(event_at(c->ev, f.nev++), c->stream));
    if (ext_ev) { hipEvent_t e0 = event_at(c->ev, f.nev), e1 = event_at(c->ev, f.nev + 1); set_launch_events(e0, e1); f.nev += 2; }
    if (c->ns) {
      if (st == 0 && fused) {
        launch_iter(a, im, true, r.gn && opt_steps > 1, nb, c->stream);
        stored_now = r.gn && opt_steps > 1;
        f.all_stored = f.all_stored && stored_now;
      } else if (st == 0 && warm) {
        warm_first = launch_warm_iteration(c, a, im);
      } else if (st == 0 && one_pass) {
        // (the matches are only stored when further Gauss-Newton steps will stream over them or the next iteration may start from
        //  them; from the second iteration on the tile leaves the match records of the warm-started form -- not the first: a
        //  registration's first step is its largest, its margins would be spent at once)
        stored_now = opt_steps > 1 || c->warm_start;
        counted = launch_tile_one_pass(c, a, im, stored_now, f.wcap && it >= 1);
        f.all_stored = f.all_stored && stored_now;
      } else if (st == 0) {
        c->rec_valid = false;
        // (search-only form of the tiles: the margin keys of its searches next to the matches)
        IterArgs sa2 = a;
        // (above the warm-started form's floor a stretch of cooperative searches is interrupted by a one-lane search now and then -- after
        //  8 iterations, then 16, 32 ...: it leaves the margin keys and the forecast the loop's decisions, this form or that, the
        //  warm-started one, are taken from)
        const bool probe = c->group_lanes < 0 && f.wcap && it >= f.next_probe;
        if (probe) { f.next_probe = it + f.probe_gap; f.probe_gap *= 2; }
        const int lanes_it = (f.group_now && !probe && !use_tiled(c) && !feat6(c)) ? f.glanes : 0;
        const bool keys = f.wcap && !feat6(c) && !lanes_it;
        if (keys) sa2.nn_lb = c->d_nn_lb;
        c->lb_fresh = keys;
        counted = keys;
        // (the cooperative form: the previous iteration's matches, when it left them in nn_pos, bound every query's search)
        if (lanes_it && it >= 1 && f.prev_stored) sa2.warm_pos = c->d_nn_pos;
        feat_warm_it = f.fwcap && f.feat_warm_now && it >= 1 && f.prev_stored && !c->policy.warm_banned;
        // (... with the sums in the same pass when the terms are the three-cloud metric's own: no source normals in the objective, no per-pair weights)
        feat_fused_it = feat_warm_it && !(c->d_src_nrm && c->symmetric) && !a.cw.enabled;
        if (feat_warm_it) { sa2.safe2 = c->d_safe2; sa2.partials = c->d_partials; launch_feat_warm(sa2, feat_fused_it ? im : (int)IM_NONE, c->stream); ++c->last_warm_iters; }
        else { const int src_rc = launch_search(c, sa2, lanes_it); if (src_rc) return src_rc; }
        { const int frc = apply_filters(c); if (frc) return frc; }
        if (timing_it) { CK(c, hipEventRecord(event_at(c->ev, f.nev++), c->stream)); CK(c, hipEventRecord(event_at(c->ev_acc, f.nacc++), c->stream)); }
        if (r.affine) launch_acc_affine(a, im, r.nb_aff, c->stream);            // streaming accumulation kernel
        else if (!feat_fused_it) launch_iter(a, im, false, false, nb, c->stream);
      } else {
        launch_iter(a, im, false, false, nb, c->stream);
      }
    }
    if (timing_it && st == 0) {
      // (two events per iteration around the search / one-pass kernels; a two-pass iteration adds a pair around its
      //  streaming accumulation, kept in a list of its own)
      if (ext_ev) {}
      else if (single || fused || !c->ns) CK(c, hipEventRecord(event_at(c->ev, f.nev++), c->stream));
      else CK(c, hipEventRecord(event_at(c->ev_acc, f.nacc++), c->stream));
      c->timed_iter.push_back((unsigned int)it);
    }
    if (st == 0) {
      if (single) ++c->last_fused_iters; else ++c->last_two_pass_iters;
      if (warm) ++c->last_warm_iters;
      const int fm = warm ? (warm_first ? FORM_WARM_FIRST : FORM_WARM) : feat_warm_it ? FORM_WARM : one_pass ? FORM_TILE_ONE_PASS : fused ? FORM_LANE_FUSED : FORM_SEARCH;
      if (timing_it) c->iter_form.push_back((unsigned char)fm);
      c->trace_form.push_back(trace_byte(fm, counted));
    }
    sa.gn_last_step = (st + 1 == opt_steps);
    if (c->ns) {
      const int prows = (st == 0 && warm) ? warm_num_blocks(c->ns) : (st == 0 && one_pass) ? tiled_partial_rows(c->ntiles) : (st == 0 && feat_fused_it) ? feat_warm_blocks(c->ns)
                        : r.affine ? r.nb_aff : nb;
      if (r.affine) launch_reduce_and_solve_affine(c->d_partials, prows, c->d_stage, sa, c->stream);
      else launch_reduce_and_solve(c->d_partials, prows, c->d_stage, c->fused_epilogue ? c->d_ticket : nullptr, sa, c->stream);
    } else {
      launch_solve(sa, c->stream);
    }
  }
  f.prev_stored = stored_now && c->ns != 0;
  return CILHIP_OK;
}

// kernel timing on: the events of the iterations that actually executed (not the early-exit launches after convergence)
static int collect_kernel_timing(cilhip_ctx* c, const ForwardRun& f, size_t iterations) {
  size_t executed = 0;
  while (executed < c->timed_iter.size() && (size_t)c->timed_iter[executed] < iterations) ++executed;
  c->last_acc_ms = 0.0;
  c->timed_ms.assign(executed, 0.0f);
  for (size_t k = 0; k < executed; ++k) {
    float m = 0.f;
    CK(c, hipEventElapsedTime(&m, c->ev[2 + 2 * k], c->ev[3 + 2 * k]));
    c->timed_ms[k] = m;
    c->last_search_ms += m;
    if (k < c->iter_form.size()) { c->form_ms[c->iter_form[k]] += m; ++c->form_n[c->iter_form[k]]; }
  }
  for (size_t k = 0; k + 1 < f.nacc; k += 2) {      // (two-pass iterations; those enqueued past convergence measure ~0)
    float m = 0.f;
    CK(c, hipEventElapsedTime(&m, c->ev_acc[k], c->ev_acc[k + 1]));
    c->last_acc_ms += m;
  }
  c->last_search_launches = (int)executed;
  return CILHIP_OK;
}

static int run_forward_loop(cilhip_ctx* c, RunSetup& r) {
  const cilhip_icp_params* p = r.p;
  IterArgs& a = r.a;
  int rc;
  if (feat6(c)) { rc = ensure_feature_arrays(c); if (rc) return rc; a.feat = feat_spec_of(c); }
  if (!filters_active(c) && !(a.cw.enabled && feat6(c))) a.nn_d2 = nullptr;   // nobody reads the distances inside the loop: 4 B per query less to write
                                                                              // (a weight evaluator over the 6-D feature distance does)
  ForwardRun f{};
  f.tile_acc = tile_accumulation(c) && !r.affine;      // (the tiles accumulate the rigid classes' terms only)
  f.timing = c->kernel_timing && p->max_iter <= 4096;
  CK(c, hipEventRecord(r.e_beg, c->stream));
  f.wcap = warm_capable(c);
  if (f.wcap) { rc = ensure_safe2(c); if (rc) return rc; rc = ensure_warm_buffers(c); if (rc) return rc; }
  // the feature adaptors' searches warm-started from the previous matches (feat_warm.hip): once the published step is within reach,
  // while the kernel's own count of the queries it had to search says that it pays
  // (from 400 000 source points up: below, the look at the published state before every enqueue costs what the form saves -- measured 200k: +5 %, 1M: -23 %)
  f.fwcap = feat6(c) && c->feat_warm && c->warm_start != 0 && c->ns >= 400000 && !filters_active(c) && !c->fused && !r.affine;
  if (f.fwcap) {
    rc = ensure_safe2(c); if (rc) return rc;
    rc = grow_partials(c, r, (size_t)feat_warm_blocks(c->ns)); if (rc) return rc;
  }
  f.paced = ((f.tile_acc || f.wcap) && c->ns && p->max_iter > 2 && c->tile_acc_adaptive) || (f.fwcap && p->max_iter > 2);
  if (f.tile_acc && !c->tile_acc_adaptive) c->policy.far_mode = false;
  c->last_fused_iters = c->last_two_pass_iters = c->last_warm_iters = c->last_rev_fused_iters = 0;
  c->rec_valid = false; c->lb_fresh = false;
  c->policy.begin_run(c->warm_enter * c->grid.cell);
  c->iter_form.clear(); c->trace_form.clear(); c->timed_iter.clear();
  for (int k = 0; k < 5; ++k) { c->form_ms[k] = 0.0; c->form_n[k] = 0; }
  // The cooperative search (several lanes per query) for the cold iterations of clouds the tiles do not take: lanes so that the
  // queries fill the machine; below the warm-started form's floor always (nothing is lost: no margin keys are wanted there), above it
  // while the cold kernels' forecast says that most queries are far from settled (their margins would not survive the next step) and
  // the loop is not yet within reach of the warm-started form -- whose entry needs the keys only the one-lane search leaves.
  f.glanes = c->group_lanes > 0 ? c->group_lanes
             : (c->group_lanes < 0 && !use_tiled(c) && !feat6(c) && !c->fused) ? (c->ns <= 400000u ? 16 : c->ns <= 1500000u ? 8 : 0) : 0;
  f.group_now = f.glanes != 0 && (c->group_lanes > 0 || !f.wcap);
  for (size_t it = 0; it < p->max_iter; ++it) {
    bool stop = false;
    if (f.paced) { rc = pace_forward(c, f, it, &stop); if (rc) return rc; if (stop) break; }
    const bool one_pass = f.tile_acc && !c->policy.far_mode;
    // Third form, from the second iteration on: search + accumulation WARM-STARTED from the previous iteration's matches and
    // the margins their searches left (kept by the forms above) -- no tile to stage at all.  Same matches, same sums up to
    // the order of the f64 additions.
    const bool warm = f.wcap && it >= 1 && (c->warm_start == 2 || (f.paced && c->policy.on));
    // (kernel timing on: does THIS iteration carry events?  Every event between dependent kernels idles the device for ~6 us --
    //  two per iteration are a tenth of a warm-started iteration at 10M -- so a caller may ask for a sample: option kernel_timing_stride)
    const bool timing_it = f.timing && (c->timing_stride <= 1 || it < 3 || it % (size_t)c->timing_stride == 0);
    rc = enqueue_forward_iteration(c, r, f, it, one_pass, warm, timing_it);
    if (rc) return rc;
    if (!f.paced) { rc = stop_when_done(c, it, p->max_iter, &stop); if (rc) return rc; if (stop) break; }
  }
  rc = finish_run(c, r, f.all_stored && !filters_active(c) && !feat6(c), false);
  if (rc) return rc;
#ifdef CILHIP_EXP_PHASE_CLOCKS
  cilhip::debug_dump_phase_clocks();
#endif
  return f.timing ? collect_kernel_timing(c, f, r.out->iterations) : CILHIP_OK;
}

static int icp_run_once(cilhip_ctx* c, const cilhip_icp_params* p, const float* T0, cilhip_icp_result* out) {
  if (c->proj_on) {
    if (const char* why = proj_conflict(c)) return fail(c, CILHIP_ERR_UNSUPPORTED, why);
    if (c->transform_mode == 1) return fail(c, CILHIP_ERR_UNSUPPORTED, "projective search: the affine loop is not available");
  }
  if (c->weight_fn && p->metric == CILHIP_METRIC_COMBINED && c->transform_mode == 0) {
    // a caller's own weight evaluators run on the host: the reference's loop step by step (search, estimate over the stored set with
    // the callback's weights, rotation() polish + compose), the combiner's loop with one engine in both roles
    if (c->search_dir != 0) return fail(c, CILHIP_ERR_UNSUPPORTED, "a pair-weight callback runs with SECOND_TO_FIRST searches (rigid loop); estimate from pair lists through cilhip_estimate_combined");
    c->last_loop_ms = 0.0; c->last_search_ms = 0.0; c->last_acc_ms = 0.0; c->last_search_launches = 0;
    return cilhip_icp_run_two_sets(c, p->max_sq_dist, c, p->max_sq_dist, p, T0, out);
  }
  // The affine classes: their loop runs device-resident like the rigid one -- search-only kernels + one streaming pass of moments
  // (k_acc_affine) while the source is far from alignment, search + moments in the warm-started kernel afterwards, the 12-unknown solve
  // and the f32 compose in k_solve_affine -- unless something asks for the stored set per iteration (post-filters, per-pair weights,
  // other directions, feature adaptors): those keep the host-driven loop (icp_run_affine: three passes + a host solve per iteration).
  RunSetup r{};
  r.p = p; r.out = out;
  r.affine = c->transform_mode == 1;
  if (r.affine) {
    if (c->index_offset) return fail(c, CILHIP_ERR_UNSUPPORTED, "the affine variants are not available on target shards");
    const bool device_loop = c->affine_device_loop && c->ns != 0 && c->grid.n != 0 && c->search_dir == 0 && !filters_active(c) && !weighted(c) && !feat6(c) && !c->fused &&
                             !(c->d_src_nrm && c->symmetric) && c->guard_axis < 0;
    if (!device_loop) return icp_run_affine(c, p, T0, out);
  }
  r.Ti = T0 ? T0 : kIdentity16;
  int rc = ensure_sorted(c, r.Ti);
  if (rc) return rc;
  const bool affine_combined = r.affine && p->metric == CILHIP_METRIC_COMBINED;
  r.im = !r.affine ? iter_metric_of(c, p) : (affine_combined && p->w_p2pl > 0.0f && c->has_normals) ? IM_AFFC : IM_AFFP;
  r.gn = (r.im != IM_KABSCH) && !r.affine;
  // max_optimization_iterations == 0 (combined metric): the estimator's loop body never runs -- one accumulation pass still counts
  // the correspondences (the "no usable terms" test, transform_estimation.hpp:264-272), the epilogue skips the solve
  const bool zero_steps = r.gn && p->max_opt_iter == 0;
  r.opt_steps = r.gn ? (p->max_opt_iter ? p->max_opt_iter : 1) : 1;
  ++c->run_tag;
  launch_init_state(c->d_state, r.Ti, c->src_mean, c->stream, c->d_feedback, c->run_tag, c->src_center, c->src_half, c->d_tie_counters);
  if (r.gn && c->ns >= 65536) ensure_pair_records(c);
  r.a = make_iter_args(c, p->max_sq_dist);
  if (!c->pair_records) r.a.grid.pn = nullptr;
  r.a.cw = corr_weights_of(c, p);
  r.sa = make_solve_args(c, p, r.im, c->src_mean);
  r.sa.gn_zero_steps = zero_steps ? 1 : 0;
  r.nb = r.sa.nblocks;
  r.nb_aff = r.affine ? affine_acc_blocks(c->ns) : 0;
  if (r.affine) {
    r.a.no_centering = affine_combined ? 0 : 1;
    r.sa.affine_centered = affine_combined ? 1 : 0;
    if (!affine_combined) { r.sa.w_p2p = 1.0f; r.sa.w_p2pl = 0.0f; }      // the point-to-point class: unit point terms of the raw coordinates
    // rows of AFF_ROW doubles: the streaming pass's or the warm-started kernel's
    const size_t rows = (size_t)std::max(r.nb_aff, warm_num_blocks(c->ns));
    rc = grow_partials(c, r, (rows * AFF_ROW + SUMS_MAX - 1) / SUMS_MAX);
    if (rc) return rc;
  }
  if (c->ns == 0) {  // no source points: the epilogue runs on all-zero sums (identity step)
    CK(c, hipMemsetAsync(c->d_sums, 0, SUMS_MAX * sizeof(double), c->stream));
    r.sa.nblocks = 0;
    r.sa.reduced = c->d_sums;
  }
  r.e_beg = event_at(c->ev, 0); r.e_end = event_at(c->ev, 1);
  if (c->proj_on) return run_projective_loop(c, r);
  return c->search_dir != 0 ? run_other_directions(c, r) : run_forward_loop(c, r);
}

int cilhip_icp_run(cilhip_ctx* c, const cilhip_icp_params* p, const float* T0, cilhip_icp_result* out) {
  if (!c || !p || !out) return CILHIP_ERR_INVALID;
  if (p->metric != CILHIP_METRIC_POINT_TO_POINT && p->metric != CILHIP_METRIC_COMBINED) return fail(c, CILHIP_ERR_INVALID, "icp_run: bad metric");
  CK(c, hipSetDevice(c->device));
  int rc = tie_prepare(c, "icp_run");
  if (rc) return rc;
  rc = icp_run_once(c, p, T0, out);
  if (rc) return rc;
  // tie_rule 2: some search of the run met exactly equidistant nearest points and the reference's order tables were not there: they
  // are now (built once per target) -- the run is executed again, from T0, with the ties resolved inside its kernels
  bool again = false;
  rc = tie_check_pending(c, &again);
  if (rc) return rc;
  return again ? icp_run_once(c, p, T0, out) : CILHIP_OK;
}

int cilhip_icp_begin(cilhip_ctx* c, const cilhip_icp_params* p, const float* T0, const float* gmean) {
  if (!c || !p) return CILHIP_ERR_INVALID;
  if (c->proj_on) return fail(c, CILHIP_ERR_UNSUPPORTED, "projective search: sharded runs (cilhip_icp_begin ..., cilhip_multi_*) are not available");
  CK(c, hipSetDevice(c->device));
  if (p->metric == CILHIP_METRIC_COMBINED && p->max_opt_iter != 1) return fail(c, CILHIP_ERR_UNSUPPORTED, "sharded runs support max_opt_iter == 1");
  if (filters_active(c)) return fail(c, CILHIP_ERR_UNSUPPORTED, "inlier_fraction / one_to_one are global filters: not available in sharded runs");
  if (c->weight_fn && p->metric == CILHIP_METRIC_COMBINED)
    return fail(c, CILHIP_ERR_UNSUPPORTED, "a pair-weight callback is evaluated on the host, per estimate: not available in sharded runs (the stock evaluators are)");
  { const int trc = tie_prepare(c, "icp_begin"); if (trc) return trc; }
  if (c->search_dir != 0) return fail(c, CILHIP_ERR_UNSUPPORTED, "search directions other than SECOND_TO_FIRST are not available in sharded runs");
  if (feat6(c) || c->transform_mode != 0) return fail(c, CILHIP_ERR_UNSUPPORTED, "point+normal features and the affine variants are not available in sharded runs");
  const float* Ti = T0 ? T0 : kIdentity16;
  int rc = ensure_sorted(c, Ti);
  if (rc) return rc;
  c->run_prm = *p;
  for (int i = 0; i < 3; ++i) c->run_src_mean[i] = gmean ? gmean[i] : c->src_mean[i];
  ++c->run_tag;
  launch_init_state(c->d_state, Ti, c->run_src_mean, c->stream, c->d_feedback, c->run_tag, c->src_center, c->src_half, c->d_tie_counters);     // (the epilogue publishes the loop state: see cilhip_icp_partial_sums)
  CK(c, hipGetLastError());
  c->run_active = true;
  c->run_nev = 0; c->run_nar = 0; c->last_allreduce_ms = 0.0; c->last_allreduce_n = 0;
  c->run_enqueue_us = 0.0; c->run_enqueue_iters = 0;
  c->run_calls = 0;
  c->rec_valid = false; c->lb_fresh = false;
  c->policy.begin_run(c->warm_enter * c->grid.cell);
  if (warm_capable(c) && !(c->d_src_nrm && c->symmetric)) { rc = ensure_safe2(c); if (rc) return rc; rc = ensure_warm_buffers(c); if (rc) return rc; }
  c->iter_form.clear(); c->trace_form.clear();
  for (int k = 0; k < 5; ++k) { c->form_ms[k] = 0.0; c->form_n[k] = 0; }
  c->last_fused_iters = c->last_two_pass_iters = c->last_warm_iters = c->last_rev_fused_iters = 0;    // counted per cilhip_icp_partial_sums call (cilhip_get_last_run_forms)
  return CILHIP_OK;
}

// Sharded runs: does this call's iteration run warm-started (see cilhip_icp_run)?  From the second call on, when the latest loop
// state this run's epilogues have published (a bounded wait for iteration run_calls - 2) says the source is near alignment.
// Ranks may differ in their choice: the sums are the same up to the order of the f64 additions.
static bool sharded_warm_now(cilhip_ctx* c) {
  if (c->warm_start == 2) return true;
  if (c->run_calls < 2) return false;
  // paced like cilhip_icp_run: at most two iterations ahead of the device (which never waits: an iteration takes
  // hundreds of microseconds), so that the loop state looked at is at least that of iteration run_calls - 2; a brief
  // wait at most (5 s without news: the cold form)
  LoopPolicy& pol = c->policy;
  FbView fv;
  if (wait_published(c, (unsigned int)(c->run_calls - 1), 5.0, &fv) != 0) return false;
  // (what a published iteration's counts mean depends on the form it ran in: loop_policy.hpp)
  const int fo = form_of(c->trace_form, fv.iterations);
  pol.note_unproven(fo, fv.unproven, c->ns);
  const bool fell = pol.judge(fv, fo, c->ns);
  // candidate for the warm-started form: decided on the step the loop made LAST -- wait for iteration run_calls - 1
  // itself (its epilogue has been enqueued by the caller's previous apply; a bubble of some tens of microseconds, only
  // while this decision is pending and the loop is within reach of it)
  if (pol.candidate(fell, fv.step) && wait_published(c, (unsigned int)c->run_calls, 5.0, &fv) == 0)
    pol.decide(fv, form_of(c->trace_form, fv.iterations), c->ns, c->warm_forecast, false);
  return pol.on;
}

// sums_dev != null: the 48 sums of this iteration's search + accumulation (cilhip_icp_partial_sums).  rows_dev != null instead: RANK_ROWS
// rows that still have to be folded -- the stage-1 reduction with a FIXED number of groups, whatever form the iteration took and
// however many blocks this rank has -- for the ranked loop, which all-reduces those (12 KB instead of 384 B: both latency-bound) and
// lets the epilogue fold them as it does in cilhip_icp_run: one kernel and one gap less per iteration.
constexpr int RANK_ROWS = 32;
static int partial_sums_core(cilhip_ctx* c, double* sums_dev, double* rows_dev) {
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  const int im = iter_metric_of(c, &c->run_prm);
  IterArgs a = make_iter_args(c, c->run_prm.max_sq_dist);
  a.cw = corr_weights_of(c, &c->run_prm);
  const int nb = iter_num_blocks(c->ns);
  int prows = nb;
  int form_now = FORM_LANE_FUSED;      // (the form this iteration takes: what its published counts will mean)
  bool counted = false;
  if (c->ns && c->grid.n) {      // (a shard without target points -- a slab beyond the target's extent -- has nothing to match: zero sums)
    if (c->fused) {
      launch_iter(a, im, true, false, nb, c->stream);
    } else {
      a.nn_d2 = nullptr;   // no post-filters in sharded runs: nobody reads the squared distances (as in cilhip_icp_run)
      const bool timing = c->kernel_timing && c->run_nev + 3 <= 3 * 4096 &&
                          (c->timing_stride <= 1 || c->run_calls < 3 || c->run_calls % c->timing_stride == 0);      // (a sample of the iterations: option kernel_timing_stride)
      const size_t e = 2 + c->run_nev;
      if (timing) CK(c, hipEventRecord(event_at(c->ev, e), c->stream));
      const bool wcap = warm_capable(c) && !(c->d_src_nrm && c->symmetric);      // (the sharded building blocks: the symmetric objective stays with the streaming pass)
      const bool warm = wcap && c->run_calls >= 1 && sharded_warm_now(c);
      if (warm) {
        form_now = launch_warm_iteration(c, a, im) ? FORM_WARM_FIRST : FORM_WARM;
        prows = warm_num_blocks(c->ns);
        ++c->last_fused_iters; ++c->last_warm_iters;
      } else if (tile_accumulation(c)) {
        form_now = FORM_TILE_ONE_PASS;
        counted = launch_tile_one_pass(c, a, im, c->warm_start != 0, wcap && c->run_calls >= 1);
        prows = tiled_partial_rows(c->ntiles);
        ++c->last_fused_iters;
      } else {
        c->rec_valid = false;
        ++c->last_two_pass_iters;
        IterArgs sa2 = a;
        const bool keys = wcap;
        if (keys) sa2.nn_lb = c->d_nn_lb;
        c->lb_fresh = keys;
        form_now = FORM_SEARCH; counted = keys;
        if (use_tiled(c)) launch_search_tiled(sa2, IM_NONE, c->d_tiles, c->d_tile_center, c->d_tile_box, c->ntiles, c->stream);
        else launch_iter(sa2, IM_NONE, true, true, nb, c->stream);
      }
      if (timing) {
        c->iter_form.push_back((unsigned char)form_now);
        CK(c, hipEventRecord(event_at(c->ev, e + 1), c->stream));
      }
      if (form_now == FORM_SEARCH) launch_iter(a, im, false, false, nb, c->stream);      // the streaming accumulation of the two-pass form
      if (timing) { CK(c, hipEventRecord(event_at(c->ev, e + 2), c->stream)); c->run_nev += 3; }
    }
    if (sums_dev) launch_reduce_partials(c->d_partials, prows, c->d_stage, sums_dev, c->stream);
    else launch_reduce_stage1_groups(c->d_partials, prows, rows_dev, RANK_ROWS, c->stream);
  } else if (sums_dev) {
    CK(c, hipMemsetAsync(sums_dev, 0, SUMS_MAX * sizeof(double), c->stream));
  } else {
    CK(c, hipMemsetAsync(rows_dev, 0, (size_t)RANK_ROWS * SUMS_MAX * sizeof(double), c->stream));
  }
  c->trace_form.push_back(trace_byte(form_now, counted));
  ++c->run_calls;
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

int cilhip_icp_partial_sums(cilhip_ctx* c, double* sums_dev) {
  if (!c || !sums_dev) return CILHIP_ERR_INVALID;
  return partial_sums_core(c, sums_dev, nullptr);
}

int cilhip_icp_apply_sums(cilhip_ctx* c, const double* sums_dev) {
  if (!c || !sums_dev) return CILHIP_ERR_INVALID;
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  const int im = iter_metric_of(c, &c->run_prm);
  SolveArgs sa = make_solve_args(c, &c->run_prm, im, c->run_src_mean);
  sa.nblocks = 0;
  sa.reduced = sums_dev;
  launch_solve(sa, c->stream);
  CK(c, hipGetLastError());
  return CILHIP_OK;
}

int cilhip_icp_state(cilhip_ctx* c, cilhip_icp_result* out) {
  if (!c || !out) return CILHIP_ERR_INVALID;
  CK(c, hipSetDevice(c->device));
  const int rc = read_state(c, out);   // (synchronises the stream)
  if (rc == CILHIP_OK && c->run_nar) {
    double ms = 0.0;
    for (size_t k = 0; k + 2 <= c->run_nar; k += 2) { float a = 0.f; CK(c, hipEventElapsedTime(&a, c->ev_ar[k], c->ev_ar[k + 1])); ms += a; }
    c->last_allreduce_ms = ms; c->last_allreduce_n = (int)(c->run_nar / 2);
    c->run_nar = 0;
  }
  if (rc == CILHIP_OK && c->run_nev) {
    // kernel timing of a sharded run: search / accumulation time summed over the cilhip_icp_partial_sums calls since
    // cilhip_icp_begin (read with cilhip_get_last_timing / cilhip_get_last_timing2)
    double sm = 0.0, am = 0.0;
    for (size_t k = 0; k + 3 <= c->run_nev; k += 3) {
      float a = 0.f, b = 0.f;
      CK(c, hipEventElapsedTime(&a, event_at(c->ev, 2 + k), event_at(c->ev, 2 + k + 1)));
      CK(c, hipEventElapsedTime(&b, event_at(c->ev, 2 + k + 1), event_at(c->ev, 2 + k + 2)));
      sm += a; am += b;
      if (k / 3 < c->iter_form.size()) { c->form_ms[c->iter_form[k / 3]] += a; ++c->form_n[c->iter_form[k / 3]]; }
    }
    c->last_search_ms = sm; c->last_acc_ms = am; c->last_search_launches = (int)(c->run_nev / 3);
    c->last_loop_ms = 0.0;
    c->run_nev = 0;
  }
  return rc;
}

// =====================================================================================================================
// One process PER device (torchrun, MPI): this process' context as one rank of an RCCL communicator, and the sharded loop's
// inner triple -- partial sums, all-reduce of the 48 f64, epilogue -- run for a number of iterations inside ONE call: per
// iteration the host enqueues a handful of launches and one ncclAllReduce on the context's stream instead of going through three
// foreign-function calls and a framework collective (measured with one rank: 0.169 -> see DESIGN.md section 8).  The id travels
// by whatever the launcher already has (torch.distributed broadcast, MPI_Bcast, a file).
namespace { RcclApi g_rank_rccl; }

int cilhip_rank_comm_unique_id(unsigned char id_out[128]) {
  if (!id_out) return CILHIP_ERR_INVALID;
  if (!g_rank_rccl.load()) return CILHIP_ERR_UNSUPPORTED;
  RcclApi::UniqueId u;
  if (g_rank_rccl.GetUniqueId(&u) != 0) return CILHIP_ERR_HIP;
  memcpy(id_out, u.internal, sizeof(u.internal));
  return CILHIP_OK;
}

// Everything of cilhip_rank_comm_init that can fail on ONE rank alone -- opening librccl, the buffer of the rows -- done beforehand, so
// that the ranks can agree (one MIN over whatever channel the launcher has) to enter the collective ncclCommInitRank only when every
// one of them will get through: a rank that bailed out before the collective would leave its peers waiting inside it.
int cilhip_rank_comm_prepare(cilhip_ctx* c) {
  if (!c) return CILHIP_ERR_INVALID;
  if (!g_rank_rccl.load()) return fail(c, CILHIP_ERR_UNSUPPORTED, "rank_comm_prepare: librccl.so.1 could not be opened");
  CK(c, hipSetDevice(c->device));
  if (!c->d_rank_sums && c->d_rank_sums.alloc((size_t)RANK_ROWS * SUMS_MAX) != hipSuccess)
    return fail(c, CILHIP_ERR_HIP, "rank_comm_prepare: out of device memory");
  return CILHIP_OK;
}

int cilhip_rank_comm_init(cilhip_ctx* c, const unsigned char id[128], int nranks, int rank) {
  if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return CILHIP_ERR_INVALID;
  if (c->rank_comm) return fail(c, CILHIP_ERR_INVALID, "rank_comm_init: the context already holds a communicator");
  if (!g_rank_rccl.load()) return fail(c, CILHIP_ERR_UNSUPPORTED, "rank_comm_init: librccl.so.1 could not be opened");
  CK(c, hipSetDevice(c->device));
  RcclApi::UniqueId u;
  memcpy(u.internal, id, sizeof(u.internal));
  rccl_comm_t comm = nullptr;
  if (g_rank_rccl.CommInitRank(&comm, nranks, u, rank) != 0 || !comm) return fail(c, CILHIP_ERR_HIP, "ncclCommInitRank failed");
  if (!c->d_rank_sums && c->d_rank_sums.alloc((size_t)RANK_ROWS * SUMS_MAX) != hipSuccess) {
    (void)g_rank_rccl.CommDestroy(comm);
    return fail(c, CILHIP_ERR_HIP, "rank_comm_init: out of device memory");
  }
  c->rank_comm = comm; c->rank_comm_size = nranks;
  return CILHIP_OK;
}

int cilhip_rank_comm_destroy(cilhip_ctx* c) {
  if (!c) return CILHIP_ERR_INVALID;
  if (c->rank_comm) { (void)hipStreamSynchronize(c->stream); (void)g_rank_rccl.CommDestroy(c->rank_comm); c->rank_comm = nullptr; c->rank_comm_size = 0; }
  c->d_rank_sums.reset();
  return CILHIP_OK;
}

int cilhip_get_last_allreduce_timing(cilhip_ctx* c, double* total_ms, int* timed) {
  if (!c) return CILHIP_ERR_INVALID;
  if (total_ms) *total_ms = c->last_allreduce_ms;
  if (timed) *timed = c->last_allreduce_n;
  return CILHIP_OK;
}

int cilhip_get_last_host_enqueue_time(cilhip_ctx* c, double* us_per_iteration) {
  if (!c || !us_per_iteration) return CILHIP_ERR_INVALID;
  *us_per_iteration = c->run_enqueue_iters ? c->run_enqueue_us / c->run_enqueue_iters : 0.0;
  return CILHIP_OK;
}

int cilhip_icp_iterate_ranked(cilhip_ctx* c, int iterations) {
  if (!c || iterations < 0) return CILHIP_ERR_INVALID;
  if (!c->rank_comm) return fail(c, CILHIP_ERR_INVALID, "icp_iterate_ranked: cilhip_rank_comm_init first");
  if (!c->run_active) return fail(c, CILHIP_ERR_INVALID, "icp_begin first");
  CK(c, hipSetDevice(c->device));
  const int im = iter_metric_of(c, &c->run_prm);
  const auto t_call = std::chrono::steady_clock::now();
  const double wait0 = c->wait_us;
  struct Acc { cilhip_ctx* c; std::chrono::steady_clock::time_point t; double w0; int n;
               ~Acc() { c->run_enqueue_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t).count() - (c->wait_us - w0); c->run_enqueue_iters += n; } } acc{c, t_call, wait0, iterations};
  for (int k = 0; k < iterations; ++k) {
    // this rank's RANK_ROWS rows of partial sums -> summed over the ranks, row by row -> folded by the epilogue (the same values on
    // every rank: identical transforms and decisions everywhere)
    // (with kernel timing on, the iterations that carry kernel events also time their collective: what the all-reduce costs per
    //  iteration ON THE STREAM -- launch of RCCL's kernel, the exchange over xGMI, the wait for the slowest rank -- is the figure a
    //  scaling curve has to be read against; cilhip_get_last_allreduce_timing)
    const bool time_ar = c->kernel_timing && c->run_nar + 2 <= 2 * 4096 &&
                         (c->timing_stride <= 1 || c->run_calls < 3 || c->run_calls % c->timing_stride == 0);
    const int rc = partial_sums_core(c, nullptr, c->d_rank_sums);
    if (rc) return rc;
    if (time_ar) {
      while (c->ev_ar.size() < c->run_nar + 2) { hipEvent_t e; CK(c, hipEventCreate(&e)); c->ev_ar.push_back(e); }
      CK(c, hipEventRecord(c->ev_ar[c->run_nar], c->stream));
    }
    if (g_rank_rccl.AllReduce(c->d_rank_sums, c->d_rank_sums, (size_t)RANK_ROWS * SUMS_MAX, RCCL_DOUBLE, RCCL_SUM, c->rank_comm, c->stream) != 0)
      return fail(c, CILHIP_ERR_HIP, "ncclAllReduce failed");
    if (time_ar) { CK(c, hipEventRecord(c->ev_ar[c->run_nar + 1], c->stream)); c->run_nar += 2; }
    SolveArgs sa = make_solve_args(c, &c->run_prm, im, c->run_src_mean);
    sa.partials = c->d_rank_sums; sa.nblocks = RANK_ROWS; sa.reduced = nullptr;
    launch_solve(sa, c->stream);
    CK(c, hipGetLastError());
  }
  return CILHIP_OK;
}

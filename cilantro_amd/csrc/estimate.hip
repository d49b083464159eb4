// estimate.hip -- the transform estimates over a stored correspondence set (the bit-pinned host paths of the reference's estimators): pair
// weights, the accumulation passes, cilhip_estimate_*, the host-driven two-set and affine loops, cilhip_compute_residuals.
#include <cmath>
#include <cstring>
#include <new>

#include "ctx.hpp"

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

// The stored set as the accumulating kernels read it when it is a pair list (FIRST_TO_SECOND / BOTH): a pair list carries its own view of
// the source, per pair -- points, values and, for the symmetric objective, normals.
void cilhip::use_stored_set(const cilhip_ctx* c, IterArgs& a, bool symmetric_normals) {
  a.src = c->pairs.src_view; a.ns = c->pairs.count; a.nn_pos = c->pairs.posd; a.nn_d2 = c->pairs.d2;
  a.src_nrm = (symmetric_normals && c->d_src_nrm && c->symmetric) ? c->pairs.nrm_view : nullptr;
}

// Accumulate over the stored set (matches or pair list; transform = nn_T), one streaming pass per metric of `metrics`, and bring the
// reduced sums to the host: pass k fills sums[k * SUMS_MAX ...].  innerL / innert: the inner transform of a Gauss-Newton step (null: none).
static int accumulate_passes(cilhip_ctx* c, const int* metrics, int np, bool symmetric_normals, bool no_centering, const double innerL[9],
                             const double innert[3], double* sums, const CorrWeights* cw) {
  for (int i = 0; i < np * SUMS_MAX; ++i) sums[i] = 0.0;
  launch_init_state(c->d_state, c->nn_T, c->src_mean, c->stream);
  if (innerL) {
    IcpState hs;
    CK(c, hipMemcpyAsync(&hs, c->d_state, sizeof(hs), hipMemcpyDeviceToHost, c->stream));
    CK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 9; ++i) { hs.innerL[i] = (float)innerL[i]; hs.dLd[i] = innerL[i]; }
    for (int i = 0; i < 3; ++i) { hs.innert[i] = (float)innert[i]; hs.dtd[i] = innert[i]; }
    CK(c, hipMemcpyAsync(c->d_state, &hs, sizeof(hs), hipMemcpyHostToDevice, c->stream));
  }
  IterArgs a = make_iter_args(c, 0.0f);
  if (cw) a.cw = *cw;
  if (c->have_pairs) use_stored_set(c, a, symmetric_normals);
  if (!symmetric_normals) a.src_nrm = nullptr;
  a.no_centering = no_centering ? 1 : 0;
  if (a.ns == 0) return CILHIP_OK;
  const int nb = iter_num_blocks(a.ns);
  const int grc = ensure_partial_rows(c, (size_t)nb);
  if (grc) return grc;
  a.partials = c->d_partials;
  for (int k = 0; k < np; ++k) {
    launch_iter(a, metrics[k], false, false, nb, c->stream);
    launch_reduce_partials(c->d_partials, nb, c->d_stage, c->d_sums + k * SUMS_MAX, c->stream);
  }
  CK(c, hipGetLastError());
  CK(c, hipMemcpyAsync(sums, c->d_sums, (size_t)np * SUMS_MAX * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  CK(c, hipStreamSynchronize(c->stream));
  return CILHIP_OK;
}
// ... one pass of the rigid classes' metrics (the symmetric objective reads the source normals)
static int accumulate_stored(cilhip_ctx* c, int metric, const double innerL[9], const double innert[3], double sums[SUMS_MAX],
                             const CorrWeights* cw = nullptr) {
  return accumulate_passes(c, &metric, 1, true, false, innerL, innert, sums, cw);
}

// A transform estimated between the centred clouds, taken back: tform = t_dst * tform * t_src, t_src = the mean of the source under nn_T
static void uncentre(const cilhip_ctx* c, const double L[9], double t[3]) {
  float smt[3];
  transform_point(c->nn_T, c->src_mean[0], c->src_mean[1], c->src_mean[2], smt[0], smt[1], smt[2]);
  for (int r = 0; r < 3; ++r)
    t[r] = t[r] - (L[r * 3] * (double)smt[0] + L[r * 3 + 1] * (double)smt[1] + L[r * 3 + 2] * (double)smt[2]) + (double)c->dst_mean[r];
}

// The Gauss-Newton loop of the rigid combined-metric estimates (transform_estimation.hpp:237-367).  `terms(L, t, g)` accumulates one
// iteration's sums under the inner transform and says how gn_normal_equations weighs them -- or that there is nothing to estimate from
// (:264-272: identity, not converged).  max_iter 0: one accumulation for that test only, no step.  c: whose clouds the estimate is between.
struct GnTerms { double sums[SUMS_MAX]; double w_p2p, w_p2pl; bool point_weighted; bool stop; };
template <class Terms>
static int rigid_gn_solve(const cilhip_ctx* c, size_t max_iter, float conv_tol, Terms terms, float dT[16], double* AtA_out, double* Atb_out, int* converged) {
  double L[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
  int conv = 0;
  const size_t steps = max_iter ? max_iter : 1;
  for (size_t it = 0; it < steps; ++it) {
    GnTerms g;
    const int rc = terms(L, t, g);
    if (rc) return rc;
    if (g.stop) return CILHIP_OK;
    if (max_iter == 0) break;
    double AtA[36], Atb[6], dth[6];
    gn_normal_equations(g.sums, g.w_p2p, g.w_p2pl, AtA, Atb, g.point_weighted);
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
  uncentre(c, L, t);
  pack_T(L, t, dT);
  if (converged) *converged = conv;
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
  memcpy(dT, kIdentity16, sizeof(kIdentity16));
  if (converged) *converged = 0;
  if (AtA_out) for (int i = 0; i < 36; ++i) AtA_out[i] = 0.0;
  if (Atb_out) for (int i = 0; i < 6; ++i) Atb_out[i] = 0.0;
  const bool wp = w_p2p > 0.0f, wl = w_p2pl > 0.0f;
  if (!wp && !wl) return CILHIP_OK;                      // transform_estimation.hpp:264-272
  if (wl && !c->has_normals) return CILHIP_OK;           // dst_p.cols() != dst_n.cols() -> identity, false
  const int metric = (wp && wl) ? IM_BOTH : (wl ? IM_PLANE : IM_POINT);
  const CorrWeights cw = corr_weights_of(c, true, w_p2p, w_p2pl);
  return rigid_gn_solve(c, max_iter, conv_tol, [&](const double L[9], const double t[3], GnTerms& g) {
    const int rc = accumulate_stored(c, metric, L, t, g.sums, &cw);
    g.stop = !(g.sums[0] > 0.0);                         // no correspondences: identity
    g.point_weighted = cw.enabled != 0;                  // (metric weights inside the per-pair weights)
    g.w_p2p = !wp ? 0.0 : (cw.enabled ? 1.0 : (double)w_p2p);
    g.w_p2pl = !wl ? 0.0 : (cw.enabled ? 1.0 : (double)w_p2pl);
    return rc;
  }, dT, AtA_out, Atb_out, converged);
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
  memcpy(dT, kIdentity16, sizeof(kIdentity16));
  if (converged) *converged = 0;
  const bool wp = w_p2p > 0.0f, wl = w_p2pl > 0.0f;
  if (!wp && !wl) return CILHIP_OK;                      // transform_estimation.hpp:264-272
  return rigid_gn_solve(cp, max_iter, conv_tol, [&](const double L[9], const double t[3], GnTerms& g) {
    bool weighted_sums = false;
    const int rc = combined_two_sets_step(cp, cl, wp, wl, w_p2p, w_p2pl, L, t, g.sums, &weighted_sums);
    const bool has_p2p = wp && g.sums[44] > 0.0, has_p2pl = wl && g.sums[0] > 0.0;     // :264-267
    g.stop = (!has_p2p && !has_p2pl) || (has_p2pl && !cl->has_normals);                // :269-272: identity, false
    g.point_weighted = true;
    g.w_p2p = !has_p2p ? 0.0 : (weighted_sums ? 1.0 : (double)w_p2p);
    g.w_p2pl = !has_p2pl ? 0.0 : (weighted_sums ? 1.0 : (double)w_p2pl);
    return rc;
  }, dT, nullptr, nullptr, converged);
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
// passes on the device (one without plane terms), one copy to the host: accumulate_passes.
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
  double sums[3 * SUMS_MAX] = {0};                       // (the passes that do not run leave zeros)
  // weight evaluators (the combined-metric class only: `centered` distinguishes it from the point-to-point class here)
  if (centered) { const int wrc = prepare_pair_weights(c); if (wrc) return wrc; }
  const CorrWeights cw = corr_weights_of(c, centered != 0, w_p2p, w_p2pl);
  const int passes[3] = {IM_AFF0, IM_AFF1, IM_AFF2};      // (the symmetric metric exists for the rigid classes only)
  const int rc = accumulate_passes(c, passes, wl ? 3 : 1, false, centered == 0, nullptr, nullptr, sums, &cw);
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
  if (centered) uncentre(c, L, t);                       // :473 tform = t_dst * tform * t_src
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
  if (it == 0) drop_correspondences(c); else c->matches_origin = 1;
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

// warp_field_icp.hip -- the non-rigid ICP loop over a context: icp_base.hpp:68-87 with the steps of
// icp_warp_field_combined_metric_sparse.hpp:202-240.  Host code only; the kernels and the estimator are warp_field.hip's.
//
// Per iteration: the dense field warps the source on the device, the context takes the warped cloud as its source
// (cilhip_set_source, device memory) and searches it under the identity (its exact 1-NN search), the estimator runs on the
// device-resident matches, the control transforms are composed (T_ctrl[i] = T_iter[i] * T_ctrl[i]) and resampled.  One word comes
// back per iteration: max_i |R_iter,i - I|_F^2 + |t_iter,i|^2.  At the end the context has the caller's source again.
// Rigid and affine node transforms (the classes at icp_common_instances.hpp:313-314 and :322-323) share the loop: the kind goes to the
// estimator and to the resample, and nothing else differs.
#include "ctx.hpp"
#include "stateless.hpp"
#include "warp_field.hpp"

#include <cmath>

namespace {

// one loop for both kinds of node transform: the estimator and the resample are the only steps that differ (section 17.4, A8)
int wf_icp_run(const char* F, WfKind kind, cilhip_ctx* c, cilhip_warp_field* wf, const cilhip_warp_params* prm, size_t max_iter, float conv_tol, float max_sq_dist,
               const float* ctrl_T0_or_null, float* ctrl_T_out, float* dense_T_out_or_null, cilhip_icp_result* out) {
  if (!c) return st_fail(CILHIP_ERR_INVALID, F, "the context is null");
  auto refuse = [c, F](int code, const char* why) { st_fail(code, F, why); return fail(c, code, st_slot().c_str()); };
  if (!wf || !ctrl_T_out || !out) return refuse(CILHIP_ERR_INVALID, "the warp field, ctrl_T_out or out is null");
  if (const char* why = wf_params_refusal(prm)) return refuse(CILHIP_ERR_INVALID, why);
  if (!std::isfinite(conv_tol) || std::isnan(max_sq_dist)) return refuse(CILHIP_ERR_INVALID, "conv_tol or max_sq_dist is not finite");
  if (!c->has_target || !c->has_source) return refuse(CILHIP_ERR_INVALID, "set_target and set_source first");
  if (wf_device(wf) != c->device) return refuse(CILHIP_ERR_INVALID, "the warp field lives on another device than the context");
  if ((size_t)c->ns != wf_n_src(wf)) return refuse(CILHIP_ERR_INVALID, "the context's source has another size than the warp field's");
  if (prm->w_p2pl > 0.0f && !c->has_normals) return refuse(CILHIP_ERR_INVALID, "w_p2pl > 0 needs a target with normals");
  if (c->proj_on) return refuse(CILHIP_ERR_UNSUPPORTED, "a projection is set on the context (the projective warp-field classes are not built)");
  if (c->search_dir != 0) return refuse(CILHIP_ERR_UNSUPPORTED, "search directions other than SECOND_TO_FIRST");
  if (filters_active(c)) return refuse(CILHIP_ERR_UNSUPPORTED, "correspondence post-filters");
  if (weighted(c) || feat6(c)) return refuse(CILHIP_ERR_UNSUPPORTED, "non-unity correspondence weights or a feature adaptor");
  if (c->index_offset || c->partial_target) return refuse(CILHIP_ERR_UNSUPPORTED, "a target shard");
  st_clear();
  ST_CK(F, hipSetDevice(c->device));
  hipStream_t s = wf_stream(wf);
  const size_t n_src = wf_n_src(wf), n_ctrl = wf_n_ctrl(wf), n_dst = c->grid.n;
  float* b[7];
  uint32_t* d_nn = nullptr;
  if (const int rc = wf_loop_buffers(F, wf, n_dst, b, &d_nn)) return rc;
  float *src0 = b[0], *warped = b[1], *dense = b[2], *T = b[3], *T_iter = b[4], *dst = b[5], *nrm = b[6];
  ST_CK(F, hipStreamSynchronize(c->stream));
  ST_CK(F, hipMemcpyAsync(src0, c->d_src_xyz, 3 * n_src * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (const int rc = wf_unsort_target_dev(F, s, c->grid.pts, c->has_normals ? c->grid.nrm : nullptr, c->grid.n, dst, nrm)) return rc;
  if (ctrl_T0_or_null) ST_CK(F, hipMemcpyAsync(T, ctrl_T0_or_null, 16 * n_ctrl * sizeof(float), hipMemcpyHostToDevice, s));
  else if (const int rc = wf_set_identity_dev(F, s, T, n_ctrl)) return rc;
  if (const int rc = wf_resample_dev(F, wf, T, dense, kind)) return rc;

  static const float I16[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  size_t iterations = 0, ncorr = 0;
  float last_delta = INFINITY;
  int rc = CILHIP_OK;
  while (iterations < max_iter) {
    if ((rc = wf_transform_points_dev(F, s, dense, src0, n_src, warped))) break;
    if (hipStreamSynchronize(s) != hipSuccess) { rc = st_fail(CILHIP_ERR_HIP, F, "hipStreamSynchronize"); break; }
    if ((rc = cilhip_set_source(c, warped, n_src, CILHIP_MEM_DEVICE))) break;
    if ((rc = cilhip_find_correspondences(c, I16, max_sq_dist, &ncorr))) break;
    if ((rc = cilhip_get_nn(c, d_nn, nullptr, CILHIP_MEM_DEVICE))) break;
    if ((rc = wf_estimate_dev(F, wf, dst, c->has_normals ? nrm : nullptr, n_dst, warped, d_nn, *prm, T_iter, nullptr, kind))) break;
    float max_delta_sq = 0.0f;
    if ((rc = wf_compose_dev(F, wf, T_iter, T, &max_delta_sq))) break;
    if ((rc = wf_resample_dev(F, wf, T, dense, kind))) break;
    last_delta = std::sqrt(max_delta_sq);
    iterations++;
    if (last_delta < conv_tol) break;
  }
  // the caller's source again, whatever happened (optional source normals and colour features belong to a source: set them again)
  (void)hipStreamSynchronize(s);
  const int back = cilhip_set_source(c, src0, n_src, CILHIP_MEM_DEVICE);
  if (rc == CILHIP_OK) rc = back;
  if (rc != CILHIP_OK) { if (st_slot().empty()) st_fail(rc, F, c->err.c_str()); else c->err = st_slot(); return rc; }
  ST_CK(F, hipMemcpyAsync(ctrl_T_out, T, 16 * n_ctrl * sizeof(float), hipMemcpyDeviceToHost, s));
  if (dense_T_out_or_null) ST_CK(F, hipMemcpyAsync(dense_T_out_or_null, dense, 16 * n_src * sizeof(float), hipMemcpyDeviceToHost, s));
  ST_CK(F, hipStreamSynchronize(s));
  for (int i = 0; i < 16; ++i) out->T[i] = I16[i];      // (a warp field has no single transform)
  out->iterations = iterations; out->last_delta_norm = last_delta; out->last_ncorr = ncorr;
  return CILHIP_OK;
}

}  // namespace

extern "C" int cilhip_warp_field_icp_run(cilhip_ctx* c, cilhip_warp_field* wf, const cilhip_warp_params* prm, size_t max_iter, float conv_tol, float max_sq_dist,
                                         const float* ctrl_T0_or_null, float* ctrl_T_out, float* dense_T_out_or_null, cilhip_icp_result* out) {
  return wf_icp_run("warp_field_icp_run", WF_RIGID, c, wf, prm, max_iter, conv_tol, max_sq_dist, ctrl_T0_or_null, ctrl_T_out, dense_T_out_or_null, out);
}
extern "C" int cilhip_warp_field_icp_run_affine(cilhip_ctx* c, cilhip_warp_field* wf, const cilhip_warp_params* prm, size_t max_iter, float conv_tol, float max_sq_dist,
                                                const float* ctrl_T0_or_null, float* ctrl_T_out, float* dense_T_out_or_null, cilhip_icp_result* out) {
  return wf_icp_run("warp_field_icp_run_affine", WF_AFFINE, c, wf, prm, max_iter, conv_tol, max_sq_dist, ctrl_T0_or_null, ctrl_T_out, dense_T_out_or_null, out);
}

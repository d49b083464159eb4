// warp_field.hpp -- what warp_field.hip (kernels, the handle, the estimator) shows to warp_field_icp.hip (the ICP loop over a
// context).  Host code only; every pointer named d_* is a device pointer and every call enqueues on the handle's own stream.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/cilantro_hip/c_api.h"

namespace cilhip {

size_t wf_n_src(const cilhip_warp_field* wf);
size_t wf_n_ctrl(const cilhip_warp_field* wf);
int wf_device(const cilhip_warp_field* wf);
hipStream_t wf_stream(cilhip_warp_field* wf);
// one argument rule shared by the estimate entry and the loop: null = the parameters are fine
const char* wf_params_refusal(const cilhip_warp_params* p);

// the node transforms of a call: rigid (section 17.1: 6 unknowns per node, output and resample through rotation()) or affine
// (section 17.4: 12 unknowns, output and resample as they are).  The first affine estimate grows the handle's solver scratch.
enum WfKind { WF_RIGID = 6, WF_AFFINE = 12 };

// the estimator of DESIGN.md section 17 on device-resident arrays; T_out: n_ctrl * 16 floats (column-major 4 x 4).  Synchronises.
int wf_estimate_dev(const char* family, cilhip_warp_field* wf, const float* d_dst, const float* d_nrm_or_null, size_t n_dst, const float* d_src, const uint32_t* d_nn,
                    const cilhip_warp_params& prm, float* d_T_out, cilhip_warp_stats* stats_or_null, WfKind kind = WF_RIGID);
// control transforms -> one transform per source point (resampleTransforms); enqueues only
int wf_resample_dev(const char* family, cilhip_warp_field* wf, const float* d_ctrl_T, float* d_dense_T, WfKind kind = WF_RIGID);
// out[i] = T[i] * xyz[i]; enqueues only
int wf_transform_points_dev(const char* family, hipStream_t s, const float* d_T, const float* d_xyz, size_t n, float* d_out);
// T[i] = T_iter[i] * T[i] for the n_ctrl control transforms; *max_delta_sq = max_i |R_iter,i - I|_F^2 + |t_iter,i|^2.  Synchronises.
int wf_compose_dev(const char* family, cilhip_warp_field* wf, const float* d_T_iter, float* d_T, float* max_delta_sq);
// the loop's buffers, owned by the handle (grown on demand): [0] 3 n_src source copy, [1] 3 n_src warped, [2] 16 n_src dense field,
// [3] 16 n_ctrl control transforms, [4] 16 n_ctrl step, [5] 3 n_dst target points, [6] 3 n_dst target normals; nn: n_src indices
int wf_loop_buffers(const char* family, cilhip_warp_field* wf, size_t n_dst, float* bufs[7], uint32_t** nn);
// dst[3 * original index] <- the grid's sorted {x, y, z, index} records (and the normals); enqueues only
int wf_unsort_target_dev(const char* family, hipStream_t s, const float4* pts, const float4* nrm_or_null, uint32_t n, float* d_xyz, float* d_nrm);
int wf_set_identity_dev(const char* family, hipStream_t s, float* d_T, size_t n);

}  // namespace cilhip

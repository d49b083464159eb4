/*
 * cilantro_hip/c_api.h -- C ABI of the MI355X-native rigid ICP engine (libcilantro_hip.so).
 *
 * cilantro (the reference) has NO ABI for this path: it is C++ template duck typing
 * (registration/icp_base.hpp:8-10,114).  This header is the drop-in
 * boundary a maintainer binds instead: plain pointers and sizes, no Eigen / torch types.
 * Each entry point cites the reference interface it replaces (paths relative to
 * /root/reference/include/cilantro/).  The C++ mirror of the reference classes that sits on
 * top of it is include/cilantro_hip/icp.hpp; INTEGRATION.md shows the binding.
 *
 * Conventions (identical to the reference):
 *   - clouds: const float* xyz, point i at xyz[3i..3i+2]  (Eigen::Matrix<float,3,Dynamic>
 *     column-major, core/data_containers.hpp:155-156); "first" = dst/target, "second" = src.
 *   - transforms: float[16], 4x4 COLUMN-major (Eigen::Transform<float,3,Isometry>::data()).
 *   - all distances are SQUARED L2 (core/kd_tree.hpp:46-47).
 *   - every call returns 0 on success or a negative cilhip_status; cilhip_last_error() has text.
 *     Nothing throws across the boundary.  A context is single-caller (like one ICP object).
 *   - `mem` arguments: CILHIP_MEM_HOST = pointer is host memory (copied), CILHIP_MEM_DEVICE =
 *     pointer is device memory on the context's GPU (copied device-to-device; caller keeps
 *     ownership either way).
 */
#ifndef CILANTRO_HIP_C_API_H
#define CILANTRO_HIP_C_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cilhip_ctx cilhip_ctx;

typedef enum {
  CILHIP_OK = 0,
  CILHIP_ERR_INVALID = -1,      /* bad argument / call order */
  CILHIP_ERR_HIP = -2,          /* HIP runtime failure (no device, OOM, launch failure) */
  CILHIP_ERR_UNSUPPORTED = -3,  /* option combination the GPU path does not implement */
  CILHIP_ERR_NO_DEVICE = -4
} cilhip_status;

enum { CILHIP_MEM_HOST = 0, CILHIP_MEM_DEVICE = 1 };

/* metric selector: which reference ICP class is being replaced */
enum {
  CILHIP_METRIC_POINT_TO_POINT = 0, /* PointToPointMetricSingleTransformICP (closed-form SVD),
                                       registration/icp_single_transform_point_to_point_metric.hpp */
  CILHIP_METRIC_COMBINED = 1        /* CombinedMetricSingleTransformICP (Gauss-Newton; defaults
                                       w_p2p=0, w_p2pl=1 = point-to-plane),
                                       registration/icp_single_transform_combined_metric.hpp */
};

/* ---- lifetime -------------------------------------------------------------------------------- */
/* device: HIP device ordinal.  Owns one stream, all device buffers, the target grid index. */
int cilhip_create(cilhip_ctx** out, int device);
void cilhip_destroy(cilhip_ctx* ctx);
/* ctx == NULL names the calling thread's last failed stateless call (the entries that take `int device` instead of a context), of any
 * family; "null context" when the last such call passed its argument rules and did not fail. */
const char* cilhip_last_error(const cilhip_ctx* ctx);
/* Run all work on a caller-owned hipStream_t (e.g. torch's current stream) instead of the
 * context's own; pass NULL to go back.  The caller keeps the stream alive.  NULL never means the legacy default
 * stream here: a caller whose work runs there (torch's default stream reports handle 0) passes hipStreamLegacy --
 * otherwise the context's own NON-BLOCKING stream is not ordered with that work at all. */
int cilhip_set_stream(cilhip_ctx* ctx, void* hip_stream);
int cilhip_synchronize(cilhip_ctx* ctx);

/* ---- Non-finite points ------------------------------------------------------------------------
 * Depth sensors produce NaN and +-inf points; every search entry point accepts them, in the indexed cloud and among the queries
 * (cilhip_set_target, cilhip_set_source / cilhip_find_correspondences in all three search directions, cilhip_knn3f,
 * cilhip_normals_*, cilhip_radius_search3f):
 *   - a point with ANY non-finite coordinate keeps its index, is never returned as a neighbour and, as a query, finds nothing
 *     (cilhip_get_nn: 0xFFFFFFFF; k-NN / radius lists: count 0, padding only; normals: a NaN row);
 *   - every other point and query gets exactly what the same call returns on the clouds with those rows removed, indices
 *     mapped back.  This is the brute force with IEEE comparisons -- a NaN or infinite squared distance is never
 *     < max_sq_dist, also when max_sq_dist is INFINITY -- and what nanoflann's dist < worstDist does with such a point;
 *   - the grid's bounding box is taken over the finite coordinates only; a cloud without a single finite point behaves as an
 *     empty index (every search returns none, n is unchanged);
 *   - a transform with a NaN or infinite entry makes every query non-finite: zero correspondences, CILHIP_OK;
 *   - cilhip_get_means keeps returning the IEEE mean (NaN or inf), as the reference's dst_mean_ / src_mean_ would;
 *   - WHICH of several exactly equidistant points is named is not defined on a cloud that holds non-finite points (the
 *     reference's tree over NaN coordinates is not meaningful either).
 * A FINITE cloud whose coordinates leave the range a single-precision grid can index (|coordinate| + 4 * extent must stay
 * below FLT_MAX: coordinates near +-3.4e38) is refused: CILHIP_ERR_UNSUPPORTED with a message, never a wrong grid.
 * Not covered: the ICP loops on such clouds (the combined metric's means are NaN in the reference too) and the 6-D / 9-D
 * feature searches with non-finite normals or colours.  DESIGN.md, "Non-finite points". */
/* ---- clouds ---------------------------------------------------------------------------------- */
/* Target ("first"/dst) cloud + optional normals.  Builds the uniform-grid index on the GPU.
 * Replaces: KDTree ctor core/kd_tree.hpp:162-170 -> nanoflann buildIndex
 * (3rd_party/nanoflann/nanoflann.hpp:1661-1687), lazily triggered at
 * correspondence_search/correspondence_search_kd_tree.hpp:202-203; and the dst_mean_ of
 * registration/icp_single_transform_combined_metric.hpp:51-54.
 * Points with a non-finite coordinate are kept (their indices stay) but are in no cell: "Non-finite points" above.  A finite cloud
 * beyond the range of a single-precision grid: CILHIP_ERR_UNSUPPORTED. */
int cilhip_set_target(cilhip_ctx* ctx, const float* xyz, const float* normals_or_null, size_t n,
                      int mem);
/* Source ("second"/src) cloud.  Replaces the PointFeaturesAdaptor src_feat_
 * (correspondence_search/common_transformable_feature_adaptors.hpp:14-17) and src_mean_
 * (icp_single_transform_combined_metric.hpp:55-58). */
int cilhip_set_source(cilhip_ctx* ctx, const float* xyz, size_t n, int mem);
/* Optional source normals (call after cilhip_set_source; NULL removes them).  With them the combined
 * metric becomes the SYMMETRIC objective, exactly as constructing CombinedMetricSingleTransformICP with four
 * clouds does (icp_single_transform_combined_metric.hpp:63-93,182-189 -> estimateTransformSymmetricMetric,
 * transform_estimation.hpp:604-739: n = n_dst + R*n_src), and computeResiduals adds them (:237). */
int cilhip_set_source_normals(cilhip_ctx* ctx, const float* normals_or_null, int mem);
/* The per-registration set-up of THIS design (the reference has no counterpart: its queries are searched in their
 * given order, correspondence_search_kd_tree_utilities.hpp:26): spatial pre-sort of the source by the target-grid cube
 * of T*s and the tile table of the LDS-tiled search.  It runs lazily inside the first search / cilhip_icp_run of a
 * (target, source) pair and is re-run when the transform has moved the source by more than a few cells; this entry
 * runs it explicitly so that its cost can be put on the bench line.  T NULL = identity; force != 0 re-sorts even if a
 * valid order exists; ms_or_null = host wall time of the step (allocations and the two host round trips of the
 * radix sort included), stream-synchronised. */
int cilhip_prepare_source(cilhip_ctx* ctx, const float* T_or_null, int force, double* ms_or_null);
/* dst_mean_ / src_mean_ as the ICP classes hold them (f64 sum, rounded to f32). */
int cilhip_get_means(cilhip_ctx* ctx, float dst_mean[3], float src_mean[3]);
/* Per-point colours of both clouds (packed rgb, n_target / n_source triples) for the point + colour feature adaptor
 * (PointColorFeaturesAdaptor3f(points, colors, color_weight), common_transformable_feature_adaptors.hpp:164-252; options
 * "feature_kind" = 1, "feature_normal_weight" = the colour weight) and for the 9-D point + normal + colour adaptor (:255-343;
 * "feature_kind" = 2, "feature_color_weight").  After cilhip_set_target and cilhip_set_source. */
int cilhip_set_color_features(cilhip_ctx* ctx, const float* dst_rgb, const float* src_rgb, int mem);
/* CorrespondenceSearchKDTree::getFirstSearchTree() / setFirstSearchTree(tree) (correspondence_search/correspondence_search_kd_tree.hpp:273-296;
 * the shared_ptr<SearchTree> of :299-300): a second engine searches the index another engine built instead of building its own --
 * many sources registered against one model (examples/fusion.cpp style) pay for the index once.  `ctx` takes `from`'s target as it
 * stands: the cell-sorted points and normals, the cell table, and everything built on top of them by now (point+normal records,
 * the nearest-other-point table of the warm-started iterations, the order tables of the reference's tree, the index -> position
 * map), without copying: the allocations become a reference-counted share, so either context may be destroyed or given another
 * target first.  What a context builds later is its own.  Same device; neither context may have work in flight on another host
 * thread during the call.  Colour features are per context (cilhip_set_color_features again). */
int cilhip_share_target(cilhip_ctx* ctx, cilhip_ctx* from);

/* ---- correspondence search (engine concept) -------------------------------------------------- */
/* CorrespondenceSearchKDTree::findCorrespondences(tform), SECOND_TO_FIRST, L2, identity
 * evaluator, inlier_fraction 1, no one-to-one/reciprocity
 * (correspondence_search/correspondence_search_kd_tree.hpp:107-229 live code :185-228):
 *   q_i = T*s_i (common_transformable_feature_adaptors.hpp:28-33), exact 1-NN of q_i among dst with
 *   d2 < max_sq_dist, strict (correspondence_search_kd_tree_utilities.hpp:26-33; nanoflann.hpp:1901).
 * Ties on d2 (several target points at EXACTLY the smallest distance) name the point the reference's kd-tree traversal meets first
 * (option "tie_rule" = 2, the default; 0: the lowest dst index).
 * Results stay on the device; n_found (optional) forces a sync and returns the count.
 * Source or target points with a non-finite coordinate, or such an entry in T, match nothing ("Non-finite points" above); the same holds
 * for the grid over the source that search directions FIRST_TO_SECOND / BOTH build. */
int cilhip_find_correspondences(cilhip_ctx* ctx, const float T[16], float max_sq_dist,
                                size_t* n_found_or_null);
/* Projective association (correspondence_search/correspondence_search_projective.hpp:156-209; DESIGN.md section 14.4, rules S1-S3).
 * K: float[9] column-major intrinsics, w x h the image, extrinsics: float[16] column-major camera pose (camera to world) or NULL.
 * While a projection is set, cilhip_find_correspondences and cilhip_icp_run (SECOND_TO_FIRST) associate through the target's index
 * map (cilhip_points_to_index_map3f's rules under these extrinsics; built lazily, once per target and projection; dropped by
 * cilhip_set_target, cilhip_share_target and this call): per source point q = T s, projected like a map point, matched to the map's
 * point j at its pixel iff |q - p_j|^2 = dx^2 + (dy^2 + dz^2) < max_sq_dist (strict).  Everything that reads "the last search" works
 * on the result.  K == NULL: back to the grid search.  Refused with CILHIP_ERR_UNSUPPORTED while a projection is set: search
 * directions other than SECOND_TO_FIRST, reciprocity, one-to-one, feature adaptors, the pair-weight callback, sharded runs
 * (cilhip_icp_begin ..., cilhip_multi_*, slab and target shards), cilhip_icp_run_two_sets and the affine loop.
 * cilhip_compute_residuals is unaffected.  CILHIP_ERR_INVALID: NULL ctx, non-finite K, w * h == 0 or >= 2^32 - 16. */
int cilhip_set_projection(cilhip_ctx* ctx, const float* K_or_null, size_t w, size_t h, const float* extrinsics_or_null);
/* Per-source raw result of the last search, in ORIGINAL source order: nn_idx[i] = dst index or
 * 0xFFFFFFFF (none), nn_d2[i] = squared distance (undefined when none).  Either may be NULL.
 * "The last search" includes the one of the last executed iteration of cilhip_icp_run: like the reference's engine, which
 * keeps `correspondences_` of its last findCorrespondences call (correspondence_search_kd_tree.hpp:231; the ICP object hands
 * the engine out, registration/icp_base.hpp:32-38), the context answers cilhip_get_nn / cilhip_get_correspondences /
 * cilhip_estimate_* after a run with that iteration's set (found under the transform BEFORE the last update). */
int cilhip_get_nn(cilhip_ctx* ctx, uint32_t* nn_idx, float* nn_d2, int mem);
/* Where the set those calls return comes from: 0 = there is none, 3 = a cilhip_find_correspondences call, 1 = left in device
 * memory by the kernels of the last cilhip_icp_run iteration (the squared distances formed again with the search's pinned
 * arithmetic), 2 = searched again on demand under that iteration's transform (loops whose kernels keep no per-query matches:
 * post-filters, pair-list directions, the feature search, options "fused" / "warm_start" = 0).  The search is exact, so 1 and
 * 2 are the same set; tests use the value to know WHICH kernel's matches they are comparing. */
int cilhip_get_last_matches_origin(cilhip_ctx* ctx, int* origin);
/* The transform (col-major 4x4) the current correspondence set was found under: the argument of the last
 * cilhip_find_correspondences, or -- after cilhip_icp_run -- transform_ as it was BEFORE the last iteration's update, the
 * tform the reference's loop handed its last engine.findCorrespondences(transform_) call
 * (registration/icp_single_transform_combined_metric.hpp:170). */
int cilhip_get_matches_transform(cilhip_ctx* ctx, float T[16]);
/* The reference's SearchResult: CorrespondenceSet<float,size_t> compacted in ascending source
 * index order (correspondence_search_kd_tree_utilities.hpp:45-50; core/correspondence.hpp:9-55),
 * as three host arrays of capacity `cap` (>= n_found): indexInFirst, indexInSecond, value. */
int cilhip_get_correspondences(cilhip_ctx* ctx, uint64_t* index_in_first, uint64_t* index_in_second,
                               float* value, size_t cap, size_t* n_out);

/* ---- estimators on the correspondences of the last search ------------------------------------ */
/* estimateTransformPointToPointMetric (rigid, closed form), registration/transform_estimation.hpp
 * :11-48 via :104-113.  dT_out: the step transform (tform_iter before the rotation() polish).
 * sums_or_null (16 doubles): n, sum p(3), sum q(3), sum p q^T(9, row-major) -- raw moments.
 * Returns CILHIP_OK; *ok_or_null = (n >= 3) as the reference's bool. */
int cilhip_estimate_point_to_point(cilhip_ctx* ctx, float dT_out[16], double* sums_or_null,
                                   int* ok_or_null);
/* estimateTransformCombinedMetric (rigid 3D, unity weights), transform_estimation.hpp:237-367,
 * called as icp_single_transform_combined_metric.hpp:191-196 does (dst_mean, T*src_mean).
 * AtA_or_null (36, row-major) / Atb_or_null (6): first Gauss-Newton step's normal equations.
 * *converged_or_null: the reference's bool return (d_theta.norm() < conv_tol inside max_iter).
 * Reads the stored set of the last search whatever its direction: the per-source matches of SECOND_TO_FIRST or the pair list of
 * FIRST_TO_SECOND / BOTH (one term per pair); with the context's weight evaluators (options) or pair-weight callback. */
int cilhip_estimate_combined(cilhip_ctx* ctx, float w_p2p, float w_p2pl, size_t max_iter,
                             float conv_tol, float dT_out[16], double* AtA_or_null,
                             double* Atb_or_null, int* converged_or_null);

/* Affine closed form: estimateTransformCombinedMetric for Affine / AffineCompact transforms
 * (transform_estimation.hpp:369-476) called as icp_single_transform_combined_metric.hpp:199-204 does (centered != 0:
 * dst_mean, T*src_mean), or estimateTransformPointToPointMetric (affine, :50-102 via :104-113) with
 * w_p2p = 1, w_p2pl = 0, centered = 0 (that overload works on the raw coordinates).  Works on the correspondences of
 * the last cilhip_find_correspondences in every search direction.  AtA_or_null (144, row-major) / Atb_or_null (12):
 * the normal equations in the reference's unknown order (row-major linear part, translation).
 * *ok_or_null: the reference's bool return (terms >= Dim + 1). */
int cilhip_estimate_affine(cilhip_ctx* ctx, float w_p2p, float w_p2pl, int centered, float dT_out[16],
                           double* AtA_or_null, double* Atb_or_null, size_t* n_corr_or_null, int* ok_or_null);

/* ---- the whole ICP loop, fused on the device ------------------------------------------------- */
typedef struct {
  int metric;            /* CILHIP_METRIC_* */
  float w_p2p, w_p2pl;   /* combined metric weights (reference defaults 0 / 1) */
  size_t max_iter;       /* icp_base.hpp:24  (default 15) */
  float conv_tol;        /* icp_base.hpp:25  (default 1e-5) */
  size_t max_opt_iter;   /* max_optimization_iterations_ (default 1) */
  float opt_conv_tol;    /* optimization_convergence_tol_ (default 1e-5) */
  float max_sq_dist;     /* engine max_distance_, SQUARED (default 0.01*0.01) */
} cilhip_icp_params;

typedef struct {
  float T[16];           /* transform_ */
  size_t iterations;     /* iterations_ */
  float last_delta_norm; /* last_delta_norm_ */
  size_t last_ncorr;     /* correspondences used by the last executed iteration */
} cilhip_icp_result;

void cilhip_icp_default_params(cilhip_icp_params* p);
/* IterativeClosestPointBase::estimate() (registration/icp_base.hpp:68-87) with
 * updateCorrespondences()+updateEstimate() of the selected class, all iterations enqueued
 * back-to-back on the stream (convergence is decided on the device); one sync at the end. */
int cilhip_icp_run(cilhip_ctx* ctx, const cilhip_icp_params* prm, const float T0_or_null[16],
                   cilhip_icp_result* out);

/* A caller's OWN correspondence weight evaluators.  The reference takes them as template arguments of the combined-metric classes
 * (registration/icp_single_transform_combined_metric.hpp:10-14, icp_common_instances.hpp:74-97) and its estimators call them once per
 * correspondence: point_corr_evaluator(corr.indexInFirst, corr.indexInSecond, corr.value) and the plane one alike
 * (registration/transform_estimation.hpp:303, :332 rigid; :432, :453 affine; core/common_pair_evaluators.hpp:14-80 are the three stock
 * classes, which the options "point_weight_evaluator" / "plane_weight_evaluator" evaluate on the device).  A functor cannot cross a C
 * boundary onto the device: with a callback set, every combined-metric estimate brings the stored correspondence set to the host, calls
 * fn ONCE with all n correspondences -- index_in_first (target), index_in_second (source), value (the search's squared distance; the
 * feature distance under a feature adaptor), in stored order: ascending source index, or ascending (first, second) for the pair
 * lists of FIRST_TO_SECOND / BOTH -- and fn writes both weights of every pair (the metric weights w_p2p / w_p2pl multiply them as in
 * the reference).  The accumulation then reads the weights from tables; cilhip_icp_run becomes the reference's loop step by step on
 * the host (search, estimate, rotation() polish, compose: cilhip_icp_run_two_sets with this engine in both roles; SECOND_TO_FIRST).
 * Applies to cilhip_estimate_combined, _estimate_combined_two_sets (each context its own callback), _estimate_affine (combined class)
 * and the loops over them; the point-to-point classes have no evaluators.  fn = NULL: back to the option-selected stock evaluators.
 * fn runs on the calling thread, between device passes.  The sharded building blocks (cilhip_icp_begin ...) refuse a context with a
 * callback (CILHIP_ERR_UNSUPPORTED: no host in their loop); the stock evaluators work there. */
typedef void (*cilhip_pair_weight_fn)(void* user, const uint64_t* index_in_first, const uint64_t* index_in_second, const float* value,
                                      size_t n, float* point_weight_out, float* plane_weight_out);
int cilhip_set_pair_weight_callback(cilhip_ctx* ctx, cilhip_pair_weight_fn fn, void* user);

/* ---- building blocks for source-sharded multi-GPU runs (one process per GPU) ----------------- */
/* Each rank holds the full target and a shard of the source.  Per iteration:
 *   cilhip_icp_begin (once)  ->  { cilhip_icp_partial_sums -> all-reduce(sum) of
 *   CILHIP_SUMS_LEN doubles over RCCL (caller, e.g. torch.distributed) -> cilhip_icp_apply_sums }
 * sums_dev: DEVICE pointer to CILHIP_SUMS_LEN doubles owned by the caller.  No host sync. */
#define CILHIP_SUMS_LEN 48
int cilhip_icp_begin(cilhip_ctx* ctx, const cilhip_icp_params* prm, const float T0_or_null[16],
                     const float global_src_mean_or_null[3]);
int cilhip_icp_partial_sums(cilhip_ctx* ctx, double* sums_dev);
int cilhip_icp_apply_sums(cilhip_ctx* ctx, const double* sums_dev);
int cilhip_icp_state(cilhip_ctx* ctx, cilhip_icp_result* out); /* syncs */

/* Spatially sharded runs (SURVEY.md 8(e) partitioning B; no counterpart in the reference, which has one address space):
 * target and source are cut into slabs along one axis -- a context holds the target points of its slab plus a halo of
 * sqrt(max distance) + slack and the source points whose image under T_part falls into the slab -- so every nearest
 * neighbour is local and the only exchange per iteration is cilhip_icp_partial_sums' 48 doubles.  The guard keeps that
 * exact: after every transform update the device bounds how far any point of the source's bounding box (centre,
 * half-extents, SOURCE coordinates, the same box on every rank) can have moved along the axis since the partition; once
 * that exceeds the slack the sticky flag cilhip_get_slab_violation reads is raised (identically on all ranks): the
 * caller re-partitions under the current transform and repeats from its last checked state.  axis < 0 disarms. */
int cilhip_set_slab_guard(cilhip_ctx* ctx, int axis, float slack, const float center[3], const float half_extent[3],
                          const float T_part[16]);
int cilhip_get_slab_violation(cilhip_ctx* ctx, int* violated_out);
/* ... and the loop state right AFTER the update that raised the flag (iterations performed, transform, update norm,
 * correspondence count): that update is still exact -- its search ran inside the halos, the flag is about the next search --
 * so a caller re-partitions under THAT transform and keeps every iteration up to and including it.  Not violated: the
 * current state. */
int cilhip_get_slab_violation_state(cilhip_ctx* ctx, int* violated, cilhip_icp_result* at_violation);

/* ---- target-sharded runs (BASELINE configs[3]: one target too large / sharded over the GPUs of a node) ----
 * Every rank holds ALL source points and ONE shard of the target (set with cilhip_set_target) plus
 *   cilhip_set_shard_info(ctx, global index of the shard's first point, GLOBAL dst mean, GLOBAL src mean).
 * Per iteration (after cilhip_icp_begin):
 *   cilhip_icp_partial_keys(ctx, keys_dev)      keys_dev[i] = (bits(d2) << 32) | global target index of source
 *                                               point i's nearest neighbour in THIS shard (0x7fff...f = none)
 *   all-reduce(MIN, int64) of keys_dev over RCCL  -> the globally nearest target per source point
 *   cilhip_icp_sums_from_keys(ctx, keys_dev, sums_dev)  accumulates only the pairs won by this shard
 *   all-reduce(SUM, f64) of sums_dev;  cilhip_icp_apply_sums(ctx, sums_dev)
 * keys_dev: DEVICE pointer to n_source uint64 (original source order). */
int cilhip_set_shard_info(cilhip_ctx* ctx, uint64_t target_index_offset, const float* dst_mean_or_null,
                          const float* src_mean_or_null);
int cilhip_icp_partial_keys(cilhip_ctx* ctx, uint64_t* keys_dev);
int cilhip_icp_sums_from_keys(cilhip_ctx* ctx, const uint64_t* keys_dev, double* sums_dev);
/* Exactly equidistant nearest points across shards: MIN of (d2, global index) keeps the lowest global index, the reference's kd-tree
 * the first one its traversal meets (core/kd_tree.hpp:82-90, nanoflann.hpp:1885-1961).  A shard notices such a tie in
 * cilhip_icp_sums_from_keys (its own nearest point is exactly as far as the winner's) and counts it like the ties its searches notice
 * (cilhip_get_tie_order_info: pending).  With the WHOLE target's order loaded on every shard (cilhip_tie_order_create over the whole
 * cloud, cilhip_load_tie_order with the shard's global indices) the searches settle the ties inside a shard, and a second key settles
 * them between shards -- per iteration, after the MIN of the first keys:
 *   cilhip_icp_order_keys(ctx, win_keys_dev, order_keys_dev)    order_keys_dev[i] = position of this shard's match of source point i in
 *                                                                 that query's traversal of the whole tree (one bit per level: 0 = the
 *                                                                 child nanoflann's searchLevel descends into first; then the slot
 *                                                                 in the leaf) if the match is at the winning distance, else 0x7fff...f
 *   all-reduce(MIN, 64-bit) of order_keys_dev
 *   cilhip_icp_sums_from_ordered_keys(ctx, win_keys_dev, order_keys_dev, sums_dev)   accumulates the pairs whose key came back
 * Trees deeper than 58 levels: CILHIP_ERR_UNSUPPORTED.  cilhip_multi_set_clouds(partition = 2) runs this protocol by itself. */
int cilhip_icp_order_keys(cilhip_ctx* ctx, const uint64_t* win_keys_dev, uint64_t* order_keys_dev);
int cilhip_icp_sums_from_ordered_keys(cilhip_ctx* ctx, const uint64_t* win_keys_dev, const uint64_t* order_keys_dev, double* sums_dev);

/* ---- residuals ------------------------------------------------------------------------------- */
/* computeResiduals() of both classes (icp_single_transform_combined_metric.hpp:220-243,
 * icp_single_transform_point_to_point_metric.hpp:68-85): unbounded 1-NN of T*s_i, then
 * w_p2p*|p-q|^2 + w_p2pl*(n.(p-q))^2  (metric 0: |p-q|^2).  out: ns floats, original order. */
int cilhip_compute_residuals(cilhip_ctx* ctx, int metric, float w_p2p, float w_p2pl,
                             const float T[16], float* out, int mem);

/* ---- next tier: KMeans3f --------------------------------------------------------- */
/* KMeans<float,3>::cluster(centroids, max_iter, tol, use_kd_tree = false)  (clustering/kmeans.hpp:24-30 ->
 * cluster_ :67-194): brute-force assignment (strict '<' over ascending cluster index, :95-119), centroid
 * update, empty-cluster repair (:134-176, including the reference's quirk that the moved point is not added
 * to the re-seeded cluster's sum), convergence on assignments (:122) or on the centroid shift (:186-188).
 * centroids: HOST array of 3*k floats, in = initial centroids, out = final.  labels_out: HOST array of n
 * (point_to_cluster_index_map_) or NULL.  k <= 2048.  Cluster sums are exact (fixed point) instead of the
 * reference's serial f32 sums; labels are bit-identical to the reference given identical centroids. */
int cilhip_kmeans3f(int device, const float* xyz, size_t n, int mem, float* centroids, size_t k, size_t max_iter,
                    float tol, uint32_t* labels_out, size_t* iterations_out);
/* The brute-force branch's assignment (kmeans.hpp:95-119: argmin over all k centroids, strict '<' over ascending index) is computed
 * EXACTLY with pruning by default: the centroids are binned into a grid (rebuilt every Lloyd iteration), a point looks at the 3x3x3
 * (then 5x5x5) block of cells around its own with the branch's own distance expression and a proof that nothing outside can win or tie,
 * and falls back to all k centroids otherwise -- labels bit-identical to the exhaustive pass (50M x 1024: 8.05 -> 1.47 ms per Lloyd
 * iteration).  on = 0 keeps the exhaustive pass (process-wide; tests, A/B runs); both branches (use_kd_tree or not) are pruned. */
int cilhip_kmeans_set_pruning(int on);
/* one assignment pass only (kmeans.hpp:95-119) */
int cilhip_kmeans3f_assign(int device, const float* xyz, size_t n, int mem, const float* centroids, size_t k,
                           uint32_t* labels_out);
/* ... with the reference's `use_kd_tree` argument (clustering/kmeans.hpp:24-30, branch :86-94 -- the mode examples/kmeans.cpp
 * uses): a kd-tree over the centroids is only a way of finding the same nearest centroid, so the device runs the same pass (pruned
 * through the centroid grid like the brute-force branch's: 50M x 1024 in 1.9 ms per Lloyd iteration, 2.2 - 2.7 ms when exact ties are met);
 * what the flag changes is the ROUNDING of the compared distance -- nanoflann's L2 metric ((dx*dx)+(dy*dy))+(dz*dz)
 * instead of Eigen's squaredNorm pairing of the brute-force branch -- so that labels equal the reference's kd-tree branch
 * wherever its nearest centroid is unique; among EXACTLY equidistant centroids the one the reference's traversal meets first: the
 * order tables of the tree over the iteration's centroids are built on the device (one workgroup for up to 2048 points: a fraction of a
 * millisecond; the reference builds its KDTree at :87) in the iterations whose pass met such points -- it lists them, k_fix_ties settles them with tie_before afterwards
 * (cilhip_knn_set_tie_rule(0): the lowest index instead).  tests/test_gpu_tie_rule.py: lattice centroids, label for label. */
int cilhip_kmeans3f_ex(int device, const float* xyz, size_t n, int mem, float* centroids, size_t k, size_t max_iter, float tol, int use_kd_tree,
                       uint32_t* labels_out, size_t* iterations_out);
int cilhip_kmeans3f_assign_ex(int device, const float* xyz, size_t n, int mem, const float* centroids, size_t k, int use_kd_tree,
                              uint32_t* labels_out);

/* KMeans over SHARDS of the points (last row: "points sharded, centroids replicated; all-reduce of k x (3 sums +
 * count)"): one shard object per device / rank holds its points and their labels; a Lloyd iteration is cilhip_kmeans_shard_assign on
 * every shard under the same centroids, the SUM of the shards' fixed-point sums {x, y, z, count} per cluster (int64: exact, order-free --
 * MPI / RCCL all-reduce of 4k integers), then clustering/kmeans.hpp:122-188 on the summed values, identically on every rank.  All shards
 * of a run use ONE scale exponent: cilhip_kmeans_scale_exponent(largest |coordinate| over all shards, total point count).  The
 * empty-cluster repair (:134-176) needs the farthest member of a cluster over all shards: cilhip_kmeans_shard_farthest returns this shard's
 * candidate as a key (bits(distance^2) << 32 | 0xFFFFFFFF - GLOBAL index; 0 = no member) whose MAXIMUM over the shards names the
 * reference's point (ties: lowest index); its owner moves it (cilhip_kmeans_shard_move_point: new label, coordinates out -- every rank
 * subtracts them from the donor cluster's sums).  With one shard holding all points this is cilhip_kmeans3f_ex itself (it runs on these
 * calls); with several the centroids, labels and iteration counts are the single-device run's bit for bit (the sums are integers).
 * cilantro_amd/distributed_models.py: ShardedKMeans3f is the loop over torch.distributed; tests/test_distributed_cpu.py (gloo, world 2)
 * and tests/test_gpu_distributed.py (two processes, HIP shards). */
typedef struct cilhip_kmeans_shard cilhip_kmeans_shard;
int cilhip_kmeans_shard_create(int device, const float* xyz, size_t n, int mem, size_t k, uint64_t index_offset, cilhip_kmeans_shard** out);
void cilhip_kmeans_shard_destroy(cilhip_kmeans_shard* shard);
int cilhip_kmeans_shard_maxabs(cilhip_kmeans_shard* shard, float* maxabs_out);
int cilhip_kmeans_scale_exponent(double maxabs_all, size_t n_all);
int cilhip_kmeans_shard_assign(cilhip_kmeans_shard* shard, const float* centroids, int scale_exponent, int use_kd_tree, int64_t* sums_out /* [4k] */,
                               uint64_t* changed_out);
int cilhip_kmeans_shard_farthest(cilhip_kmeans_shard* shard, uint32_t cluster, const float center[3], uint64_t* key_out);
int cilhip_kmeans_shard_move_point(cilhip_kmeans_shard* shard, uint64_t global_index, uint32_t to_cluster, float xyz_out[3]);
/* Non-finite coordinates have no fixed-point image: they are left out of cilhip_kmeans_shard_maxabs and of the sums (their point still
 * counts).  flags_out[j] names what the last cilhip_kmeans_shard_assign met among cluster j's members of THIS shard, three bits per
 * coordinate d (<< 3d): 1 a NaN, 2 a +inf, 4 a -inf; the bitwise OR over the shards is the run's.  Coordinate d of such a cluster's
 * centroid is what the reference's IEEE sum gives: NaN for a NaN or both infinities, else the infinity. */
int cilhip_kmeans_shard_nonfinite(cilhip_kmeans_shard* shard, uint32_t* flags_out /* [k] */);
int cilhip_kmeans_shard_labels(cilhip_kmeans_shard* shard, uint32_t* labels_out);

/* ---- next tier: PlaneRANSACEstimator3f ----------------------------------- */
typedef struct {
  float normal[3];     /* Eigen::Hyperplane<float,3>::normal()  (unit; sign as PCA leaves it)               */
  float offset;        /* ::offset(): the plane is normal . x + offset = 0                                  */
  size_t iterations;   /* getNumberOfPerformedIterations()   (ransac_base.hpp:103)                          */
  size_t n_inliers;    /* getModelInliers().size()                                                          */
  int target_reached;  /* targetInlierCountAchieved()        (ransac_base.hpp:172)                          */
  double device_ms;    /* kernels only (hypothesis fit + scoring + re-estimation + outputs), HIP events     */
} cilhip_plane_model;
/* HyperplaneRANSACEstimator<float,3>::estimate() (model_estimation/ransac_base.hpp:64-131 with
 * ransac_hyperplane_estimator.hpp:47-55 computeResiduals and :78-85 estimate_params_).
 * samples: HOST array of 3*max_iter point indices, the random sample of every iteration in order
 *   (ransac_base.hpp:83-91), or NULL to draw them here (uniform distinct triples from `seed`; the
 *   reference seeds std::mt19937 from std::random_device, so its sequence is not reproducible either).
 * All max_iter hypotheses may be scored, but the result is the one the reference's sequential loop reaches
 * with the same samples: first strictly-better model wins, stop at the first iteration whose best inlier
 * count reaches target_inliers (clamped to n, :68).  re_estimate: PCA over the best model's inliers, then
 * residuals / inliers of the re-estimated plane (:118-128).
 * residuals_out: HOST, n floats or NULL.  inliers_out: HOST, capacity n, ascending indices, or NULL.
 * No accepted model => NaN plane, no inliers. */
int cilhip_plane_ransac3f(int device, const float* xyz, size_t n, int mem, const uint32_t* samples, uint64_t seed,
                          float max_residual, size_t target_inliers, size_t max_iter, int re_estimate,
                          cilhip_plane_model* out, float* residuals_out, uint32_t* inliers_out);
/* inlier counts (#points with absDistance <= max_residual, ransac_base.hpp:98-100) of m given planes
 * (HOST, 4*m floats: normal, offset) in one pass over the points per 128 planes.  counts_out: HOST, m. */
int cilhip_plane_score3f(int device, const float* xyz, size_t n, int mem, const float* planes, size_t m,
                         float max_residual, uint32_t* counts_out);
/* estimateModel() over ALL points (ransac_hyperplane_estimator.hpp:22-25, :70-76): PCA plane fit. */
int cilhip_plane_fit3f(int device, const float* xyz, size_t n, int mem, float plane_out[4]);

/* ---- RigidTransformRANSACEstimator3f (model_estimation/ransac_transform_estimator.hpp, SURVEY.md section 2 "next tier") ---- */
typedef struct cilhip_transform_model {
  float T[16];         /* getModel(): col-major 4x4 rigid transform mapping src onto dst (identity when nothing was estimated) */
  size_t iterations;   /* getNumberOfPerformedIterations()                                                   */
  size_t n_inliers;    /* getModelInliers().size()                                                           */
  int have_model;      /* bit 0: some hypothesis was accepted (>= sample_size inliers), bit 1: re-estimated  */
  int target_reached;  /* targetInlierCountAchieved()        (ransac_base.hpp:172)                           */
  double device_ms;    /* kernels only, HIP events                                                           */
} cilhip_transform_model;
/* TransformRANSACEstimator<RigidTransform<float,3>>::estimate() over n point PAIRS (dst_xyz[i], src_xyz[i]) -- the
 * reference's constructors gather them from a correspondence set or two index lists (ransac_transform_estimator.hpp:34-59);
 * estimateModel = estimateTransformPointToPointMetric of the sampled pairs (:75-83; registration/transform_estimation.hpp:11-48),
 * residual_i = |T * src_i - dst_i| (:90-98), loop / replay / re-estimation as ransac_base.hpp:64-131.
 * samples: HOST, 3 * max_iter pair indices (the sample of every iteration, in order) or NULL to draw them here from `seed`.
 * Defaults of the reference (:27-30): sample size 3, target ceil(n / 2), 100 iterations, max residual 0.01, re-estimate.
 * residuals_out: HOST, n floats or NULL.  inliers_out: HOST, capacity n, ascending pair indices, or NULL.
 * No accepted model and no re-estimation => identity, no inliers (the reference's model is then uninitialised). */
int cilhip_transform_ransac3f(int device, const float* dst_xyz, const float* src_xyz, size_t n, int mem, const uint32_t* samples, uint64_t seed,
                              float max_residual, size_t target_inliers, size_t max_iter, int re_estimate, cilhip_transform_model* out,
                              float* residuals_out, uint32_t* inliers_out);
/* inlier counts of m given transforms (HOST, 16 * m floats, col-major 4x4 each), one pass over the pairs per 64 transforms */
int cilhip_transform_score3f(int device, const float* dst_xyz, const float* src_xyz, size_t n, int mem, const float* transforms, size_t m,
                             float max_residual, uint32_t* counts_out);
/* estimateModel() over ALL pairs (ransac_transform_estimator.hpp:61-64): the closed-form rigid fit */
int cilhip_transform_fit3f(int device, const float* dst_xyz, const float* src_xyz, size_t n, int mem, float T_out[16]);

/* ---- next tier: k-NN (k > 1) and NormalEstimation ------------------------- */
/* KDTree<float,3,L2>::kNNSearch / kNNInRadiusSearch for a set of queries (core/kd_tree.hpp:216-256, :286-318;
 * result adaptor :63-109): the k nearest reference points of every query with d2 < max_sq_dist (strict; pass
 * INFINITY for a plain k-NN), ascending by (d2, index).  query_xyz == NULL: the reference points are the queries
 * (every point then finds itself first).  1 <= k <= 32.  All outputs are HOST arrays:
 * idx_out [n_query*k] (row per query, padded with 0xFFFFFFFF), d2_out [n_query*k] or NULL (padded with +inf),
 * counts_out [n_query] or NULL (neighbours found).  Neighbour sets, their order and the distances are the reference's bit for
 * bit -- among EXACTLY equal distances (inside a list and at its k-th place) the candidates the reference's kd-tree traversal meets
 * first, in that order (core/kd_tree.hpp:80-99 over nanoflann searchLevel): the search notices lists that hold equal distances or
 * whose k-th distance was met on a further point, builds the order tables of the reference's tree over the searched cloud
 * (csrc/tie_build.hip, on the device) the first time a call needs them, and searches again with them -- a cloud without exact ties never pays.
 * cilhip_knn_set_tie_rule (process-wide; also cilhip_normals_knn3f): 2 = that (default), 1 = tables built up front, 0 = lowest
 * index among equal distances (a brute-force argsort's order).  tests/test_gpu_parity.py: the reference's sensor frames and
 * lattices, index for index against the reference's own nanoflann knnSearch.
 * Reference points with a non-finite coordinate are in no list -- no entry at distance inf appears, also with max_sq_dist = INFINITY --,
 * such queries get count 0 and padding only ("Non-finite points" above). */
int cilhip_knn_set_tie_rule(int rule);
int cilhip_knn3f(int device, const float* ref_xyz, size_t n_ref, const float* query_xyz, size_t n_query, int mem, size_t k,
                 float max_sq_dist, uint32_t* idx_out, float* d2_out, uint32_t* counts_out);
/* KDTree<float,3>::radiusSearch (core/kd_tree.hpp:251-282; RadiusSearchResultAdaptor :111-142): per query, EVERY target
 * point with squared distance < radius_sq (strict), ascending by distance; equal distances are ordered by index (the
 * reference leaves them as std::sort does).  query_xyz == NULL: the target points are the queries.
 * offsets_out: HOST n_query + 1 -- list of query i = [offsets[i], offsets[i+1]); *total_out_or_null = offsets[n_query].
 * idx_out / d2_out: HOST `capacity` entries (d2_out may be NULL); when capacity < total (or idx_out == NULL) only the
 * offsets and the total are produced -- call again with enough room.  radius_sq must be finite.
 * Reference points with a non-finite coordinate are in no list, such queries own empty lists ("Non-finite points" above). */
int cilhip_radius_search3f(int device, const float* ref_xyz, size_t n_ref, const float* query_xyz, size_t n_query, int mem,
                           float radius_sq, uint64_t* offsets_out, uint32_t* idx_out, float* d2_out, size_t capacity,
                           size_t* total_out_or_null);
/* NormalEstimation<float,3>::estimateNormalsAndCurvatureKNN / ...KNNInRadius (core/normal_estimation.hpp:72-90,
 * :166-187 -> :362-420): per point the k-NN neighbourhood (including the point itself), mean and covariance of it
 * (core/covariance.hpp:140-170), normal = eigenvector of the smallest eigenvalue, curvature = l_min / (l0+l1+l2);
 * fewer than 3 neighbours => NaN.  view_point: 3 floats; if all finite the normal is flipped to point towards it
 * (:326-330), NULL / non-finite: sign left as the eigen-solver gives it (as in the reference).
 * normals_out: HOST 3*n, curvature_out: HOST n or NULL.  f32 per-term arithmetic, f64 accumulation and f64 Jacobi
 * eigen-solve in place of Eigen's f32 SelfAdjointEigenSolver: the mean is summed in f64 and rounded to f32, the centred
 * terms and their products are f32 (one rounding each), sums and eigen-solve f64, results rounded to f32.
 * A neighbourhood of >= 3 copies of ONE point (zero covariance): the normal is finite and unit -- (0, 0, 1), flipped by the
 * view-point rule like any other --, the curvature is 0 / 0 = NaN (as the reference's eigenvalues()[0] / eigenvalues().sum()).
 * Every row is inside the a-priori bound of DESIGN.md section 6.9 around the f64 PCA of the same list (tests/test_gpu_normals.py). */
int cilhip_normals_knn3f(int device, const float* xyz, size_t n, int mem, size_t k, float max_sq_dist, const float* view_point,
                         float* normals_out, float* curvature_out);
/* ...Radius (core/normal_estimation.hpp:120-162, RadiusNeighborhoodSpecification): every point with d2 < radius_sq
 * (strict) takes part; the neighbourhood is unbounded, its moments are accumulated without listing it. */
int cilhip_normals_radius3f(int device, const float* xyz, size_t n, int mem, float radius_sq, const float* view_point,
                            float* normals_out, float* curvature_out);
/* NormalEstimation<float, 3, MinimumCovarianceDeterminant<float, 3>>::getNormalsKNN / ...KNNInRadius (the reference's
 * examples/robust_normal_estimation.cpp; core/covariance.hpp:185-371): per point i, over the list L[0..m) that
 * cilhip_knn3f(xyz, xyz, k, max_sq_dist) returns for it under the process's tie rule, num_trials random elemental starts of 3 distinct
 * list positions, each followed by num_refinements concentration steps (rank the list by Mahalanobis distance, keep the h closest,
 * re-estimate), the trial of the smallest covariance determinant kept, then the chi-square test on the point itself.  The contract,
 * operation by operation, is DESIGN.md section 15.1; in short
 *   h = min(max(3, llroundf(inlier_ratio * (float)m)), m)  (covariance.hpp:317-319); m < 3: NaN row; m == 3 or h == m: the plain
 *       covariance of the whole list, no trials (:204, :349-352) -- with inlier_ratio 1 and chi_square_threshold <= 0 the call returns
 *       the bytes of cilhip_normals_knn3f;
 *   trial j of point i draws its start with draw_samples(seed ^ ((uint64_t)i << 8 | j), m, 3, 1, .) (a stated seed where the reference
 *       asks std::random_device: two runs give the same bytes);
 *   mean and covariance of a subset: the arithmetic of cilhip_normals_knn3f (f64 sums, f32 mean, f32 centred terms and products);
 *   ranking by q = d^T adj(C) d in f64 (det(C) times the squared Mahalanobis distance: no division, defined for the singular covariance
 *       of a 3-point start, where it orders by distance to the plane through the start), ties by list position, NaN last;
 *   a trial replaces the best iff its determinant is smaller (strict; NaN and inf never win); no winner: NaN row;
 *   inlier iff chi_square_threshold <= 0 or q_0 <= (double)chi_square_threshold * det; an outlier's normal and curvature are NaN
 *       (normal_estimation.hpp:300, :381); normal, view-point flip and curvature from the chosen covariance as cilhip_normals_knn3f.
 * mem: where xyz AND the four outputs live.  view_point: HOST, 3 floats, NULL / non-finite: no flip.  normals_out: 3*n floats;
 * curvature_or_null: n floats; subset_mask_or_null: n words, bit j set iff list position j is in the final subset (0 for a NaN row
 * that is not an outlier); inlier_or_null: n bytes, 1 = inlier.  A point with a non-finite coordinate is in no list and gets a NaN row.
 * CILHIP_ERR_INVALID, before a device is opened and with nothing written: params, xyz (n > 0) or normals_out NULL, k outside 1..32,
 * num_trials outside 1..64, num_refinements outside 0..16, inlier_ratio not finite or <= 0, chi_square_threshold NaN, n >= 2^32 - 16,
 * unknown mem.  Radius-only neighbourhoods keep no list (cilhip_normals_radius3f) and have no robust form. */
typedef struct cilhip_mcd_params {
  size_t k;                     /* list length, 1..32 */
  float max_sq_dist;            /* only neighbours with d2 < max_sq_dist (INFINITY: none left out) */
  int num_trials;               /* 1..64 */
  int num_refinements;          /* 0..16 */
  float inlier_ratio;
  float chi_square_threshold;   /* <= 0: no point is labelled an outlier */
  uint64_t seed;
} cilhip_mcd_params;
/* 6 trials, 3 refinements, ratio 0.75, threshold -1 (covariance.hpp:365-369); max_sq_dist INFINITY, k 0 (to be set), seed 0 */
void cilhip_mcd_params_default(cilhip_mcd_params* params);
int cilhip_robust_normals_knn3f(int device, const float* xyz, size_t n, int mem, const cilhip_mcd_params* params, const float* view_point,
                                float* normals_out, float* curvature_or_null, uint32_t* subset_mask_or_null, uint8_t* inlier_or_null);

/* ---- voxel-grid downsampling ---------------------------------------------------------------------------------- */
/* PointsGridDownsampler<float,3> and its siblings with normals / colours (core/grid_downsampler.hpp:8-340 over
 * core/grid_accumulator.hpp:76-199 and core/common_accumulators.hpp:36-256): what PointCloud3f::gridDownsample
 * (utilities/point_cloud.hpp:247-266) runs.  One averaged row per occupied cell of a cubic grid of edge bin_size:
 *   cell of a point: floor(p * (1.0f / bin_size)) per axis, in f32 (grid_accumulator.hpp:79, :114-123);
 *   a bin's sums: its members in ascending input index, one f32 add at a time, starting AS the first member
 *   (common_accumulators.hpp:45-46, :68-72) -- the reference's order with parallel = false, or on one thread;
 *   normals: if (dot(sum, n_i) < 0) sum -= n_i; else sum += n_i (:122-131), dot = x x' + (y y' + z z') without FMA;
 *   rows: scale = 1.0f / (float)count; scale * pointSum, scale * colorSum, normalized(scale * normalSum)
 *   (grid_downsampler.hpp:118-126); bins with fewer than min_points_in_bin members are left out (:27, :119).
 * bin_order: 1 = lexicographic in (cell_x, cell_y, cell_z), x most significant (the reference's parallel = true:
 * grid_accumulator.hpp:10-39, :180-184), 0 = first appearance, i.e. ascending lowest member index (parallel = false, :186-197).
 * A point with a non-finite coordinate belongs to no bin and is counted nowhere; non-finite normals / colours go through
 * the arithmetic as they are.  A finite point whose cell index lies outside [-2^20, 2^20) on some axis:
 * CILHIP_ERR_UNSUPPORTED.  bin_size not finite and positive, n >= 2^32, unknown mem / bin_order, NULL xyz with n > 0:
 * CILHIP_ERR_INVALID -- checked before the device is opened.  n == 0: CILHIP_OK, *n_out = 0, no device needed.
 * mem says where ALL array arguments live (inputs and outputs).  normals_or_null / rgb_or_null: optional attributes, 3 floats
 * per point; their outputs (and counts_out_or_null, members per row) are written when both the input and the output are
 * given.  Outputs hold `capacity` rows; *n_out = the number of rows.  All outputs NULL and capacity == 0: only *n_out is
 * set.  capacity < *n_out: CILHIP_ERR_INVALID, *n_out set, nothing written; capacity = n always suffices.  In every error
 * case no output array is written; cilhip_last_error(NULL) names the rule the calling thread's last call broke. */
int cilhip_grid_downsample3f(int device, const float* xyz, const float* normals_or_null, const float* rgb_or_null, size_t n, int mem,
                             float bin_size, size_t min_points_in_bin, int bin_order, float* xyz_out, float* normals_out, float* rgb_out,
                             uint32_t* counts_out_or_null, size_t capacity, size_t* n_out);

/* ---- connected-component segmentation ------------------------------------------------------------------------- */
/* ConnectedComponentExtraction<float,3>::segment with a RadiusNeighborhoodSpecification
 * (clustering/connected_component_extraction.hpp:162-265, :394-422) and the proximity evaluators of
 * core/common_pair_evaluators.hpp:84-259; labels as clustering/clustering_base.hpp:7-18.  DESIGN.md section 11 is the long form.
 *   Graph: points i != j are joined iff d2(i, j) < radius_sq (strict; d2 = ((dx*dx)+(dy*dy))+(dz*dz) in f32, the engine's pinned
 *   form) and every selected clause holds (connected_component_extraction.hpp:201-204).  Both conditions are symmetric: the
 *   result does not depend on any traversal order.
 *   Clauses (selected independently; the reference's eight evaluator classes are their combinations, AlwaysTrueEvaluator is none):
 *     use_distance: d2 < max_distance                                                        (:100, :159, :185, :243)
 *     use_colors:   |c_i - c_j|^2 < color_thresh * color_thresh (the product formed once in f32; differences in f32;
 *                   |v|^2 = x*x + (y*y + z*z), every operation rounded, no FMA)              (:136-141)
 *     use_normals:  dot = x*x' + (y*y' + z*z') (same rounding; not checked against a compiled reference, Eigen being absent where
 *                   this was written); angle = (float)acos((double)dot); max_angle >= 0: angle <| max_angle, otherwise
 *                   min(angle, (float)M_PI - angle) <| -max_angle, the subtraction in f32.  <| is <= when angle_inclusive != 0
 *                   (NormalsProximityEvaluator, :119-121) and < otherwise (every combined evaluator, :162-164, :213-215,
 *                   :247-249).  A dot product that rounds above 1 gives acos = NaN: the pair is NOT similar, as in the reference
 *                   (two identical, slightly over-long normals are not joined; nothing is clamped).
 *   Output: the connected components -- with a seed list only those that contain a seed -- each with its members in ascending
 *   index; kept iff min_segment_size <= size <= max_segment_size (:246-261: a segment past the maximum is dropped whole);
 *   ordered by size, descending, equal sizes by lowest member index ascending (the reference leaves equal sizes to std::sort; this
 *   is what a stable sort of its list gives with all seeds).  labels_out[i] = the rank of i's segment, or *n_segments_out for a
 *   point in no kept segment (clustering_base.hpp:10-11).  offsets_out_or_null[0 .. *n_segments_out] / members_out_or_null: the
 *   segments as CSR lists; members_out[offsets_out[*n_segments_out] .. n) are the unlabelled points, ascending.
 *   Deviations: the reference skips the first entry of every neighbour list, taking it for the point itself (:202); here a point
 *   is never its own neighbour and an exact duplicate always is one (identical on clouds without duplicates).  A point with a
 *   non-finite coordinate has no neighbours: a component of size 1.  A finite radius_sq <= 0: every point is a singleton.
 * mem says where xyz / normals / rgb and the three output arrays live; seeds_or_null is always a HOST array (NULL: every point
 * is a seed; non-NULL with n_seeds == 0: no segment), n_segments_out a host word.  Output sizes that always suffice: labels n,
 * offsets n + 1, members n.
 * CILHIP_ERR_INVALID, before the device is opened, nothing written, cilhip_last_error(NULL) naming the rule: a normals or
 * colours clause without its array; a seed index >= n; n >= 2^32; unknown mem; radius_sq not finite; NULL params / xyz / labels
 * / n_segments_out.  n == 0: CILHIP_OK, zero segments, no device needed. */
typedef struct cilhip_cc_params {
  float radius_sq;
  int use_distance; float max_distance;
  int use_normals; float max_angle; int angle_inclusive;
  int use_colors; float color_thresh;
  size_t min_segment_size, max_segment_size;
} cilhip_cc_params;
/* no clause, radius_sq = 0, min_segment_size = 1, max_segment_size = SIZE_MAX (:168-169) */
void cilhip_cc_default_params(cilhip_cc_params* params);
int cilhip_connected_components3f(int device, const float* xyz, const float* normals_or_null, const float* rgb_or_null, size_t n, int mem,
                                  const cilhip_cc_params* params, const uint32_t* seeds_or_null, size_t n_seeds, uint32_t* labels_out,
                                  uint32_t* offsets_out_or_null, uint32_t* members_out_or_null, size_t* n_segments_out);
/* The "given neighbours" overloads (connected_component_extraction.hpp:20-160) over CSR lists: list i is
 * idx[offsets[i] .. offsets[i + 1]) (offsets: n + 1 words, as cilhip_radius_search3f returns them; rows of cilhip_knn3f: offsets[i]
 * = i * k), n_entries the length of idx (nothing past it is read; entries >= n, the k-NN rows' padding among them, are no
 * neighbours).  keep_or_null: one byte per entry, 0 = the caller's own evaluator refused the pair.  skip_first != 0 drops entry 0
 * of every list, as :55 does.  Lists may be directed (k-NN lists are): the result is the WEAKLY connected components -- what the
 * reference computes with all seeds, where every edge either spreads a label or records a merge.  With a seed list the reference's
 * result over directed lists depends on its traversal order: symmetric == 0 together with seeds_or_null is CILHIP_ERR_UNSUPPORTED.
 * Everything after the edges (sizes, limits, order, labels, outputs, seeds, mem, errors) is shared with the entry above. */
int cilhip_connected_components_lists(int device, size_t n, const uint64_t* offsets, const uint32_t* idx, const unsigned char* keep_or_null,
                                      size_t n_entries, int skip_first, int symmetric, int mem, size_t min_segment_size, size_t max_segment_size,
                                      const uint32_t* seeds_or_null, size_t n_seeds, uint32_t* labels_out, uint32_t* offsets_out_or_null,
                                      uint32_t* members_out_or_null, size_t* n_segments_out);

/* ---- mean-shift clustering ---------------------------------------------------------------------
 * cilantro's MeanShift3f (clustering/mean_shift.hpp:38-124; float, 3-D, L2), the flow of examples/mean_shift.cpp.  DESIGN.md section 13
 * is the long form; the rules, each with the reference line it restates:
 *   1 ball      point j is in seed i's ball iff d2(seed_i, p_j) < radius_sq, strict (:60, kd_tree.hpp:251-257); d2 is the engine's pinned
 *               ((dx*dx)+(dy*dy))+(dz*dz) in f32, radius_sq = kernel_radius * kernel_radius formed once in f32 (:46).  A point with a
 *               non-finite coordinate is in no ball.
 *   2 weights   w_j = 1 (kernel_kind 0, UnityWeightEvaluator), d2_j (1, IdentityWeightEvaluator) or exp(coeff * d2_j) (2, RBFKernelWeightEvaluator,
 *               coeff = -0.5f / (sigma * sigma) in f32, the product and the exponential in the pinned f32 arithmetic of the ICP weight
 *               evaluators) -- common_pair_evaluators.hpp:13-79, mean_shift.hpp:64-66.
 *   3 step      S = sum (double)w_j * (double)p_j per axis (every product exact), W = sum (double)w_j, new = (float)(S / W) (:61-70).  The sums
 *               run in a fixed order that the input alone decides; no floating-point atomics: two runs agree bit for bit.  Deviation: the
 *               reference sums in f32 in ascending-distance order (equal distances as std::sort leaves them) and multiplies by
 *               1.0f / total_weight.
 *   4 converged a seed has converged when d2(old, new) < convergence_tol * convergence_tol (f32 product); it still takes `new` and is never
 *               examined again (:71-76).  *iterations_out counts the passes performed, the one in which the last seed converged included
 *               (:79-81); max_iter = 0 performs none: shifted = seeds.
 *   5 empty     an empty or zero-weight ball gives 0 / 0: the seed becomes (NaN, NaN, NaN) -- the reference's 0 * inf.  It never converges
 *               and finds nothing again, so once no other seed is active the remaining passes are not run and *iterations_out = max_iter,
 *               the reference's count.  A seed that comes in with a non-finite coordinate behaves so from pass 1.
 *   6 grouping  a ~ b iff d2(s_a, s_b) < cluster_tol * cluster_tol (f32 product).  Leaders: i is one iff no leader j < i has j ~ i -- the
 *               reference's serial first-fit (:84-100).  Clusters are numbered by ascending leader index (its creation order, not a size
 *               order); labels_out[i] = the lowest-numbered cluster whose leader is ~ i; a NaN seed is ~ nobody: a cluster of its own with
 *               a NaN mode.  offsets_out / members_out: the clusters as CSR lists, members in ascending index.
 *   7 modes     per cluster and axis the f64 sum of the members' shifted seeds (member k of the list in partial sum k mod 64, the 64 partials
 *               added by a fixed tree), then (float)(sum / size).  Deviation: the reference adds in f32 along the list and multiplies by the
 *               reciprocal (:102-112).
 * seeds_or_null == NULL: every point is a seed (:118-124; n_seeds is ignored).  mem says where points, seeds and the five output arrays
 * live; n_clusters_out and iterations_out are host words.  Sizes that always suffice: shifted 3 n_seeds, labels n_seeds, modes 3 n_seeds,
 * offsets n_seeds + 1, members n_seeds.  form: which shift kernel runs -- 0: the code decides from the estimated mean ball population,
 * 1: one lane per seed, 2: one wave per seed (the results of 1 and 2 differ only by the summation order of rule 3).
 * CILHIP_ERR_INVALID, before the device is opened, nothing written, cilhip_last_error(NULL) naming the rule: NULL points with n > 0; n_seeds
 * > 0 with NULL seeds; n or n_seeds >= 2^32; kernel_radius, cluster_tol or convergence_tol not finite or negative; an RBF sigma not finite
 * and positive; unknown kernel_kind, form or mem; NULL params, n_clusters_out, iterations_out, or (with at least one seed) NULL
 * shifted_seeds_out / labels_out.  No seed at all: CILHIP_OK, zero clusters, zero iterations, no device needed.  n == 0 with seeds is
 * legal: every ball is empty (rule 5).
 * Not built: double, other distance adaptors, a caller's functor as kernel evaluator, a caller-owned tree (MeanShift(const SearchTree&)
 * is "the same points"), a sharded run.  2-D and dynamic-dimension points: cilhip_mean_shift_nd below. */
typedef struct cilhip_ms_params {
  float kernel_radius; size_t max_iter; float cluster_tol; float convergence_tol;
  int kernel_kind;      /* 0 Unity, 1 Identity, 2 RBF over the squared distance */
  float kernel_sigma;   /* RBF only */
  int form;             /* 0 chosen by the code, 1 one lane per seed, 2 one wave per seed */
} cilhip_ms_params;
/* Unity kernel, convergence_tol = FLT_EPSILON (:41), kernel_sigma = 1, form 0; radius, max_iter and cluster_tol 0: the caller sets them */
void cilhip_ms_default_params(cilhip_ms_params* params);
int cilhip_mean_shift3f(int device, const float* points, size_t n, const float* seeds_or_null, size_t n_seeds, int mem, const cilhip_ms_params* params,
                        float* shifted_seeds_out, uint32_t* labels_out, float* modes_out_or_null, uint32_t* offsets_out_or_null,
                        uint32_t* members_out_or_null, size_t* n_clusters_out, size_t* iterations_out);
/* What the calling thread's last successful cilhip_mean_shift3f did (bench tool, tests): the shift form that ran, the ball population the
 * choice was made from, host wall time of the shift passes and of the grouping (each pass and round ends in a synchronisation), the
 * passes that ran (rule 5: *iterations_out can be larger) and the grouping rounds. */
typedef struct cilhip_ms_stats {
  int form_used;
  double est_ball, shift_ms, group_ms;
  size_t passes, rounds;
} cilhip_ms_stats;
int cilhip_ms_last_stats(cilhip_ms_stats* out);

/* ---- mean-shift clustering in 1 to 16 dimensions ---------------------------------------------------
 * cilantro's MeanShift2f / MeanShiftXf (clustering/mean_shift.hpp:142-164 over :38-124; float, L2).  points and seeds are point-major
 * n x dim arrays (the layout of cilhip_knn_nd).  Exhaustive: every active seed meets every point in every pass, and the grouping is a
 * quadratic scan (DESIGN.md section 22 states the cost and the worst cases).  The rules are those of cilhip_mean_shift3f with three
 * changes -- the distance (M1), the stated summation order (M3) and the absence of forms:
 *   M1 ball      point j is in seed i's ball iff d2(seed_i, p_j) < radius_sq, strict.  d2 is rule N1 of cilhip_knn_nd: nanoflann's
 *                L2_Adaptor::evalMetric in f32, in groups of four coordinates and then the tail one coordinate at a time, every operation
 *                rounded, nothing contracted (dim = 3: the 3-D entry's d2 bit for bit).  radius_sq = kernel_radius * kernel_radius, one f32
 *                product.  A point with a non-finite coordinate is in no ball: its d2 is NaN or +inf.
 *   M2 weights   rule 2 above: 1, d2_j or exp(coeff * d2_j) in the pinned f32 arithmetic.
 *   M3 step      S_a = sum (double)w_j * (double)p_ja (every product exact), W = sum (double)w_j, new_a = (float)(S_a / W).  Order: the
 *                point stream is cut into s slices of consecutive indices (s a function of n and of the number of seeds still active,
 *                evaluated once per pass); within a slice the sum ascends by point index from 0; the slices' sums are added in ascending
 *                order from 0.  No floating-point atomics: two runs agree bit for bit.  Deviation from rule 3 above: the last bit of a
 *                step may depend on how many seeds are still active, because s does; it never depends on the schedule.
 *   M4 converged d2(old, new) < convergence_tol * convergence_tol (one f32 product, strict); the seed takes `new` and is never examined
 *                again.  *iterations_out counts the passes performed; max_iter = 0 performs none: shifted = seeds bit for bit.
 *   M5 empty     an empty or zero-weight ball: the seed becomes NaN on all dim axes and is never examined again.  If the loop runs out of
 *                active seeds after any seed became NaN, *iterations_out = max_iter.  A seed that comes in with a non-finite coordinate
 *                behaves so from pass 1.
 *   M6 grouping  rule 6 above with M1's d2: a ~ b iff d2(s_a, s_b) < cluster_tol * cluster_tol (one f32 product, strict); leaders by the
 *                serial first-fit; clusters numbered by ascending leader index; labels_out[i] = the lowest-numbered cluster whose leader
 *                is ~ i; a seed with a non-finite coordinate is ~ nobody: a cluster of its own.  cluster_tol = 0: every seed is a cluster.
 *   M7 modes     rule 7 above per axis: member k of the list in partial sum k mod 64, the 64 partials added by a fixed tree, then
 *                (float)(sum / size).
 * seeds_or_null == NULL: every point is a seed (n_seeds is ignored).  mem says where points, seeds and the five output arrays live;
 * n_clusters_out and iterations_out are host words.  Sizes that always suffice: shifted dim n_seeds, labels n_seeds, modes dim n_seeds,
 * offsets n_seeds + 1, members n_seeds.  cilhip_ms_params is the 3-D entry's; form must be 0.
 * Refused before a device is opened, nothing written, cilhip_last_error(NULL) naming the rule -- CILHIP_ERR_INVALID: dim == 0; form != 0;
 * n or n_seeds >= 2^32 - 16; and everything the 3-D entry refuses (NULL points with n > 0, n_seeds > 0 with NULL seeds, a tolerance or
 * radius that is not finite or is negative, an RBF sigma not finite and positive, unknown kernel_kind or mem, NULL params,
 * n_clusters_out, iterations_out, or with at least one seed NULL shifted_seeds_out / labels_out); CILHIP_ERR_UNSUPPORTED: dim > 16.
 * No seed at all: CILHIP_OK, zero clusters, zero iterations, no device needed.  n == 0 with seeds is legal: M5 for every seed.
 * Not built: double, dim > 16, other distance adaptors, a caller's functor as kernel evaluator, a pruned search for large n, a sharded
 * run. */
int cilhip_mean_shift_nd(int device, const float* points, size_t n, size_t dim, const float* seeds_or_null, size_t n_seeds, int mem,
                         const cilhip_ms_params* params, float* shifted_seeds_out /* n_seeds*dim */, uint32_t* labels_out,
                         float* modes_out_or_null /* up to n_seeds*dim */, uint32_t* offsets_out_or_null, uint32_t* members_out_or_null,
                         size_t* n_clusters_out, size_t* iterations_out);
/* What the calling thread's last successful cilhip_mean_shift_nd did: the shift passes that ran (M5: *iterations_out can be larger), the
 * grouping rounds, the slice count of the first and of the last pass (M3), host wall time of the passes and of the grouping. */
typedef struct cilhip_msn_stats { size_t passes, rounds, slices_first, slices_last; double shift_ms, group_ms; } cilhip_msn_stats;
int cilhip_msn_last_stats(cilhip_msn_stats* out);   /* the calling thread's last successful cilhip_mean_shift_nd */

/* ---- connected-component segmentation in 1 to 16 dimensions ------------------------------------------
 * cilantro's ConnectedComponentExtraction<float, EigenDim>::segment with a RadiusNeighborhoodSpecification for EigenDim 2 and Dynamic
 * (clustering/connected_component_extraction.hpp:162-265, :394-457) and the evaluator templates of core/common_pair_evaluators.hpp:92-259.
 * points and normals are point-major n x dim arrays (the layout of cilhip_knn_nd), rgb is n x 3.  cilhip_cc_params is the 3-D entry's.
 * No neighbour list is ever written.  DESIGN.md section 23 is the long form; the rules:
 *   C1 graph      points i != j are joined iff d2(i, j) < radius_sq (strict, connected_component_extraction.hpp:201-204) and every selected
 *                 clause holds.  d2 is rule N1 of cilhip_knn_nd (groups of four coordinates, then the tail, every operation rounded, nothing
 *                 contracted; dim = 3: the 3-D entry's d2 bit for bit).  A row with a non-finite coordinate has no neighbours: its d2 is NaN
 *                 or +inf.  Finite coordinates whose d2 overflows are not joined.  radius_sq <= 0: every point is a singleton.
 *   C2 clauses    use_distance: d2 < max_distance (common_pair_evaluators.hpp:100, :159, :185, :243).  use_colors: exactly as in
 *                 cilhip_connected_components3f; colours always have 3 components (:136-141).  use_normals: dot = c_0 + (c_1 + (... +
 *                 c_{dim-1})) with c_a = n_ia * n_ja, every product and sum rounded to f32, no contraction, folded from the last axis
 *                 (dim = 3: the 3-D entry's x x' + (y y' + z z') bit for bit); angle = (float)acos((double)dot); max_angle >= 0: angle <|
 *                 max_angle, otherwise min(angle, (float)M_PI - angle) <| -max_angle; <| is <= when angle_inclusive != 0 (:119-121) and <
 *                 otherwise (:162-164, :213-215, :247-249).  A dot above 1 gives NaN: not similar.  Stated deviation: Eigen's summation
 *                 order for dynamic sizes is not restated, and nothing is checked against a compiled reference.
 *   C3 output     everything after the edges is word for word cilhip_connected_components3f's: sizes, min / max_segment_size (:246-261),
 *                 order by size descending then lowest member, labels (clustering_base.hpp:10-11), CSR lists with the unlabelled tail,
 *                 seeds_or_null (a HOST array; NULL: every point is a seed; non-NULL with n_seeds == 0: no segment), mem, and n == 0
 *                 (CILHIP_OK, zero segments) without a device.
 *   C4 repeatable a component's root is its lowest original index whatever happened in between: two runs, and forms 1 and 2, agree on every
 *                 output word.
 *   C5 refusals   before a device is opened, outputs untouched, cilhip_last_error(NULL) naming the rule -- CILHIP_ERR_INVALID: dim == 0;
 *                 form outside 0..2; n >= 2^32 - 16; and everything the 3-D entry refuses (a normals or colours clause without its array, a
 *                 seed index >= n, n_seeds > 0 with NULL seeds, unknown mem, radius_sq not finite, NULL params / points / labels_out /
 *                 n_segments_out); CILHIP_ERR_UNSUPPORTED: dim > 16.
 * form: 1 the exhaustive triangle -- every pair of points is tested once; 2 sweep and prune, exact -- rows with a non-finite coordinate are
 * set aside (singletons), the others sorted along the axis of largest finite extent (lowest axis on ties), and a tile of 256 sorted rows is
 * not tested against a tile that lies R or more before it on that axis, R the smallest f32 with fl(R * R) >= radius_sq: rounding is
 * monotone and N1 adds only non-negative rounded terms, so such a pair has d2 >= radius_sq; 0 the code decides (2 from n = 65 536 up: below
 * that the sort costs more than it saves, measured on a uniform cloud).
 * Not built: double, dim > 16, other distance adaptors, kNN neighbourhoods fused in N-D, a caller's functor (both: cilhip_knn_nd /
 * cilhip_radius_search_nd + cilhip_connected_components_lists), a sharded run. */
int cilhip_connected_components_nd(int device, const float* points, const float* normals_or_null, const float* rgb_or_null, size_t n, size_t dim,
                                   int mem, const cilhip_cc_params* params, int form, const uint32_t* seeds_or_null, size_t n_seeds,
                                   uint32_t* labels_out, uint32_t* offsets_out_or_null, uint32_t* members_out_or_null, size_t* n_segments_out);
/* What the calling thread's last successful cilhip_connected_components_nd did: the form that ran, form 2's sweep axis, the 256 x 256 tile
 * pairs of the triangle and those tested, the hook launches, host wall time of the preparation (staging, sort, plan), of the hook launches
 * and of everything after them. */
typedef struct cilhip_ccn_stats { int form_used; size_t axis, tiles_total, tiles_tested, launches; double prep_ms, hook_ms, finish_ms; } cilhip_ccn_stats;
int cilhip_ccn_last_stats(cilhip_ccn_stats* out);   /* the calling thread's last successful call */
/* No hook launch tests more than max_pairs_per_launch pairs (0: the default, 6e10 -- under a quarter of a second at the slowest measured N-D
 * pair rate); per calling thread.  For tests of the cut into launches: the result does not depend on it (C4). */
void cilhip_ccn_set_pair_cap(size_t max_pairs_per_launch);

/* ---- depth images <-> points ------------------------------------------------------------------------------------ */
/* core/image_point_cloud_conversions.hpp: DepthValueConverter / TruncatedDepthValueConverter (:7-51), the eight
 * depthImageToPoints[Normals] / RGBDImagesToPoints[Normals]Colors overloads (:53-695), pointsToDepthImage /
 * pointsColorsToRGBDImages (:697-863) and pointsToIndexMap (:865-934), for float.  DESIGN.md section 14 is the long form
 * (rules D1-D8, P1-P5); dot3(a, b) = a0 b0 + (a1 b1 + a2 b2) and the point transform (L_r0 x + (L_r1 y + L_r2 z)) + t_r are
 * the engine's pinned ones, every product and sum rounded to f32, no FMA.
 * Intrinsics K: float[9], column-major (Eigen::Matrix3f::data()).  Extrinsics: float[16], column-major rigid transform
 * (camera to world), or NULL for the identity.  mem says where ALL arrays of a call live.  Images are row-major, pixel k = y * w + x;
 * an rgb image has 3 bytes per pixel.
 * The converter: metric z = (1.0f / scale) * (float)raw, truncated: z < max_depth ? z : 0; back: raw = (RawT)(scale * z),
 * truncated: 0 unless z < max_depth.  raw_type says what the depth image holds. */
enum { CILHIP_DEPTH_U16 = 0, CILHIP_DEPTH_F32 = 1 };
typedef struct cilhip_depth_converter {
  int raw_type;     /* CILHIP_DEPTH_U16 | CILHIP_DEPTH_F32 */
  float scale;      /* raw units per metric unit (1000: millimetres) */
  int truncated;    /* 0: DepthValueConverter, 1: TruncatedDepthValueConverter */
  float max_depth;
} cilhip_depth_converter;
/* U16, scale 1, not truncated, max_depth FLT_MAX */
void cilhip_depth_default_converter(cilhip_depth_converter* conv);
/* Depth (and rgb) image -> points (, normals) (, colours).  Camera-frame point of pixel (x, y): Kinv * (z x, z y, z), Kinv the
 * inverse of K formed in f64 and rounded once.  Without normals a pixel gives a row iff its point's z is > 0; with
 * want_normals iff it is an interior pixel whose own and four neighbouring points' z are > 0 (the normal:
 * normalized(cross(P[k+w] - P[k-w], P[k+1] - P[k-1]))).  keep_invalid: all w * h rows, normals NaN where the rule gives none.
 * Rows are in ascending pixel index.  Extrinsics are applied last (points: E * P, normals: linear(E) * n).
 * colour = (1.0f / 255.0f) * (float)byte.  Outputs hold `capacity` rows, *n_out = the number of rows; all outputs NULL and
 * capacity == 0: only *n_out is set; capacity < *n_out: CILHIP_ERR_INVALID, *n_out set, nothing written; capacity = w * h always
 * suffices.  normals_out is written with want_normals, rgb_out with an rgb image.
 * CILHIP_ERR_INVALID, before the device is opened, nothing written, cilhip_last_error(NULL) naming the rule: NULL n_out / conv / K /
 * depth (w * h > 0); unknown mem or raw_type; scale not finite and positive; truncated with a NaN max_depth; w * h >= 2^32 - 16;
 * K not finite or singular; capacity > 0 with xyz_out NULL, with want_normals and normals_out NULL, or with rgb and rgb_out NULL.
 * w * h == 0: CILHIP_OK, *n_out = 0, no device needed. */
int cilhip_depth_image_to_points3f(int device, const void* depth, const unsigned char* rgb_or_null, size_t w, size_t h, int mem,
                                   const cilhip_depth_converter* conv, const float* K, const float* extrinsics_or_null, int keep_invalid,
                                   int want_normals, float* xyz_out, float* normals_out, float* rgb_out, size_t capacity, size_t* n_out);
/* Points (and colours, 3 floats per point) -> depth (and rgb) image of w x h pixels.  c = to_cam * p with to_cam the inverse of
 * the extrinsics, (R^T, -R^T t) formed in f64 and rounded once (no extrinsics: c = p).  A point takes part iff c_z > 0 and both
 * projections u = (1.0f / c_z) * dot3(K_row0, c), v likewise, are finite; its pixel is (llround(u), llround(v)) -- ties away
 * from zero -- if that lies inside the image.  raw = (RawT)(scale * c_z), truncated toward zero (U16: a product that is NaN or
 * >= 65536 skips the point); a point contributes iff raw > 0.  A pixel holds the smallest raw value that landed on it, 0 if
 * none; its rgb is (uchar)(255.0f * colour) -- truncated, saturated to [0, 255], NaN -> 0 -- of the lowest-index point among
 * those with that value.  depth_out: w * h values of conv->raw_type; rgb_out: 3 w h bytes, written when colours are given.
 * CILHIP_ERR_INVALID as above, and for n >= 2^32 - 16, NULL xyz with n > 0, NULL depth_out, colours without rgb_out.
 * w * h == 0: CILHIP_OK, no device needed; n == 0 with host arrays: the empty images, no device needed. */
int cilhip_points_to_depth_image3f(int device, const float* xyz, const float* rgb_or_null, size_t n, int mem, const float* extrinsics_or_null,
                                   const float* K, const cilhip_depth_converter* conv, size_t w, size_t h, void* depth_out,
                                   unsigned char* rgb_out_or_null);
/* Points -> index map: index_out[pixel] = the point with the smallest c_z among those that project to the pixel (projection as
 * above), equal c_z: the lowest index -- the reference's loop run serially (:889, strict <); 0xFFFFFFFF: no point. */
int cilhip_points_to_index_map3f(int device, const float* xyz, size_t n, int mem, const float* extrinsics_or_null, const float* K, size_t w,
                                 size_t h, uint32_t* index_out);

/* ---- map fusion of registered depth frames (stateless; the "Map" step of examples/fusion.cpp:147-236) ------------------------
 * A surfel model -- points, normals, colours and one confidence per point -- takes in one frame (points, normals and colours in
 * the CAMERA frame, as fromRGBDImages gives them) seen from cam_pose: model points the frame confirms are averaged with it by
 * confidence, surface the model has not seen is appended, model points in observed free space are removed.  DESIGN.md section 16
 * has the contract in full (rules F1-F9, compared bit for bit with tests/_fusion_refs.py); in short, with the rounding conventions of
 * the image conversions above (dot3, the pinned transform, no FMA, correctly rounded quotients and square roots):
 *   F1  model map = index map of model_xyz under extrinsics cam_pose (c = to_cam p, nc = linear(to_cam) n: model_t, :152, :156);
 *       frame map = index map of frame_xyz without extrinsics (:158)
 *   F2  interior pixels 1 <= x <= w - 2, 1 <= y <= h - 2 in ascending k = y w + x (:172-173; none for w < 3 or h < 3); a pixel
 *       whose frame entry is empty does nothing (:177).  f, m: the two maps' entries at the pixel
 *   F3  fz = frame_xyz[f].z, mz = c_m.z (:182-184); rw = pinned_expf(radial_factor * (dx dx + dy dy)), dx = (float)x - K02,
 *       dy = (float)y - K12 (:185-186); ang(v) = (float)acos((double)min(1.0f, max(-1.0f, v))) (std::min / std::max as written:
 *       NaN becomes -1), compared in f64 against T(deg) = ((double)deg * M_PI) / 180.0; a = ang(dot3(nc_m, frame_normals[f]))
 *   F4  the first that holds (:188-226): FUSE m exists, |mz - fz| < fusion_dist_thresh, a < T(fuse_max_angle_deg);
 *       APPEND m empty and the pixel's four neighbours in the model map empty, or m exists and a > T(append_min_angle_deg);
 *       REMOVE m exists, fz > mz + occlusion_dist_thresh, ang(-dot3(normalized(c_m), nc_m)) < T(free_space_max_angle_deg);
 *       otherwise the pixel is untouched
 *   F5  fuse (:194-203): g = rw / (rw + conf[m]), gc = 1.0f - g, q = cam_pose frame_xyz[f], nq = linear(cam_pose) frame_normals[f];
 *       point and colour per component gc old + g new, normal normalized(gc n + g nq), conf[m] += g (0 / 0 gives NaN)
 *   F6  the removed set S leaves as the reference's remove() / vec_remove do (utilities/point_cloud.hpp:154-198, fusion.cpp:8-33):
 *       n' = n - |S| (|S| >= n: the model is cleared); a row p < n' not in S stays; the k-th smallest member of S below n' receives
 *       the k-th LARGEST surviving row of [n', n)
 *   F7  then rows (q, nq, frame_rgb[f], conf = rw) are appended in ascending pixel order (:229-235)
 *   F8  *n_out = n_model - removed + appended; counts: the five populations, visited = their sum
 * The model is edited in place: its four arrays hold `capacity` rows (xyz, normals, rgb: 3 floats per row; conf: 1), the first n_model
 * are the model, after the call the first *n_out.  capacity = n_model + min(n_frame, w h) always suffices.  A capacity that is too
 * small: CILHIP_ERR_INVALID, *n_out = the size needed, and NOTHING is written to the model (every decision is made in scratch before
 * the first row changes).  mem says where all arrays live; host arrays are staged and copied back.
 * CILHIP_ERR_INVALID before the device is opened, nothing written, cilhip_last_error(NULL) naming the rule: NULL n_out, params, K or
 * cam_pose; a NULL model array with capacity > 0; a NULL frame array with n_frame > 0; n_model > capacity; n_model, n_frame or
 * w h >= 2^32 - 16; unknown mem; a non-finite K, pose or parameter; a negative threshold or angle.  w h == 0 or n_frame == 0:
 * CILHIP_OK, *n_out = n_model, no device needed. */
typedef struct cilhip_fusion_params {
  float fusion_dist_thresh;        /* 0.01   fusion.cpp:98 */
  float occlusion_dist_thresh;     /* 0.025  :99 */
  float radial_factor;             /* -0.5f / (120 * 120)  :100 */
  float fuse_max_angle_deg;        /* 75   :192 */
  float append_min_angle_deg;      /* 105  :211 */
  float free_space_max_angle_deg;  /* 45   :223 */
} cilhip_fusion_params;
void cilhip_fusion_default_params(cilhip_fusion_params* params);
typedef struct cilhip_fusion_counts { size_t visited, fused, appended, removed, untouched; } cilhip_fusion_counts;
int cilhip_fuse_frame3f(int device, float* model_xyz, float* model_normals, float* model_rgb, float* model_conf, size_t n_model, size_t capacity,
                        const float* frame_xyz, const float* frame_normals, const float* frame_rgb, size_t n_frame, int mem,
                        const float* cam_pose /* float[16] column-major, camera to world */, const float* K, size_t w, size_t h,
                        const cilhip_fusion_params* params, size_t* n_out, cilhip_fusion_counts* counts_or_null);
/* F9, cleanup_callback (fusion.cpp:51-59): S = {i : conf[i] < conf_thresh} (a NaN confidence stays) leaves by F6; in place, *n_out rows
 * remain.  CILHIP_ERR_INVALID: NULL n_out, a NULL array with n_model > 0, n_model >= 2^32 - 16, unknown mem.  n_model == 0: CILHIP_OK,
 * no device needed. */
int cilhip_fusion_remove_unstable3f(int device, float* model_xyz, float* model_normals, float* model_rgb, float* model_conf, size_t n_model, int mem,
                                    float conf_thresh, size_t* n_out);

/* ---- non-rigid registration on a sparse warp field (rigid 3-D transforms, float) ---------------------------------------------
 * estimateSparseWarpFieldCombinedMetric (registration/warp_field_estimation.hpp:1388-1846), resampleTransforms
 * (registration/warp_field_utilities.hpp:14-48), transformPoints with one transform per point, and the loop of
 * CombinedMetricSparseWarpFieldICP (icp_base.hpp:68-87 over icp_warp_field_combined_metric_sparse.hpp:202-240), the flow of
 * examples/non_rigid_icp.cpp.  DESIGN.md section 17 has the contract; in short:
 *   graph     n_ctrl control nodes; per source point a list of k_ctrl nodes and squared distances, per node a list of k_reg nodes
 *             (itself first), both in the layout cilhip_knn3f writes: idx[n * k] padded with 0xFFFFFFFF, d2[n * k].  Weights
 *             w = eval(d2): kernel 0 = Unity (1), 1 = RBF on the squared distance, pinned_expf((-0.5f / (sigma * sigma)) * d2).
 *             total_i = the weights of point i summed in list order (:1456-1465).  Row i of the regularisation lists, entries
 *             j >= 1, gives the arc (first entry, entry j) with weight sqrt(w_reg) * sqrt(eval(d2)); both directions are kept when
 *             both rows list the pair; the lower node index comes first (:1748).  A row whose first entry is padding gives no arc.
 *   unknowns  (a, b, c, t) per node, blended per source point by w / total; rotation Rz(c) Ry(b) Rx(a) (computeRotationTerms, :38-89)
 *   rows      per matched source point three point rows (w_p2p > 0) and one plane row (w_p2pl > 0) with unity correspondence
 *             weights; total_i == 0: rows of zeros (:1687-1690); per arc six sqrtHuberLoss rows (:10-36, :1750-1802)
 *   solve     per Gauss-Newton step (A^T A) delta = A^T b by Eigen's Jacobi-preconditioned conjugate_gradient() from x0 = 0, matrix
 *             free; vectors in f32, every dot product and gather accumulated in f64 in a fixed order (no floating-point atomics:
 *             two runs give the same bits); tforms += delta; converged when max over nodes |delta_node|^2 < gn_conv_tol^2 (:1819-1829)
 *   output    per node Rz(c) Ry(b) Rx(a) through rotation() (the closest rotation), translation t; 4 x 4 column-major
 *   no data   no match in nn_idx, or w_p2p <= 0 and w_p2pl <= 0: identity transforms, converged = 0, gn_iterations = 0 (:1427-1433)
 * cilhip_warp_field_create builds the graph once per (source, control graph) pair (mem: where the four list arrays live); the handle
 * also owns the solver's scratch and is used by one thread at a time.  estimate3f: src_xyz is the ALREADY WARPED source, nn_idx the
 * target index per source point (0xFFFFFFFF or any value >= n_dst: none); mem says where dst_xyz, dst_normals (may be NULL when
 * w_p2pl == 0), src_xyz, nn_idx and ctrl_transforms_out live.  resample3f: the dense field T_i = sum_j w_ij T_j / total_i through
 * rotation(), the identity where total_i == 0.  cilhip_transform_points_per_point3f: out_i = ((L0 x + L1 y) + L2 z) + t of T_i,
 * every operation rounded once.
 * CILHIP_ERR_INVALID (CILHIP_ERR_UNSUPPORTED for an unknown kernel code) before a device is touched, nothing written,
 * cilhip_last_error(NULL) naming the rule: a NULL pointer; n_src == 0 or n_ctrl == 0; k_ctrl or k_reg outside 1 .. 32;
 * n_src * k_ctrl >= 2^32 - 16 or n_ctrl * k_reg >= 2^28 - 1; a non-finite sigma, or sigma == 0 with the RBF kernel; a list index >= n_ctrl
 * that is not 0xFFFFFFFF (lists in device memory: checked after the device is opened); unknown mem; a non-finite parameter, a negative
 * weight, huber_boundary <= 0, an iteration limit >= 2^32 - 16; NULL dst_normals with w_p2pl > 0 and n_dst > 0. */
typedef struct cilhip_warp_field cilhip_warp_field;
typedef struct cilhip_warp_params {
  float w_p2p;             /* 0     icp_warp_field_combined_metric_sparse.hpp:67 */
  float w_p2pl;            /* 1     :68 */
  float w_reg;             /* 1     :69 (stiffness) */
  float huber_boundary;    /* 1e-4  warp_field_estimation.hpp:1411 */
  size_t max_gn_iter;      /* 10    :1412 */
  float gn_conv_tol;       /* 1e-5  :1413 */
  size_t max_cg_iter;      /* 1000  :1414 */
  float cg_conv_tol;       /* 1e-5  :1415 */
} cilhip_warp_params;
typedef struct cilhip_warp_stats {
  int gn_iterations, converged;
  unsigned cg_iterations_total;     /* Eigen's iterations() summed over the Gauss-Newton steps */
  float last_cg_residual_norm2;     /* |A^T b - A^T A delta|^2 of the last step's recurrence */
  float max_delta_sq;
} cilhip_warp_stats;
void cilhip_warp_default_params(cilhip_warp_params* params);
int cilhip_warp_field_create(int device, size_t n_src, size_t n_ctrl, const uint32_t* ctrl_idx, const float* ctrl_d2, size_t k_ctrl, int ctrl_kernel,
                             float ctrl_sigma, const uint32_t* reg_idx, const float* reg_d2, size_t k_reg, int reg_kernel, float reg_sigma, int mem,
                             cilhip_warp_field** out);
void cilhip_warp_field_destroy(cilhip_warp_field* field);
int cilhip_warp_field_estimate3f(cilhip_warp_field* field, const float* dst_xyz, const float* dst_normals, size_t n_dst, const float* src_xyz,
                                 const uint32_t* nn_idx, int mem, const cilhip_warp_params* params, float* ctrl_transforms_out /* n_ctrl * 16 */,
                                 cilhip_warp_stats* stats_or_null);
int cilhip_warp_field_resample3f(cilhip_warp_field* field, const float* ctrl_T /* n_ctrl * 16 */, float* dense_T_out /* n_src * 16 */, int mem);
int cilhip_transform_points_per_point3f(int device, const float* T /* n * 16 */, const float* xyz, size_t n, int mem, float* out);
/* The loop.  The context holds the target (with normals when w_p2pl > 0) and the ORIGINAL source, of the field's n_src points, on the
 * field's device.  Per iteration: the dense field warps the source on the device, the context searches the warped cloud under the identity
 * (max_sq_dist as in cilhip_find_correspondences), the estimator runs on the device-resident matches, T_ctrl[i] = T_iter[i] * T_ctrl[i],
 * the field is resampled, last_delta_norm = sqrt(max_i(|R_iter,i - I|_F^2 + |t_iter,i|^2)); stops after max_iter iterations or when
 * last_delta_norm < conv_tol.  ctrl_T0_or_null, ctrl_T_out (n_ctrl * 16) and dense_T_out_or_null (n_src * 16) are HOST arrays.  out->T
 * is the identity (a warp field has no single transform), out->last_ncorr the last search's count.  Afterwards the context's source is
 * the caller's again (restored by cilhip_set_source: optional source normals and colour features have to be set again) and it holds no
 * correspondence set.  CILHIP_ERR_INVALID: a NULL pointer, a parameter rule of above, no target or source, sizes or devices that differ,
 * w_p2pl > 0 without target normals.  CILHIP_ERR_UNSUPPORTED: a projection set on the context, a search direction other than
 * SECOND_TO_FIRST, post-filters, correspondence weight evaluators, a feature adaptor, a target shard. */
int cilhip_warp_field_icp_run(cilhip_ctx* ctx, cilhip_warp_field* field, const cilhip_warp_params* params, size_t max_iter, float conv_tol,
                              float max_sq_dist, const float* ctrl_T0_or_null, float* ctrl_T_out, float* dense_T_out_or_null, cilhip_icp_result* out);

/* ---- the same warp field with AFFINE node transforms ------------------------------------------------------------------------
 * estimateSparseWarpFieldCombinedMetric's affine overload (registration/warp_field_estimation.hpp:1859-2234; the dense estimator
 * :725-1005 is the same system on the lists ctrl_idx[i] = i, k_ctrl = 1, Unity), resampleTransforms with Mode != Isometry
 * (registration/warp_field_utilities.hpp:14-48) and the loop of SimpleCombinedMetric{Sparse,Dense}AffineWarpFieldICP3f
 * (icp_common_instances.hpp:293-294, :322-323).  Three entries on the SAME handle, with the signatures, parameters, statistics and
 * refusals (codes, and before a device is touched where the rigid ones are) of their rigid siblings above.  The graph, the weights,
 * the totals, the arcs, the CG and the no-data case are those of above; DESIGN.md section 17.4 has the contract, in short:
 *   A1 unknowns  12 per node: the 3 x 3 linear part row-major, then t (:2005-2008); the start is the identity and t = 0
 *   A2 blend     lin = sum_j w_ij L_j, tr = sum_j w_ij t_j in f32 and list order, both then MULTIPLIED by 1 / total_i (:2050-2063);
 *                total_i == 0: rows of zeros (:2068-2071).  s_t = ((L0 . s) + tr), the products summed left to right
 *   A3 rows      weight = (sqrt(w_metric) / total_i) * w_ij.  Point row eq: weight * s_t[nz] at 3 eq + nz, weight at 9 + eq, right-hand
 *                side sqrt(w_p2p) * (d - s_t)[eq] (:2084-2099).  Plane row: (weight * n[block]) * s_t[curr] at 3 block + curr,
 *                weight * n[curr] at 9 + curr, right-hand side ((n0 e0 + n1 e1) + n2 e2) * sqrt(w_p2pl), e = d - s_t (:2145-2163).
 *                OBSERVATION: the linear part's coefficients carry the TRANSFORMED point s_t, not s.  That is the reference as written,
 *                in both estimators (:2091, :2153; :881, :914): the true Jacobian at the first Gauss-Newton step (s_t == s there), not
 *                from the second on.  It is reproduced, not corrected: these entries promise the reference's iterates
 *   A4 arcs      twelve sqrtHuberLoss rows per arc, one per unknown, otherwise as above (:2169-2193)
 *   A5 step      tforms += delta; converged when max over nodes |delta_node|^2 (12 components) < gn_conv_tol^2 (:2204-2219)
 *   A6 output    the linear part and t as they are, no rotation() (:2222-2231); 4 x 4 column-major, last row 0 0 0 1
 *   A7 resample  T_i = (sum_j w_ij T_j) * (1 / total_i) in f32 and list order, not polished; the identity where total_i == 0
 *   A8 loop      cilhip_warp_field_icp_run with A6 / A7: T_ctrl[i] = T_iter[i] * T_ctrl[i] as a plain affine product,
 *                last_delta_norm = sqrt(max_i(|L_iter,i - I|_F^2 + |t_iter,i|^2))
 * The first affine estimate on a handle grows its solver scratch from 6 to 12 unknowns per node; rigid calls on the same handle give
 * the same bytes before and afterwards.  cilhip_transform_points_per_point3f serves affine transforms as it is. */
int cilhip_warp_field_estimate_affine3f(cilhip_warp_field* field, const float* dst_xyz, const float* dst_normals, size_t n_dst, const float* src_xyz,
                                        const uint32_t* nn_idx, int mem, const cilhip_warp_params* params, float* ctrl_transforms_out /* n_ctrl * 16 */,
                                        cilhip_warp_stats* stats_or_null);
int cilhip_warp_field_resample_affine3f(cilhip_warp_field* field, const float* ctrl_T /* n_ctrl * 16 */, float* dense_T_out /* n_src * 16 */, int mem);
int cilhip_warp_field_icp_run_affine(cilhip_ctx* ctx, cilhip_warp_field* field, const cilhip_warp_params* params, size_t max_iter, float conv_tol,
                                     float max_sq_dist, const float* ctrl_T0_or_null, float* ctrl_T_out, float* dense_T_out_or_null, cilhip_icp_result* out);

/* ---- introspection (bench / tests) ----------------------------------------------------------- */
typedef struct {
  int nx, ny, nz;        /* grid dims */
  float cell;            /* cell edge */
  float origin[3];
  size_t n_cells;
  double avg_occupancy;  /* sum(count^2)/n: expected own-cell candidates of a target point */
  double build_ms;       /* last set_target wall time (upload + grid build) */
} cilhip_grid_info;
int cilhip_get_grid_info(cilhip_ctx* ctx, cilhip_grid_info* out);
/* How many source points have, under T and within max_sq_dist, a nearest target point that is NOT unique in the pinned f32 squared
 * distance (exactly equidistant candidates: duplicated points, a depth sensor's lattice).  Only there do a brute-force argmin
 * (lowest target index) and the reference differ: nanoflann keeps the candidate its traversal meets first (core/kd_tree.hpp:82-90) --
 * both exact nearest neighbours; option "tie_rule" says which one the engine names.  Diagnostic (one more exact search of every query). */
int cilhip_get_tie_count(cilhip_ctx* ctx, const float T[16], float max_sq_dist, size_t* n_ties);
/* Option "tie_rule" != 0: of the last cilhip_find_correspondences (or summed over the searches of the last cilhip_icp_run / since
 * the last cilhip_icp_begin), the queries that had several exactly equidistant nearest target points, and how many of their
 * matches are NOT the lowest index (the reference's traversal met another one first). */
int cilhip_get_tie_rule_stats(cilhip_ctx* ctx, size_t* tied_queries, size_t* repointed);
/* The order tables behind "tie_rule" (kd_tree.hpp:162-170 -> nanoflann.hpp:1150-1212, :1321-1428: the permutation and the splits of
 * the index the reference builds over the target), built ON THE DEVICE (csrc/tie_build.hip: all nodes of a level are independent
 * segments -- a segmented min / max, two flagged prefix sums and two scatters per level reproduce planeSplit's two-pointer sweeps slot
 * for slot).  loaded: this context's target has them on the device; builds: how often this context built them (tie_rule 2 builds
 * when a search first meets a tie; never, on clouds that do not tie); build_ms: wall time of the last build; pending: tied queries the searches since the last
 * cilhip_icp_begin / find_correspondences met WITHOUT tables (cilhip_icp_run and cilhip_find_correspondences deal with those
 * themselves; a caller driving cilhip_icp_begin / _partial_sums / _apply_sums reads it after its loop, calls
 * cilhip_build_tie_order and runs the loop again -- cilantro_amd/distributed.py does). */
typedef struct cilhip_tie_order_info { int loaded; int builds; double build_ms; size_t pending; } cilhip_tie_order_info;
int cilhip_get_tie_order_info(cilhip_ctx* ctx, cilhip_tie_order_info* out);
/* Builds and loads the tables for this context's own target now (no-op when loaded). */
int cilhip_build_tie_order(cilhip_ctx* ctx);
/* The same tables for a target that is only PART of the cloud the reference would index (a spatial slab of a sharded run): the
 * order is a property of the WHOLE cloud.  cilhip_tie_order_create builds it once from the whole cloud (host memory, original
 * order; built on the calling thread's current HIP device -- CILHIP_ERR_NO_DEVICE without one -- and kept on the host);
 * cilhip_load_tie_order hands a context the entries of its own points: global_index[i] = index in the whole cloud of the
 * context's target point i (null: the context holds the whole cloud).  cilhip_tie_order_tables copies the tables out (tests,
 * tools: leaf and slot by original index, 16-byte node records {parent, (depth << 3) | (dimension << 1) | second child, divlow,
 * divhigh}; any pointer may be null). */
typedef struct cilhip_tie_order cilhip_tie_order;
int cilhip_tie_order_create(const float* xyz, size_t n, cilhip_tie_order** out);
void cilhip_tie_order_destroy(cilhip_tie_order* order);
int cilhip_tie_order_tables(const cilhip_tie_order* order, uint32_t* leaf_by_index, uint32_t* slot_by_index, void* nodes_out, size_t nodes_cap,
                            size_t* n_nodes, int* max_depth);
int cilhip_load_tie_order(cilhip_ctx* ctx, const cilhip_tie_order* order, const uint32_t* global_index);

/* CorrespondenceSearchCombinedMetricCombiner (registration/correspondence_search_combined_metric_combiner.hpp:8-81): the combined
 * metric's point-to-point terms read ONE engine's correspondence set, its point-to-plane terms ANOTHER's (own radius, feature
 * adaptors, post-filters) over the same two clouds.  Both contexts hold the same target / source and SECOND_TO_FIRST matches
 * found under the same transform (cilhip_find_correspondences on each); ctx_point == ctx_plane is the single-engine case.
 * cilhip_estimate_combined_two_sets = estimateTransformCombinedMetric with its two set arguments
 * (registration/transform_estimation.hpp:237-367); cilhip_icp_run_two_sets = the ICP loop of
 * icp_single_transform_combined_metric.hpp:169-217 with that engine (host-driven: both searches, the estimate, compose, test). */
int cilhip_estimate_combined_two_sets(cilhip_ctx* ctx_point, cilhip_ctx* ctx_plane, float w_p2p, float w_p2pl, size_t max_iter, float conv_tol,
                                      float dT[16], int* converged);
int cilhip_icp_run_two_sets(cilhip_ctx* ctx_point, float max_sq_point, cilhip_ctx* ctx_plane, float max_sq_plane, const cilhip_icp_params* p,
                            const float* T0, cilhip_icp_result* out);

/* ---- one process, several devices (devices[], one stream per device) ---------------------------------------
 * The sharded ICP loop driven from C: one context per entry of devices[], per iteration every context enqueues its partial
 * sums, the 48 f64 are all-reduced on the devices' streams by RCCL (ncclAllReduce; librccl is opened at run time, only when
 * ndev > 1) and every context applies them -- the reference has no counterpart; the loop is
 * IterativeClosestPointBase::estimate (registration/icp_base.hpp:68-87).  devices[] may repeat ONE ordinal (several shards on one
 * GPU, reduced by a kernel: what a single-GPU box can test).
 * cilhip_multi_set_clouds copies the host clouds (they are cut again when a slab guard fires) and uploads every shard:
 * partition 0 = the source in contiguous shards, the whole target on every device; 1 = spatial slabs along the longest axis of the
 * target's bounding box, target slabs with a halo of sqrt(max_sq_dist) + slack (slack = 2 sqrt(max_sq_dist)), source points by the
 * slab their image under T_part (null: identity; cilhip_multi_icp_run re-cuts under its T0) falls into, the device-side guard
 * armed (cilhip_set_slab_guard) and handled inside cilhip_multi_icp_run: all shards re-partitioned under the last exact
 * transform, no exact iteration discarded; 2 = the TARGET in contiguous index shards, the whole source on every device (SURVEY.md 8(e)
 * partitioning A: for a target that does not fit one device): per iteration an all-reduce(MIN) of one packed (d2, global index) key
 * per source point (ncclUint64 / ncclMin over RCCL), every shard accumulates the pairs it won, then the all-reduce of the sums; when
 * the searches meet exactly equidistant nearest points (inside a shard or across shards) the whole target's tie order is built once
 * and the run repeated with a second MIN per iteration (cilhip_icp_order_keys): the reference's matches, index for index.
 * Engine options are set per shard through cilhip_multi_context(rank). */
typedef struct cilhip_multi cilhip_multi;
int cilhip_multi_create(cilhip_multi** out, const int* devices, int ndev);
void cilhip_multi_destroy(cilhip_multi* m);
const char* cilhip_multi_last_error(const cilhip_multi* m);
cilhip_ctx* cilhip_multi_context(cilhip_multi* m, int rank);
int cilhip_multi_set_clouds(cilhip_multi* m, const float* dst_xyz, const float* dst_nrm_or_null, size_t n_dst, const float* src_xyz, size_t n_src,
                            float max_sq_dist, int partition, const float* T_part_or_null);
int cilhip_multi_icp_run(cilhip_multi* m, const cilhip_icp_params* p, const float* T0, int check_every, cilhip_icp_result* out);
/* Host time the shards' enqueue calls took per iteration of the last cilhip_multi_icp_run (the slowest shard's thread: the run has one
 * host thread per shard; CILHIP_MULTI_THREADS=0 in the environment: one thread walks the shards, and the figure is the mean per shard). */
int cilhip_multi_last_host_time(const cilhip_multi* m, double* us_per_iteration_per_shard);
int cilhip_multi_repartitions(const cilhip_multi* m);
/* how far a source point may move along the slab axis before the slabs are cut again (the halos are the search radius + this);
 * < 0: the default, twice the search radius.  Takes effect at the next cilhip_multi_set_clouds. */
int cilhip_multi_set_slab_slack(cilhip_multi* m, float slack);
int cilhip_multi_shard_sizes(const cilhip_multi* m, int rank, size_t* n_target, size_t* n_source);

/* ---- one process PER device (torchrun, MPI): this context as one rank of an RCCL communicator -------------------------------
 * The sharded loop's inner triple (cilhip_icp_partial_sums, all-reduce of the 48 f64, cilhip_icp_apply_sums) for `iterations`
 * iterations inside one call, the all-reduce = ncclAllReduce on the context's stream (librccl opened at run time): per iteration
 * the host enqueues a handful of launches instead of three foreign-function calls and a framework collective.  Rank 0 creates
 * the id (cilhip_rank_comm_unique_id), the launcher carries its 128 bytes to every rank (torch.distributed.broadcast, MPI_Bcast,
 * a file), every rank calls cilhip_rank_comm_init(ctx, id, nranks, rank) -- collective, as ncclCommInitRank is.  Between
 * cilhip_icp_begin and cilhip_icp_state the caller alternates cilhip_icp_iterate_ranked(k) with whatever it checks every k
 * iterations (convergence, cilhip_get_slab_violation_state).  Every rank must ask for the same number of iterations.  The
 * reference has no counterpart; the loop is IterativeClosestPointBase::estimate (registration/icp_base.hpp:68-87). */
int cilhip_rank_comm_unique_id(unsigned char id_out[128]);
/* What cilhip_rank_comm_init can fail at on one rank alone (opening librccl, its buffer), beforehand: the ranks agree -- one MIN over the
 * launcher's channel -- before any of them enters the collective init (cilantro_amd/distributed.py init_rank_comm). */
int cilhip_rank_comm_prepare(cilhip_ctx* ctx);
int cilhip_rank_comm_init(cilhip_ctx* ctx, const unsigned char id[128], int nranks, int rank);
int cilhip_rank_comm_destroy(cilhip_ctx* ctx);
int cilhip_icp_iterate_ranked(cilhip_ctx* ctx, int iterations);
/* With kernel timing on (cilhip_enable_kernel_timing; sampled by option "kernel_timing_stride"): the time of the ranked loop's
 * ncclAllReduce ON THE STREAM -- hipEvents around the collective: launch of RCCL's kernel, the exchange over xGMI, the wait for the
 * slowest rank -- summed over the `timed` iterations since cilhip_icp_begin; valid after cilhip_icp_state.  (No reference
 * counterpart: what bench.py --gpus N reports as allreduce_us_per_iteration.) */
int cilhip_get_last_allreduce_timing(cilhip_ctx* ctx, double* total_ms, int* timed);
/* Host time the ranked loop's enqueue calls took per iteration since cilhip_icp_begin -- launches and the collective's enqueue, the
 * paced waits for the device's feedback word (the host stays at most two iterations ahead) excluded: what must stay below a rank's
 * iteration time for the host to be off the critical path (bench.py: host_enqueue_us_per_iteration_per_rank). */
int cilhip_get_last_host_enqueue_time(cilhip_ctx* ctx, double* us_per_iteration);

/* How the iterations of the last cilhip_icp_run were executed: as ONE pass (search with the accumulation inside the LDS
 * tiles) or as TWO (search with its in-tile 3x3x3 second pass, then the streaming accumulation).  Large clouds choose per
 * iteration from the device's count of queries the first search stage left unproven (source far from alignment: two passes).
 * Sharded runs: the same two counts over the cilhip_icp_partial_sums calls since cilhip_icp_begin. */
int cilhip_get_last_run_forms(cilhip_ctx* ctx, int* one_pass_iterations, int* two_pass_iterations);
/* ... and how many of the one-pass iterations ran as the WARM-STARTED per-lane kernel (option "warm_start"): from the second
 * iteration on, near alignment, the search starts from the previous iteration's match -- a real target point, so its
 * distance from the new query bounds the search -- and usually ends inside the query's own cell; same matches. */
int cilhip_get_last_warm_iterations(cilhip_ctx* ctx, int* warm_iterations);
/* The device-resident FIRST_TO_SECOND / BOTH loops (no post-filter, no correspondence weight evaluators): how many iterations of the
 * last cilhip_icp_run took their sums from the warm-started reverse search itself (option "reverse_warm_start": every iteration but the
 * first) instead of from a separate pass over the reverse matches.  0 after any other loop.  Counted on the host. */
int cilhip_get_last_reverse_fused_iterations(cilhip_ctx* ctx, int* fused_iterations);
/* The last cilhip_icp_run iteration by iteration (at most the first 256, at most `cap`; written by the device's epilogue, read
 * back here): queries the search's first stage left unproven, queries a warm-started iteration had to search, the bound on
 * how far any source point moved in the iteration's update (what the warm-started form's margins are spent on), the update
 * norm (last_delta_norm_ of icp_base.hpp:83) and the kernel form (the codes of cilhip_get_last_form_timing).  Any output
 * array may be null.  Diagnostics: nothing in the loop depends on it. */
int cilhip_get_last_run_trace(cilhip_ctx* ctx, int cap, int* n, unsigned int* unproven, unsigned int* listed, float* step, float* delta, int* form);
/* With kernel timing on: kernel time (hipEvents on the ctx stream) and launch count of the last run's iterations per FORM of
 * their search kernel -- 0: search alone (a streaming accumulation follows: cilhip_get_last_timing2), 1: LDS-tiled search with
 * the accumulation inside the tile, 2: the first warm-started iteration of a stretch (gathers through the stored matches and
 * writes the match records), 3: warm-started iterations reading the records, 4: the per-lane fused kernel (option "fused"). */
int cilhip_get_last_form_timing(cilhip_ctx* ctx, int form, double* kernel_ms, int* launches);
/* ... and iteration by iteration: which iterations of the last cilhip_icp_run carried events (option "kernel_timing_stride") and the time
 * of the search (+ accumulation) kernel(s) of each.  *n = how many (may exceed cap: the first cap are written). */
int cilhip_get_last_iteration_timing(cilhip_ctx* ctx, int cap, int* n, unsigned int* iteration, float* kernel_ms);

/* ms of the kernels of the last cilhip_icp_run, measured with hipEvents on the ctx stream:
 * total loop, and the fused search+accumulate kernel alone (sum over executed iterations). */
int cilhip_get_last_timing(cilhip_ctx* ctx, double* loop_ms, double* search_kernel_ms,
                           int* search_kernel_launches);
/* Record a hipEvent pair around every fused search+accumulate launch of cilhip_icp_run (off by
 * default: the extra event records perturb a back-to-back loop slightly). */
int cilhip_enable_kernel_timing(cilhip_ctx* ctx, int on);
/* Tuning knobs (never change results beyond f64 summation order):
 *   "fused" (default 0): 1 = one fused search+accumulate kernel per iteration,
 *                        0 = search kernel (stores the matches) + streaming accumulation kernel.
 *   "tiled" (default 1): LDS-tiled search kernel (one workgroup stages the cell region around an
 *                        12x12x12-cell cube of queries in LDS; tiles that do not fit fall back per tile):
 *                        0 = never (per-lane global-memory search), 1 = when the cloud is large enough
 *                        to fill the chip with tiles (>= 600 tiles, ~1M points), full enough tiles and a
 *                        target density that fits a tile's LDS budget, 2 = always.
 *   "tile_accumulation" (default 1): where the first Gauss-Newton step of an iteration is accumulated when the tiled search runs
 *                        without post-filters: 0 = always in a separate streaming pass, 1 = inside the LDS tiles (one pass per
 *                        iteration) unless the device reports the source far from alignment, 2 = always inside the tiles.
 *   "warm_start" (default 1): the warm-started iteration kernel (cilhip_get_last_warm_iterations): 0 = never, 1 = once the last
 *                        update moved no source point by more than "warm_enter_fraction" of a grid cell (and for as long as the
 *                        kernel settles most queries from their margins: it reports how many it had to search), 2 = from the
 *                        second iteration on.
 *   "warm_forecast" (default 1): the cold iterations of a run count the queries whose margin the next update is expected to spend
 *                        (or that leave without one); the warm-started form is entered only when that is at most an eighth of the
 *                        queries -- a pair whose matches lie far beyond the target's point spacing never pays for a try.  0 = enter
 *                        on the step alone (tests).
 *   "tie_rule" (default 2): which of several EXACTLY equidistant nearest target points a correspondence names.  The reference's
 *                        kd-tree search returns the candidate its traversal meets FIRST (core/kd_tree.hpp:82-90 over nanoflann
 *                        1.7.1 searchLevel), which depends on the tree it built (leaf size 10, core/kd_tree.hpp:162-170).
 *                        2 = that point, on the device, in every kernel form: each search notices when its smallest distance was
 *                        met on a second point and settles such a query from the order tables of the reference's tree (per point:
 *                        leaf + slot of the reference's permutation; per node: parent, depth, split -- csrc/tie_build.hip builds
 *                        them on the device, level by level, csrc/search_device.hpp tie_settle reads them).  The tables are built when a search first
 *                        MEETS a tie (that search / run is then executed once more): a target whose searches never tie never pays
 *                        for a tree, one that does pays once.  1 = the same choice, tables built before the first search.
 *                        0 = the lowest index (what a brute-force argmin gives).  Covers every search over point features:
 *                        SECOND_TO_FIRST, rigid and affine, sharded runs included (cilhip_load_tie_order; index shards of a target:
 *                        cilhip_icp_order_keys), and the reverse matches of FIRST_TO_SECOND / BOTH -- there the reference's tree is
 *                        over the TRANSFORMED SOURCE, a new one per search (correspondence_search_kd_tree.hpp:185-222): a reverse
 *                        search counts the target points with several exactly equidistant source points; when they are
 *                        systematic (at least 16 and one target point in 100 000: duplicated points, lattices; under 1: always,
 *                        from the start) that tree's tables are built (on the device) before every reverse search (2 ms for a
 *                        110k-point cloud, 25 ms at 10M points) and the loops run one search at a time -- for this source, until it is set
 *                        again (duplicated points and lattices tie under every transform / systematically).  Below that (the coincidence of
 *                        two f32 distances in a large random cloud: about one target point in ten million) rule 2 keeps the
 *                        lowest source index for those and reports them (cilhip_get_tie_rule_stats).  The 6-D / 9-D feature adaptors
 *                        (SECOND_TO_FIRST) follow the tree the reference builds over the target's FEATURES (DIM = 6 / 9: other
 *                        splits, other leaves; tables per feature weights, rebuilt when those change; tie_before_nd); their
 *                        reverse searches keep the lowest index (refused under 1).  tests/test_gpu_tie_rule.py: every
 *                        index of the reference's sensor frames, of clouds with doubled and tripled points and of lattices with
 *                        8-way ties equals nanoflann's, in every direction.
 *   "group_search" (default -1): the global-memory search with SEVERAL lanes per query (small clouds, sources far from alignment: one
 *                        lane per query leaves the chip idle behind chains of dependent trips -- the reference's 120k-point sensor
 *                        frames: 0.34 -> 0.12 ms per iteration).  G adjacent lanes share a query: the rows of the block around its
 *                        cell are dealt to them, each row clipped to the cells the ball of the best distance so far reaches, the
 *                        minimum key goes round the group, the previous iteration's match bounds the search.  Same keys, same tie
 *                        rule, same results.  -1 = the ICP loop decides per iteration (clouds the tiles do not take: always below
 *                        the warm-started form's floor of 65 536 points; above it while the cold kernels' forecast says most
 *                        queries are far from settled); 0 = never; 4, 8, 16, 32, 64 = that many lanes in every such search.
 *   "fused_epilogue" (default 0): 1 = the stage-1 reduction of the partial sums and the epilogue run as ONE launch (the block that takes
 *                        the last ticket of the 32 stage-1 blocks runs the epilogue behind a device-scope fence).  Bitwise the same
 *                        results; measured slower than the two launches on this eight-L2 part (0.129 -> 0.136 ms per iteration at
 *                        10M, 0.037 -> 0.044 at 1M: NOTEBOOK.md) -- kept for A/B runs.
 *   "warm_extra_fraction" (default 0.0625): a query the warm-started form has to search is searched inside the ball of its bound
 *                        plus this fraction of a grid cell -- the room its fresh margin can have.  Larger: more cells per
 *                        search, margins that last longer; measured best at 10M (independent source: 0.25 -> 0.216 ms per
 *                        warm-started iteration, 0.0625 -> 0.197, 0.03 -> 0.199).  Never changes a result.
 *   "kernel_timing_stride" (default 1): with kernel timing on (cilhip_enable_kernel_timing), iterations 0, 1, 2 and every stride-th one
 *                        carry events; the others run as they do without timing.  An event between two dependent kernels idles the
 *                        device for ~6 us: two per iteration are a tenth of a warm-started iteration at 10M.  The per-form averages
 *                        of cilhip_get_last_form_timing are then over the timed launches (its `launches` = how many).
 *   "pair_records" (default 1): the streaming accumulation (second pass of a two-pass iteration, later Gauss-Newton steps) gathers a
 *                        match's point and normal from ONE 32-byte record instead of two arrays (a copy of the target in that layout,
 *                        32 B per point, built by the first run that needs it; without room for it the two arrays serve): 123.5 ->
 *                        113.5 us at 10M.  0 = the two arrays (A/B).  Same values, same sums.
 *   "tile_records" (default 1): the accumulating tile kernel writes the match records of the warm-started form itself (from a
 *                        run's second iteration on), so that the next iteration can read them; 0 = the first warm-started
 *                        iteration of a stretch gathers through the stored matches and writes them (A/B).
 *   "warm_enter_fraction" (default 0.15): that bar, as a fraction of a grid cell (halved each time a warm-started iteration of
 *                        the run had to search more than a quarter of its queries).
 *                        Neither option changes a result beyond the order of f64 additions.
 *   "refined_occupancy_factor" (default 3): a target whose density-based first guess of the cell size leaves far too many points per
 *                        cell (a surface, clusters: most cells of its bounding box are empty) has its grid refined until the expected
 *                        own-cell population is at most 3 x cell_occupancy x this factor.  1 = as fine a grid as a volumetric cloud
 *                        gets.  A search that has to leave the first block of cells walks shells of mostly empty cells on such a cloud,
 *                        and pays per cell: measured on the reference's sensor frames (120k points), frame_1 vs frame_2 (residuals of
 *                        several cells) 0.67 ms per iteration at factor 1, 0.30 at 3, 0.25 at 5; the near-aligned pair 0.033 / 0.036 /
 *                        0.045.  Used by the next cilhip_set_target; never changes a result.
 *   "cell_occupancy" (default 1): target points per grid cell, used by the next cilhip_set_target.
 *   "kernel_timing": same as cilhip_enable_kernel_timing.
 * Engine post-filters (correspondence_search_kd_tree.hpp:224-225, setInlierFraction / setOneToOne :253-271):
 *   "inlier_fraction" (default 1): in (0,1) keeps the llround(f*n) correspondences of smallest value
 *                        (core/correspondence.hpp:57-66; equal values: lowest source index first),
 *   "one_to_one" (default 0): 1 keeps, per target point, the correspondence of smallest value (:84-95).
 *   Applied to cilhip_find_correspondences and inside cilhip_icp_run; not available in sharded runs.
 * Search direction (correspondence_search_kd_tree.hpp:185-222, setSearchDirection / setRequireReciprocality :239-263):
 *   "search_direction" (default 0): 0 = SECOND_TO_FIRST (source points look for their nearest target point),
 *                        1 = FIRST_TO_SECOND (every target point looks for its nearest TRANSFORMED source point; like the
 *                        reference, an index over the transformed source is rebuilt for every search), 2 = BOTH (the
 *                        union of the two sets in (indexInFirst, indexInSecond) order, kd_tree_utilities.hpp:65-101),
 *   "require_reciprocality" (default 0): with BOTH, the intersection instead of the union.
 *   With 1 / 2 the correspondence set is a pair list (up to n_target + n_source entries): read it with
 *   cilhip_get_correspondences (cilhip_get_nn does not apply); the post-filters follow the reference's branches for
 *   those directions (one-to-one: per source point for FIRST_TO_SECOND, a no-op for BOTH, correspondence.hpp:72-98);
 *   cilhip_icp_run accumulates over the pair list.  Not available in sharded runs.
 *   "reverse_warm_start" (default 1): the device-resident loops of those directions (rigid start transform, no post-filters, plain
 *                        point features) start every reverse search but the first from the previous iteration's reverse matches: a
 *                        target point whose old match T s_i is nearer than half the distance from T s_i to its nearest other
 *                        transformed source point (a table over the source, built once) keeps it without looking at a cell; the rest
 *                        is searched as before -- the exact argmin either way (bidir.hip k_reverse_warm).  0 = every search from
 *                        scratch, for A/B runs.
 * Feature adaptor of the engine (correspondence_search/common_transformable_feature_adaptors.hpp):
 *   "feature_normal_weight" (default 0 = PointFeaturesAdaptor3f, :8-57): w > 0 = PointNormalFeaturesAdaptor3f (:60-161)
 *                        on both clouds -- features (p, w n), transformed as (T p, L (w n)), matched by the 6-D squared
 *                        distance (which is then also what max_sq_dist, the filters and the returned values refer to).
 *                        Needs target normals and source normals (cilhip_set_source_normals).  Every search direction; under
 *                        "transform_mode" = 1 the normal part follows the adaptor's non-rigid branch (:112-124):
 *                        normal_weight * (L^-T (w n)).normalized(), normal_weight = |w n_0| of the first source point.
 *                        Unsharded runs.
 *   "feature_kind" (default 0): 1 = the 6-D features are point + COLOUR, PointColorFeaturesAdaptor (:164-252): (p, w c) with
 *                        the colour part untouched by the transform; colours through cilhip_set_color_features, weight through
 *                        "feature_normal_weight".  2 = the 9-D point + NORMAL + COLOUR features, PointNormalColorFeaturesAdaptor
 *                        (:255-343): (p, wn n, wc c), matched by the 9-D squared distance (nanoflann's DIM = 9 summation order);
 *                        the normal part follows the transform as for kind 0, the colour part does not move; wn through
 *                        "feature_normal_weight", wc through "feature_color_weight"; needs both clouds' normals and colours.
 *   "feature_color_weight" (default 0): the colour weight of feature_kind 2.
 *   "feature_warm_start" (default 1): SECOND_TO_FIRST loops over features (rigid classes, no post-filters, >= 400 000 source points):
 *                        once an update moves no source point by more than the warm-started form's entry fraction of a cell, the
 *                        search starts from the previous matches -- a query whose old match p has 4 d_feat(q, p) < nnd(p)^2 (nnd: the
 *                        distance from p to its nearest other target point; d_feat >= the squared point distance) keeps it without looking
 *                        at a cell, the rest is searched in full (feat_warm.hip) -- and goes back to the tile search when more than a
 *                        quarter of the queries had to be searched.  With the three-cloud metric and unity evaluators the same pass also
 *                        accumulates the step's sums.  Same correspondences either way; 0 = every search from scratch (A/B).
 *   "symmetric_metric" (default 1): 0 = source normals feed the feature adaptor only and the combined metric stays the
 *                        three-cloud one (the reference decides this by the ICP constructor used,
 *                        icp_common_instances.hpp:74-97).  The symmetric objective runs the plain loop's kernel forms, the
 *                        warm-started one included (the queries' source normals streamed with them); the accumulating tiles and the
 *                        sharded building blocks keep the streaming pass for it.
 * Transform family (registration/icp_common_instances.hpp:253-267):
 *   "transform_mode" (default 0): 0 = rigid -- cilhip_icp_run is Simple{PointToPoint,Combined}MetricRigidICP3f;
 *                        1 = affine -- Simple{PointToPoint,Combined}MetricAffineICP3f: same loop and correspondence engine,
 *                        the step is cilhip_estimate_affine's closed form and there is no rotation() polish
 *                        (icp_single_transform_combined_metric.hpp:207-216); max_opt_iter / opt_conv_tol are unused,
 *                        as in the reference's affine overload.  Not available in sharded runs.
 *   "affine_device_loop" (default 1): the affine classes' loop runs device-resident like the rigid one whenever nothing needs the
 *                        stored correspondence set per iteration (SECOND_TO_FIRST, no post-filters, unity evaluators, point features):
 *                        search-only kernels + ONE streaming pass of the 112 moments on the matrix cores while the source is far from
 *                        alignment, search + moments in the warm-started kernel afterwards, the pivoted 12x12 LDL^T, the un-centring and
 *                        the f32 compose in the epilogue kernel -- no host round trip per iteration.  0 = the host-driven loop (three
 *                        moment passes + a host solve per iteration: what the other configurations run), for A/B runs.
 * Correspondence weight evaluators of the combined-metric classes (the PointToPoint/PointToPlaneCorrWeightEvaluatorT
 * template arguments of registration/icp_single_transform_combined_metric.hpp:11-14, core/common_pair_evaluators.hpp):
 *   "point_weight_evaluator", "plane_weight_evaluator" (default 0): 0 = UnityWeightEvaluator (:30-43),
 *                        1 = IdentityWeightEvaluator (:14-27: the weight is the correspondence's value, i.e. the squared
 *                        search distance -- 6-D with the point+normal features), 2 = RBFKernelWeightEvaluator over squared
 *                        distances (:46-80): exp(-0.5 / sigma^2 * value).
 *   "point_weight_sigma", "plane_weight_sigma" (default 1): the RBF evaluators' sigma (setSigma, :55-58).
 *                        The per-pair f32 weight is metric weight * evaluator(value) as transform_estimation.hpp:301-303,
 *                        :330-332 form it; exp() is a pinned f32 sequence (within 1 ulp of the correctly rounded value; the
 *                        reference's std::exp depends on its libm).  Rigid classes only (cilhip_icp_run, the sharded
 *                        building blocks, cilhip_estimate_combined); the accumulation then always runs as its own
 *                        streaming pass. */
int cilhip_set_option(cilhip_ctx* ctx, const char* key, double value);
/* The same options as a typed table: an enum a C caller can check at compile time, and per option its key, default, admissible
 * range and one line of documentation (the long form is the comment above).  cilhip_option_info(id) is valid for
 * 0 <= id < cilhip_option_count() == CILHIP_OPT_COUNT, in the enum's order (NULL otherwise); cilhip_set_option_id is
 * cilhip_set_option by id; cilhip_get_option reads the current value back.  cilhip_set_option refuses (CILHIP_ERR_INVALID) a value
 * outside [min_value, max_value] of its row.  tests/test_capi_symbols.py walks the table: every option is documented, accepted
 * with its default, readable, refused outside its range, and named by at least one test. */
typedef enum cilhip_option {
  CILHIP_OPT_FUSED = 0, CILHIP_OPT_INLIER_FRACTION, CILHIP_OPT_ONE_TO_ONE, CILHIP_OPT_TILED, CILHIP_OPT_WARM_START, CILHIP_OPT_WARM_FORECAST,
  CILHIP_OPT_FUSED_EPILOGUE, CILHIP_OPT_GROUP_SEARCH, CILHIP_OPT_TIE_RULE, CILHIP_OPT_WARM_EXTRA_FRACTION, CILHIP_OPT_PAIR_RECORDS,
  CILHIP_OPT_TILE_RECORDS, CILHIP_OPT_WARM_ENTER_FRACTION, CILHIP_OPT_POINT_WEIGHT_EVALUATOR, CILHIP_OPT_PLANE_WEIGHT_EVALUATOR,
  CILHIP_OPT_POINT_WEIGHT_SIGMA, CILHIP_OPT_PLANE_WEIGHT_SIGMA, CILHIP_OPT_TILE_ACCUMULATION, CILHIP_OPT_SEARCH_DIRECTION,
  CILHIP_OPT_FEATURE_NORMAL_WEIGHT, CILHIP_OPT_FEATURE_KIND, CILHIP_OPT_FEATURE_COLOR_WEIGHT, CILHIP_OPT_SYMMETRIC_METRIC,
  CILHIP_OPT_TRANSFORM_MODE, CILHIP_OPT_REQUIRE_RECIPROCALITY, CILHIP_OPT_CELL_OCCUPANCY, CILHIP_OPT_REFINED_OCCUPANCY_FACTOR,
  CILHIP_OPT_KERNEL_TIMING, CILHIP_OPT_KERNEL_TIMING_STRIDE, CILHIP_OPT_REVERSE_WARM_START, CILHIP_OPT_FEATURE_WARM_START, CILHIP_OPT_AFFINE_DEVICE_LOOP,
  CILHIP_OPT_COUNT
} cilhip_option;
typedef struct cilhip_option_info_t {
  int id;                 /* enum cilhip_option */
  const char* key;        /* the name cilhip_set_option takes */
  double default_value, min_value, max_value;
  const char* doc;
} cilhip_option_info_t;
int cilhip_option_count(void);
const cilhip_option_info_t* cilhip_option_info(int id);
int cilhip_set_option_id(cilhip_ctx* ctx, cilhip_option id, double value);
int cilhip_get_option(cilhip_ctx* ctx, const char* key, double* value);
/* With "fused"=0 and kernel timing on: ms spent in the search kernels and in the accumulation
 * kernels of the last cilhip_icp_run (sum over executed iterations).  Sharded runs: the same two sums over the
 * cilhip_icp_partial_sums calls since cilhip_icp_begin, available after cilhip_icp_state (which synchronises);
 * cilhip_get_last_timing then reports the number of those calls as the launch count. */
int cilhip_get_last_timing2(cilhip_ctx* ctx, double* search_ms, double* accumulate_ms);
/* Tiled search bookkeeping of the most recent search launch: out[0] = queries, out[1] = whole tiles that were
 * handed to the global-memory clean-up pass (syncs). */
int cilhip_debug_counters(cilhip_ctx* ctx, uint32_t out[2]);
/* Stateless: out[0] = device allocations the library holds in this process right now (all contexts, handles and calls in flight),
 * out[1] = their bytes.  Every allocation and free of the library goes through one pair of functions that keeps the two counts, so
 * "nothing leaked" can be checked exactly, without reading the device's free memory (which other processes move). */
int cilhip_debug_live_allocations(unsigned long long out[2]);

/* ---- spectral clustering: sparse affinities, Laplacian embedding, k-means in D dimensions ---------------------------------------- */
/* clustering/spectral_clustering.hpp (computeLaplacianSpectralEmbedding, sparse input, :191-312; SpectralClustering :398-416) with
 * utilities/nearest_neighbor_graph_utilities.hpp:63-118 in front of it and KMeans<float, Dynamic> (kmeans.hpp:67-194) behind it, for
 * float.  DESIGN.md section 18 is the long form; tests/_spectral_refs.py restates every rule in numpy.
 *   S1 graph     a neighbour list (of cilhip_knn3f: idx[n*k] padded with 0xFFFFFFFF and d2[n*k], offsets == NULL, k_or_total = k; or CSR
 *                lists as cilhip_radius_search3f returns them: offsets[n + 1], idx, d2, k_or_total = offsets[n]) becomes the sparse matrix
 *                of getNNGraphFunctionValueSparseMatrix (:89-118).  Entry e of point i's list with neighbour j = idx[e] (the first entry, the
 *                point itself, is KEPT, as in the reference) gives val = 1 (kernel_kind 0), d2[e] (1) or exp(coeff * d2[e]) (2, coeff =
 *                -0.5f / (sigma * sigma), the pinned f32 arithmetic of cilhip_ms_params) and M(j, i) = val; with force_symmetry also M(i, j)
 *                = val.  duplicates = 0: values that fall on one (row, column) are SUMMED (setFromTriplets: a mutual pair carries 2 val and
 *                the self entry 2 val; the sum runs in the order (i, e) of the contributing list entries, which for two terms is order-free).
 *                duplicates = 1: the dense variant's rule (:63-87), assignment -- the contribution with the largest (i, e) stays.  The build
 *                runs on the device (count, scan, fill, per-row sort, merge) with integer atomics only: the result does not depend on
 *                scheduling.  The matrix: CSR, columns strictly ascending per row, f32 values, uint64 offsets.
 *                CILHIP_ERR_INVALID (cilhip_last_error(NULL) names the rule, *out untouched): NULL idx or out; NULL d2 unless kernel_kind is 0;
 *                n == 0 or n >= 2^32 - 16; k == 0 or n * k >= 2^32 in the k-NN layout; unknown kernel_kind, mem or duplicates; an RBF sigma
 *                not finite and positive; and, found on the device, an index >= n that is not the padding, offsets that are not ascending or
 *                whose last entry is not k_or_total.
 *   S2 operator  W is taken as symmetric (the caller's promise, as in the reference).  d_i = the f64 sum of row i in column order
 *                (deviation: the reference sums in f32).  laplacian_type 0 UNNORMALIZED: A = D - W, spectrum in [0, 2 max d]; 1
 *                NORMALIZED_SYMMETRIC: A = I - D^-1/2 W D^-1/2, spectrum in [0, 2]; 2 NORMALIZED_RANDOM_WALK: (D - W) v = lambda D v with
 *                v^T D v = 1 (:276-309), computed as the symmetric form's u with v = D^-1/2 u.  A degree that is not finite and positive
 *                under a normalised type: CILHIP_ERR_INVALID.  Solver storage and arithmetic are f64, the matrix stays f32; there is no
 *                floating-point atomic anywhere.
 *   S3 sizes     max_num_clusters == 0 or >= n: 2 clusters, estimation off (:406-412).  nev = estimate ? min(max + 1, n - 1) : max
 *                (:198-200).  max_num_clusters > 16: CILHIP_ERR_UNSUPPORTED.  n < 3: CILHIP_ERR_INVALID.
 *   S4 solver    Chebyshev-filtered subspace iteration on a block of b = min(nev + max(guard, nev / 2), n) columns, guard = 3: a start block
 *                from a counter-based hash of (row, column), then per outer iteration a Rayleigh-Ritz step (Ritz values theta ascending)
 *                and, unless every one of the first nev Ritz pairs passes Spectra's test (3rd_party/Spectra/HermEigsBase.h:152-167 with the
 *                float literals of spectral_clustering.hpp:202) on its TRUE residual in f64,
 *                    ||A x - theta x||_2 < 1e-7f * max(pow(FLT_EPSILON, 2/3), |theta|)      (x of unit length),
 *                a filter of degree `degree` (24) that damps [largest Ritz value of the block, the upper bound of S2], scaled at the lowest
 *                Ritz value by the three-term recurrence, and CholQR2.  After max_outer (1000) iterations without acceptance the call still
 *                returns CILHIP_OK, with n_converged < num_eigenvalues in the result (the reference doubles max_iter for ever).
 *   S5 output    eigenvalues rounded to f32, negative ones set to 0 (:225-228); with estimation num_clusters =
 *                estimateNumberOfClustersEigengap (:46-68, literally, f32 on the rounded values); the embedding is the first num_clusters
 *                vectors, point-major n x num_clusters f32 (the reference's column-major dim x n); NORMALIZED_SYMMETRIC divides each point's
 *                vector by its f32 norm (ascending f32 sum of squares, sqrtf) when 1 / norm is finite (:269-272).  Addition: each vector's
 *                sign makes its largest-magnitude component (f64, before the type's scaling; lowest index among equals) positive.  Two runs
 *                agree bit for bit; vectors inside a repeated eigenvalue's space are whatever the iteration gives.
 *   S6 k-means   cilhip_kmeans_nd: cilhip_kmeans3f's rules (brute-force branch, the empty-cluster repair with its quirk) in 1 <= dim <= 16
 *                dimensions, k <= 256.  Distance: the f32 sum ((d0 d0 + d1 d1) + d2 d2) + ... in ascending coordinate order, no FMA;
 *                assignment: strict '<' over ascending cluster index; cluster sums: f64, the points in chunks of ceil(n / min(256,
 *                ceil(n / 256))) consecutive indices, ascending inside a chunk, the chunks' partial sums added in ascending order; centroid
 *                = (float)(sum / count) (deviation: the reference sums in f32).  centroids: HOST dim * k floats, in and out; mem: where x
 *                and labels_out live.
 * embedded_out: n * num_clusters floats where `mem` says (room for n * max_num_clusters always suffices); eigenvalues_out: HOST, nev floats
 * (room for max_num_clusters + 1).  Not built: double, 2-D and dense-input device paths, the kd-tree branch of the D-dimensional k-means,
 * a sharded run, a check of W's symmetry. */
typedef struct cilhip_sparse cilhip_sparse;
int cilhip_nn_graph_matrix(int device, size_t n, const uint64_t* offsets_or_null, const uint32_t* idx, const float* d2, size_t k_or_total, int mem,
                           int kernel_kind, float kernel_sigma, int force_symmetry, int duplicates, cilhip_sparse** out);
/* a caller's CSR matrix (n x n; mem: where the three arrays live).  CILHIP_ERR_INVALID: a NULL array, n == 0 or >= 2^32 - 16, offsets[0] != 0
 * or descending, columns of a row not strictly ascending (unsorted or duplicate), a column >= n, a value that is not finite. */
int cilhip_sparse_from_csr(int device, size_t n, const uint64_t* offsets, const uint32_t* columns, const float* values, int mem, cilhip_sparse** out);
/* any of the three may be NULL */
int cilhip_sparse_info(const cilhip_sparse* m, size_t* n_out, size_t* nnz_out, size_t* longest_row_out);
/* copy-out: offsets n + 1, columns nnz, values nnz, each where `mem` says, each optional */
int cilhip_sparse_get(const cilhip_sparse* m, uint64_t* offsets_out, uint32_t* columns_out, float* values_out, int mem);
void cilhip_sparse_destroy(cilhip_sparse* m);

typedef struct cilhip_spectral_params {
  size_t max_num_clusters;
  int estimate_num_clusters;
  int laplacian_type;      /* 0 UNNORMALIZED, 1 NORMALIZED_SYMMETRIC, 2 NORMALIZED_RANDOM_WALK */
  size_t max_outer;        /* S4: outer iterations before the call gives up */
  int degree;              /* S4: degree of the filter, 2 .. 512 */
  int guard;               /* S4: guard columns, 1 .. 15 */
} cilhip_spectral_params;
typedef struct cilhip_spectral_result {
  size_t num_clusters, num_eigenvalues, n_converged, outer_iterations, block_products;
  double max_residual;     /* the largest true residual among the first num_eigenvalues Ritz pairs at the end */
  double wall_ms;
} cilhip_spectral_result;
/* max_num_clusters 2, no estimation, NORMALIZED_RANDOM_WALK (:401), max_outer 1000, degree 24, guard 3 */
void cilhip_spectral_default_params(cilhip_spectral_params* params);
int cilhip_spectral_embedding(const cilhip_sparse* W, const cilhip_spectral_params* params, float* embedded_out, float* eigenvalues_out, int mem,
                              cilhip_spectral_result* result);
int cilhip_kmeans_nd(int device, const float* x, size_t n, size_t dim, int mem, float* centroids, size_t k, size_t max_iter, float tol,
                     uint32_t* labels_out, size_t* iterations_out);

/* ---- multidimensional scaling and principal component analysis ------------------------------------------------------------------------ */
/* utilities/multidimensional_scaling.hpp (computeDistancePreservingSpectralEmbedding :34-83, MultidimensionalScaling :86-120) for float: the
 * classical (Torgerson) embedding of n points from their n x n distance matrix.  DESIGN.md section 19 is the long form;
 * tests/_mds_refs.py restates every rule in numpy.
 *   M1 input     D: n x n f32, row-major, leading dimension n, where `mem` says.  Symmetry is the caller's promise, as in the reference;
 *                whether D or its transpose is applied is unspecified (the reference's column-major matrix is the same bytes).
 *                distances_are_squared == 0: Dhat_ij = d * d as one f32 product (array().square() in ScalarT, :57); otherwise Dhat = D.
 *                CILHIP_ERR_INVALID (cilhip_last_error(NULL) names the rule, the outputs untouched): a NULL pointer; n < 3 or n >= 2^32 - 16;
 *                unknown mem; degree outside [1, 512], guard outside [1, 15], max_outer == 0; and, found on the device in the pass that
 *                forms the column means, an entry of Dhat that is not finite.  Argument errors are refused before any device call.
 *   M2 operator  B = -1/2 J Dhat J, J = I - 1 1^T / n, is applied in f64 and never formed: with r_i the mean of column i of Dhat and g the
 *                mean of r, (B x)_i = -1/2 (sum_j Dhat_ji x_j - r_i sum_j x_j - sum_j r_j x_j + g sum_j x_j).  The sum over j runs in
 *                chunks of max(128, ceil(n / 64)) consecutive rows, ascending inside a chunk, the chunks' sums added in ascending order; the
 *                two moments of x (sum_j x_j, sum_j r_j x_j) in the fixed two-stage shape of S4's residual sums (DESIGN.md 19.1 spells it
 *                out); g: ascending i on the host.  The order depends on n and the block width alone.  No floating-point atomic.
 *   M3 sizes     max_dim == 0 or >= n: dimension 2, estimation off (:110-118).  nev = estimate ? min(max_dim + 1, n - 1) : max_dim (:41-42).
 *                max_dim > 16: CILHIP_ERR_UNSUPPORTED.
 *   M4 solver    the nev eigenpairs of LARGEST MAGNITUDE, ordered by descending |theta| (Spectra's LargestMagn for selection and sort,
 *                :65-66), each accepted by Spectra's test (3rd_party/Spectra/HermEigsBase.h:152-167 with the float literal of :44) on its
 *                TRUE residual in f64,
 *                    ||B x - theta x||_2 < 1e-7f * max(pow(FLT_EPSILON, 2/3), |theta|)      (x of unit length).
 *                Subspace iteration on a block of b = min(nev + max(guard, nev / 2), n) columns from S4's start block: per outer iteration
 *                a Rayleigh-Ritz step on the unlocked columns (Ritz pairs by descending magnitude), locking of the leading pairs that pass
 *                the test, and on the rest a filter that damps [-e, e] (e: the smallest magnitude of the block) and is 1 at the first
 *                unlocked magnitude, of a degree <= `degree` (24) chosen so that its gain stays within 1e6 down to the lowest wanted
 *                magnitude and within 1e10 up to the largest locked one; then two projections against the locked vectors and CholQR2.
 *                After max_outer (1000) iterations without acceptance the call still returns CILHIP_OK, with n_converged < num_eigenvalues
 *                (the reference doubles max_iter for ever).  That is what a request for a pair inside the rounding noise of exactly
 *                low-rank data gets (estimate_dim with max_dim >= the rank).
 *   M5 output    eigenvalues rounded to f32, negative ones set to 0 in place (:70-73: the order stays the magnitude order); with estimation
 *                dim = estimateEmbeddingDimensionEigengap (:10-31, literally, f32 on the clamped values); the embedding is point-major
 *                n x dim f32 (the reference's column-major dim x n), sqrtf(ev[c]) * (float)(sign_c * x_ic) (:79-80).  Addition: sign_c makes
 *                the largest-magnitude component of the f64 vector positive (lowest index among equals).  Two runs agree bit for bit;
 *                vectors inside a repeated eigenvalue's space are whatever the iteration gives.
 * embedded_out: n * dim floats where `mem` says (room for n * max_dim -- n * 2 when M3 falls back -- always suffices); eigenvalues_out: HOST,
 * nev floats (room for max_dim + 1).  Not built: double, a sharded run, a check of D's symmetry. */
typedef struct cilhip_mds_params {
  size_t max_dim;
  int estimate_dim;
  int distances_are_squared;
  size_t max_outer;        /* M4: outer iterations before the call gives up */
  int degree;              /* M4: largest degree of the filter, 1 .. 512 */
  int guard;               /* M4: guard columns, 1 .. 15 */
} cilhip_mds_params;
typedef struct cilhip_mds_result {
  size_t dim, num_eigenvalues, n_converged, outer_iterations, block_products, locked;
  double max_residual;     /* the largest true residual among the num_eigenvalues Ritz pairs at the end */
  double wall_ms;
} cilhip_mds_result;
/* max_dim 2, no estimation, squared distances (:97, :109), max_outer 1000, degree 24, guard 3 */
void cilhip_mds_default_params(cilhip_mds_params* params);
int cilhip_mds_embedding(int device, const float* D, size_t n, int mem, const cilhip_mds_params* params, float* embedded_out, float* eigenvalues_out,
                         cilhip_mds_result* result);
/* The operator of M2 alone: y = B x for a row-major n x b f64 block (1 <= b <= 32; x and y_out where `mem` says, like D), in the order M2
 * states.  product_ms_out (optional): device time of the product itself, without the pass that forms the column means. */
int cilhip_mds_apply(int device, const float* D, size_t n, int mem, int distances_are_squared, const double* x, size_t b, double* y_out, double* product_ms_out);

/* core/principal_component_analysis.hpp with core/covariance.hpp:31-180 for float.  x: n points of `dim` coordinates, point-major (the
 * reference's column-major dim x n), 1 <= dim <= 16, where `mem` says; subset_or_null: n_subset uint32 indices into x (the subset
 * constructor; where `mem` says), an index >= n is found on the device: CILHIP_ERR_INVALID.  count = n_subset, or n without a subset.
 *   P1 mean        f64 coordinate sums -- the sample in chunks of ceil(count / min(256, ceil(count / 64))) consecutive entries, ascending
 *                  inside a chunk, the chunks' sums added in ascending order -- and mean = (float)(sum / count) (deviation: the reference
 *                  sums in f32, covariance.hpp:64-68).
 *   P2 covariance  tmp = x - mean in f32 (:73); the products tmp_a tmp_c and their sums in f64, the same order; cov = (float)(sum / (count - 1)).
 *   P3 small       count < 2 (min_sample_size_, :35-39): mean, covariance, eigenvalues and eigenvectors are all NaN, *valid_out = 0, CILHIP_OK.
 *   P4 eigen       cyclic Jacobi in f64 on the f32 covariance, eigenvalues descending (principal_component_analysis.hpp:76-84), outputs f32.
 *                  eigenvectors_out[c * dim + k]: component k of vector c (the reference's column-major matrix).  Addition: vectors
 *                  0 .. dim - 2 get M5's sign rule, the last one the sign that makes the determinant positive (:79-82).
 *   P5 maps        project: out[i][t] = (float) sum_k V[t][k] * (x[i][k] - mean[k]), t < target_dim <= dim (:46-49): the difference in f32,
 *                  products and the ascending sum in f64.  reconstruct: out[i][k] = (float)(sum_{t < source_dim} V[t][k] y[i][t] + mean[k])
 *                  in f64 (:59-62).  target_dim / source_dim outside [1, dim]: CILHIP_ERR_INVALID.  mean and eigenvectors: HOST.
 * mean_out dim, cov_out dim * dim (row-major), eigenvalues_out dim, eigenvectors_out dim * dim: HOST. */
int cilhip_pca_fit(int device, const float* x, size_t n, size_t dim, const uint32_t* subset_or_null, size_t n_subset, int mem, float* mean_out, float* cov_out,
                   float* eigenvalues_out, float* eigenvectors_out, int* valid_out);
int cilhip_pca_project(int device, const float* x, size_t m, size_t dim, int mem, const float* mean, const float* eigenvectors, size_t target_dim, float* out);
int cilhip_pca_reconstruct(int device, const float* y, size_t m, size_t source_dim, size_t dim, int mem, const float* mean, const float* eigenvectors, float* out);

/* spatial/convex_polytope.hpp, convex_hull_utilities.hpp:570-740 (convexHullFromPoints) for float in 2 and 3 dimensions.
 * Qhull is not ported: the device finds the extreme points among n (filter and refine), a plain-C++ builder orders them (csrc/hull_host.hpp).
 * points: n rows of `dim` floats where `mem` says.
 *   H1 arithmetic  every plane is f64 on the f32 coordinates: nrm = normalise((b - a) x (c - a)), off = -nrm . a (2-D: the edge's outward
 *                  normal); d(p) = nrm . p + off, positive outside.
 *   H2 band        tol = max(merge_tol, 2^-44 M), M the largest finite |coordinate|.  Outside iff d > tol.  Points within the band of the
 *                  boundary (face interiors, edges, duplicates of a vertex) are not vertices; of exact duplicates the lowest index is.
 *   H3 input       non-finite rows are ignored and counted.  Fewer than dim + 1 finite points, or no simplex of height > tol
 *                  (convex_hull_utilities.hpp:582-628): the reference's empty polytope -- is_empty, no vertices, no facets, the two
 *                  placeholder halfspaces (1, 0, .., 1) and (-1, 0, .., 1), area = volume = 0, a NaN interior point -- and CILHIP_OK.
 *   H4 order       vertex_point_indices ascend; vertices are those rows, copied.  A facet lists vertex-list indices counter-clockwise seen
 *                  from outside, its smallest first (2-D: the edge (v0, v1) with the interior on its left, as it is); facets are sorted
 *                  lexicographically.  Triangles whose opposite vertices lie within tol of each other's plane merge into their boundary
 *                  polygon; simplicial_facets = 1 lists each polygon as the fan (v0, vi, vi+1) from its smallest vertex.  Halfspace k is
 *                  (nrm, off) of facet k rounded to f32 (a polygon: of its fan triangle with the smallest sorted index triple), so
 *                  nrm . x + off <= 0 inside (convex_polytope.hpp:109-115).  facet_neighbors[j] of facet k: the facet across the edge
 *                  (v_j, v_j+1 mod m) (2-D: the other edge at v_j).  vertex_facets ascend.  interior_point: the f32 mean of the vertices,
 *                  summed in order (:238).  area / volume (f64, Qhull's meaning: perimeter / enclosed area in 2-D): the facets' areas, the
 *                  signed simplex volumes from the interior point, both summed in facet order.
 *   H5 repeatable  every array and `info` agree bit for bit between two runs.
 * Refused with CILHIP_ERR_INVALID before a device is opened (cilhip_last_error(NULL) names the rule): a NULL points / out / info, dim outside
 * {2, 3}, n >= 2^32 - 16, an unknown mem, a negative or non-finite merge_tol.  n == 0: the empty polytope, no device needed.
 * Not built (CILHIP_ERR_UNSUPPORTED where a call could ask): the halfspace constructor's vertex enumeration, intersectionWith,
 * SpaceRegion::complement / relativeComplement / getVolume (they need the QP of convex_hull_utilities.hpp:12-193 and a dual hull), double,
 * dimension above 3, hulls of lower-dimensional input beyond FlatConvexHull3f. */
typedef struct cilhip_hull cilhip_hull;
typedef struct cilhip_hull_info {
  int dim, is_empty;
  size_t n_vertices, n_facets, n_facet_indices, n_vertex_facets;
  size_t n_halfspaces;                 /* n_facets, or the 2 placeholders of the empty polytope */
  double area, volume;
  float interior_point[3];
  size_t rounds;                       /* cull launches */
  size_t n_nonfinite;
  size_t survivors_first_round;        /* points still outside the seed hull after the first cull */
  unsigned long long plane_tests;      /* sum over the rounds of survivors x facets */
  size_t facet_tile;                   /* facets per LDS tile of the cull kernel */
  double cull_ms;                      /* device time of the cull kernels by events; 0 unless CILHIP_HULL_TIMING=1 is set (see below) */
} cilhip_hull_info;
int cilhip_convex_hull_create(int device, const float* points, size_t n, size_t dim, int mem, int simplicial_facets, double merge_tol, cilhip_hull** out,
                              cilhip_hull_info* info);
/* HOST arrays, any NULL one is skipped: vertex_point_indices n_vertices; vertices n_vertices x dim; halfspaces n_halfspaces columns of dim + 1
 * (column k contiguous); facet_offsets n_facets + 1; facet_indices and facet_neighbors n_facet_indices; vertex_facet_offsets n_vertices + 1;
 * vertex_facets n_vertex_facets; survivors_per_round `rounds` entries. */
int cilhip_convex_hull_get(const cilhip_hull* hull, uint32_t* vertex_point_indices, float* vertices, float* halfspaces, uint32_t* facet_offsets, uint32_t* facet_indices,
                           uint32_t* facet_neighbors, uint32_t* vertex_facet_offsets, uint32_t* vertex_facets, uint64_t* survivors_per_round);
void cilhip_convex_hull_destroy(cilhip_hull* hull);
/* CILHIP_HULL_TIMING=1 in the environment makes create() time its cull kernels with device events (info.cull_ms; 0 otherwise). */

/* Containment (convex_polytope.hpp:109-141, space_region.hpp:208-234).  halfspaces: HOST, the polytopes' columns of dim + 1 floats one after
 * the other; poly_offsets: HOST, n_polytopes + 1 column offsets ascending from 0.  points (n rows of dim floats) and the output where `mem` says.
 *   Q1  v = ((h0 x + h1 y) + h2 z) + h3 in f32, left to right, no contraction (2-D: (h0 x + h1 y) + h2)
 *   Q2  inside a polytope iff no column has v > -offset (a point leaves at its first failing column); inside the region iff inside any
 *       polytope.  No columns: contains everything.  The empty polytope's placeholders contain nothing.
 * signed_distances: out[k * n + i] = v of column k at point i.  interior_mask: n bytes, 0 / 1.  interior_indices: ascending indices; *n_out
 * (HOST) always gets the count; capacity == 0 only counts; a capacity below the count is CILHIP_ERR_INVALID and writes nothing
 * (the rules of cilhip_grid_downsample3f).  n == 0 needs no device.  Refused: NULL arrays, dim outside {2, 3}, n >= 2^32 - 16, an unknown
 * mem, poly_offsets that do not ascend from 0, a NaN offset. */
int cilhip_polytope_signed_distances(int device, const float* halfspaces, size_t n_facets, const float* points, size_t n, size_t dim, int mem, float* out);
int cilhip_polytopes_interior_mask(int device, const float* halfspaces, const uint32_t* poly_offsets, size_t n_polytopes, const float* points, size_t n, size_t dim, int mem,
                                   float offset, uint8_t* mask_out);
int cilhip_polytopes_interior_indices(int device, const float* halfspaces, const uint32_t* poly_offsets, size_t n_polytopes, const float* points, size_t n, size_t dim, int mem,
                                      float offset, uint32_t* indices_out, size_t capacity, size_t* n_out);

/* ---- exact neighbour search in 1 to 16 dimensions ------------------------------------------------------------------------------------- */
/* KDTree<float, EigenDim, L2> for EigenDim != 3 (core/kd_tree.hpp:144-406: KDTree2f, KDTreeXf): kNNSearch, kNNInRadiusSearch and
 * radiusSearch over n x dim float points, exhaustively (csrc/knn_nd.hip).  DESIGN.md section 21 is the long form.
 * ref / query_or_null: point-major n x dim floats (the layout of cilhip_kmeans_nd), where `mem` says; query_or_null == NULL: the reference
 * points are the queries (n_query is ignored; every finite point finds itself first, at distance 0).  The outputs are HOST arrays with the
 * shapes, padding (0xFFFFFFFF / +inf), NULL rules (d2_out, counts_out, total_out_or_null may be NULL) and the two-call capacity protocol of
 * cilhip_knn3f and cilhip_radius_search3f.
 *   N1 distance    nanoflann's L2_Adaptor::evalMetric (nanoflann.hpp:570-604) in f32, every operation rounded, nothing contracted: with
 *                  s_i = (q_i - p_i)^2, r = 0; for each full group of four coordinates r = r + (((s_d + s_d+1) + s_d+2) + s_d+3); for the
 *                  0 to 3 coordinates left over, one at a time, r = r + s_d.  dim = 3: the d2 of cilhip_knn3f bit for bit; dim = 6:
 *                  (g0 + s4) + s5, never g0 + (s4 + s5).
 *   N2 acceptance  a candidate enters iff d2 < max_sq_dist (strict; INFINITY: plain k-NN) and d2 is finite: a reference row with a
 *                  non-finite coordinate is in no list, nor is a candidate whose finite coordinates overflow d2 to +inf; a non-finite
 *                  query gets count 0 (an empty list).
 *   N3 order       lists ascend by (d2, index); among exactly equal distances the lowest reference index wins, inside a list and at its
 *                  k-th place (cilhip_knn3f under tie rule 0).  cilhip_knn_set_tie_rule does not apply.  A stated deviation: the
 *                  reference's KDTreeXf names whichever equal candidate its traversal meets first.
 *   N4 sizes       1 <= dim <= 16, 1 <= k <= 32 (k > n_ref: padded rows); n_ref, n_query < 2^32 - 16; the radius lists hold at most
 *                  2^32 - 16 entries together (else CILHIP_ERR_UNSUPPORTED, as in 3-D).  CILHIP_ERR_UNSUPPORTED: dim > 16, k > 32.
 *                  CILHIP_ERR_INVALID: ref NULL with n_ref > 0, idx_out NULL (k-NN), offsets_out NULL (radius), dim == 0, k == 0, a NaN
 *                  max_sq_dist, a radius_sq that is not finite, an unknown mem, a size at or above 2^32 - 16.  All of these are refused
 *                  before a device is opened and leave the outputs untouched; cilhip_last_error(NULL) names the rule.  n_ref == 0,
 *                  n_query == 0 or a bound <= 0: empty lists / count 0, no device needed.
 *   N5 radius      every reference point with d2 < radius_sq, ascending by (d2, index); radius_sq <= 0: empty lists.
 *   N6 repeatable  two runs agree bit for bit. */
int cilhip_knn_nd(int device, const float* ref, size_t n_ref, const float* query_or_null, size_t n_query, size_t dim, int mem, size_t k, float max_sq_dist,
                  uint32_t* idx_out, float* d2_out, uint32_t* counts_out);
int cilhip_radius_search_nd(int device, const float* ref, size_t n_ref, const float* query_or_null, size_t n_query, size_t dim, int mem, float radius_sq,
                            uint64_t* offsets_out, uint32_t* idx_out, float* d2_out, size_t capacity, size_t* total_out_or_null);

#ifdef __cplusplus
}
#endif
#endif

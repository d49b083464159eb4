// ctx_options.hpp -- the options of a context, each written ONCE: the fields a context keeps them in (struct CtxOptions, a base of
// cilhip_ctx), and one table row per option (enum cilhip_option in c_api.h) with its id, key, default, admissible range, one line of
// documentation, how the current value reads back, how a value is stored, and what of the context's state the new value makes stale.
// cilhip_set_option (c_api.hip) checks a value against the row's range, hands it to the row and applies what the row reports
// (ctx.hpp: apply_stale); a fresh CtxOptions holds every row's default because the rows stored it.  Plain C++17, no HIP: compiled by
// hipcc for the library and swept by tests/cpp/test_ctx_options.cpp on the host.  Long-form documentation: c_api.h above cilhip_set_option.
#pragma once

#include "../../include/cilantro_hip/c_api.h"

#include <type_traits>

namespace cilhip {

// (no initialisers: the defaults are the table's default_value column, stored by the constructor)
struct CtxOptions {
  CtxOptions();
  int warm_start{};               // option "warm_start": 0 = never, 1 = when the device reports the source near alignment, 2 = from the second iteration on
  int tiled{};                    // 0: per-lane global-memory search; 1: LDS-tiled search when the cloud is large enough; 2: always tiled
  bool warm_forecast{};           // option "warm_forecast": the cold kernels' count of the queries a warm-started iteration would have to search gates the form
  // option "tie_rule": which of several EXACTLY equidistant nearest target points a correspondence names.  0 = the lowest target index;
  // 1 = the one the reference's kd-tree traversal meets first, order tables built before the first search; 2 (default) = the same
  // choice, the tables built when a search first MEETS a tie (that search / run is then executed again): a target that never ties never
  // pays for a tree.  The device resolves ties inside its search kernels (TieDev, kernels.hip: tie_settle).
  int tie_rule{};
  // option "group_search": the global-memory search with SEVERAL lanes per query (k_search_group: small clouds and sources far from
  // alignment, where one lane per query leaves the chip idle behind chains of dependent trips).  -1 (default) = the ICP loop decides per
  // iteration (cold iterations of clouds the tiles do not take: always for clouds below the warm-started form's floor, from the
  // kernels' own forecast above it); 0 = never; 4 .. 64 = that many lanes in every global-memory search.
  int group_lanes{};
  bool feat_warm{};               // option "feature_warm_start": the feature adaptors' forward search warm-started from the previous matches once the loop moves little (feat_warm.hip)
  bool affine_device_loop{};      // option "affine_device_loop": the affine classes' loop device-resident (one-pass moments on the matrix cores, 12-unknown
                                  // solve in the epilogue kernel) whenever nothing needs the stored set per iteration; 0 = the host-driven loop (A/B)
  bool fused_epilogue{};          // option "fused_epilogue": stage-1 reduction + epilogue in ONE launch (the last of the 32 stage-1 blocks runs the
                                  // epilogue).  Bitwise the same results, measured SLOWER: 0.129 -> 0.136 ms per iteration at 10M, 0.037 -> 0.044 at 1M --
                                  // a device-scope fence costs more on this eight-L2 part than the kernel boundary it removes (NOTEBOOK.md): off
  float warm_extra{};             // option "warm_extra_fraction"
  bool pair_records{};            // option "pair_records": the streaming accumulation gathers a match's point and normal from one 32-byte record (GridDev::pn)
  bool tile_records{};            // option "tile_records": the accumulating tile kernel writes the warm-started form's match records itself
  float warm_enter{};             // option "warm_enter_fraction": the bar a run starts with, as a fraction of a grid cell
  int cw_point_kind{}, cw_plane_kind{};          // correspondence weight evaluators (CW_*), combined metric
  float cw_point_sigma{}, cw_plane_sigma{};
  bool tile_acc_adaptive{};       // choose one pass / two passes per iteration from the device's feedback (option "tile_accumulation" = 2: always one pass)
  bool tile_acc{};                // accumulate inside the LDS tiles of the search when the engine allows it (option "tile_accumulation", A/B)
  bool fused{};                   // true: search+accumulate in one kernel; false: search kernel + streaming accumulate kernel (faster: the search runs at 2x the occupancy)
  double cell_occupancy{};        // target points per grid cell (takes effect at the next set_target)
  double refined_occupancy{};     // option "refined_occupancy_factor": how much denser than that a REFINED grid (surface-like / clustered target) may stay
  // engine post-filters (correspondence_search_kd_tree.hpp:224-225)
  double inlier_fraction{};
  bool one_to_one{};
  // other search directions (correspondence_search_kd_tree.hpp:185-222): the correspondence set is a pair list
  int search_dir{};               // 0 = SECOND_TO_FIRST (default), 1 = FIRST_TO_SECOND, 2 = BOTH
  bool reciprocal{};              // require_reciprocality_ (BOTH only)
  int transform_mode{};           // 0 = rigid (Isometry), 1 = affine: which ICP instance family cilhip_icp_run mirrors
  float normal_weight{};          // > 0: the correspondence search runs on 6-D features (point, weight * v)
  int feature_kind{};             // option "feature_kind": 0 = v = normals, following the transform (PointNormalFeaturesAdaptor);
                                  // 1 = v = colours, untouched by it (PointColorFeaturesAdaptor; cilhip_set_color_features)
  float color_weight{};           // option "feature_color_weight" (feature_kind 2: the 9-D adaptor's colour weight)
  bool symmetric{};               // source normals, when set, also switch the combined metric to the symmetric objective
  bool reverse_warm{};            // option "reverse_warm_start": the device-resident FIRST_TO_SECOND / BOTH loops start every reverse search but the first from the previous matches
  bool kernel_timing{};
  int timing_stride{};            // option "kernel_timing_stride": with kernel timing on, iterations 0..2 and every stride-th one carry events
};

// What a newly stored value makes stale, by event (ctx.hpp: apply_stale says which buffers and flags each one lets go of).
enum : unsigned {
  STALE_CORRESPONDENCES = 1u,     // the stored correspondence set, matches and pair list
  STALE_MATCHES = 2u,             // ... the matches alone
  STALE_PENDING_MATCHES = 4u,     // ... a finished run's set that has not been searched again yet (cilhip_get_last_matches_origin 2): it would be
                                  // filtered with the NEW values; a set already in memory is what its search left, whatever is set afterwards
  STALE_SRC_GRID = 8u,            // the source's own grid (it carries the feature vectors of the reverse searches)
  STALE_FEAT_ORDER = 16u,         // the feature tree's order tables (one target under one set of feature options)
};

// A row stores a value that is a number inside [min_value, max_value]: it adds what a range cannot say (the discrete values of
// group_search, tie_rule, ...) and returns the key's own refusal, or stores, reports through *stale, and returns null.
struct OptionRow {
  cilhip_option_info_t info;
  double (*get)(const CtxOptions&);
  const char* (*set)(CtxOptions&, double, unsigned* stale);
};

namespace option_rows {
// a field that takes the value as its own type does: a bool is "not zero" (0.5 stores true), an int truncates (1.5 stores 1)
template <auto M> double get_field(const CtxOptions& o) { return (double)(o.*M); }
template <auto M> const char* set_field(CtxOptions& o, double v, unsigned*) {
  o.*M = static_cast<std::remove_reference_t<decltype(o.*M)>>(v);
  return nullptr;
}
inline bool whole_up_to(double v, int hi) {
  for (int k = 0; k <= hi; ++k) if (v == (double)k) return true;
  return false;
}
constexpr const char* kEvaluatorKinds = "weight evaluator: 0 = Unity, 1 = Identity, 2 = RBF kernel";
}  // namespace option_rows

#define CILHIP_FIELD(ID, KEY, DEF, LO, HI, DOC, FIELD) \
  {{ID, KEY, DEF, LO, HI, DOC}, option_rows::get_field<&CtxOptions::FIELD>, option_rows::set_field<&CtxOptions::FIELD>}
#define CILHIP_ROW(ID, KEY, DEF, LO, HI, DOC, GET, ...)                              \
  {{ID, KEY, DEF, LO, HI, DOC}, [](const CtxOptions& o) -> double { return (double)(GET); }, \
   [](CtxOptions& o, double v, unsigned* stale) -> const char* { (void)stale; __VA_ARGS__ return nullptr; }}
inline const OptionRow kOptionRows[] = {
  CILHIP_FIELD(CILHIP_OPT_FUSED, "fused", 0, 0, 1, "1 = one per-lane search+accumulate kernel per iteration; 0 = search kernel + streaming accumulation (or the LDS tiles)", fused),
  CILHIP_ROW(CILHIP_OPT_INLIER_FRACTION, "inlier_fraction", 1, 0, 1, "CorrespondenceSearchKDTree::setInlierFraction: keep that fraction of the correspondences, nearest first", o.inlier_fraction,
             if (o.inlier_fraction != v) *stale |= STALE_PENDING_MATCHES;
             o.inlier_fraction = v;),
  CILHIP_ROW(CILHIP_OPT_ONE_TO_ONE, "one_to_one", 0, 0, 1, "setOneToOne: a target point keeps only its nearest source point", o.one_to_one,
             if (o.one_to_one != (v != 0.0)) *stale |= STALE_PENDING_MATCHES;
             o.one_to_one = v != 0.0;),
  CILHIP_FIELD(CILHIP_OPT_TILED, "tiled", 1, 0, 2, "LDS-tiled search: 0 = never, 1 = when the cloud fills the chip with full tiles, 2 = always", tiled),
  CILHIP_FIELD(CILHIP_OPT_WARM_START, "warm_start", 1, 0, 2, "warm-started iterations (margin proof): 0 = never, 1 = when the loop is near alignment, 2 = from the second iteration on", warm_start),
  CILHIP_FIELD(CILHIP_OPT_WARM_FORECAST, "warm_forecast", 1, 0, 1, "the cold kernels' forecast gates the warm-started form (0: the step alone; tests)", warm_forecast),
  CILHIP_FIELD(CILHIP_OPT_FUSED_EPILOGUE, "fused_epilogue", 0, 0, 1, "stage-1 reduction + epilogue as one launch behind a device-scope fence (bitwise equal, measured slower; A/B)", fused_epilogue),
  CILHIP_ROW(CILHIP_OPT_GROUP_SEARCH, "group_search", -1, -1, 64, "lanes per query of the cooperative global-memory search: -1 = the loop decides, 0 = never, 4 / 8 / 16 / 32 / 64", o.group_lanes,
             if (v != -1.0 && v != 0.0 && v != 4.0 && v != 8.0 && v != 16.0 && v != 32.0 && v != 64.0)
               return "group_search: -1 (the loop decides), 0 (never), or 4, 8, 16, 32, 64 lanes per query";
             o.group_lanes = (int)v;),
  CILHIP_ROW(CILHIP_OPT_TIE_RULE, "tie_rule", 2, 0, 2, "exactly equidistant nearest points: 0 = lowest index, 1 = the reference's kd-tree order (tables up front), 2 = the same, tables when a tie is first met", o.tie_rule,
             if (!option_rows::whole_up_to(v, 2))
               return "tie_rule: 0 (lowest index), 1 (the reference's kd-tree order, tables built up front) or 2 (the same, tables built when a tie is first met)";
             if (((int)v != 0) != (o.tie_rule != 0)) *stale |= STALE_MATCHES;      // (switched on or off; a pair list keeps the order its own search settled)
             o.tie_rule = (int)v;),
  CILHIP_FIELD(CILHIP_OPT_WARM_EXTRA_FRACTION, "warm_extra_fraction", 0.0625, 1e-9, 1, "room (fraction of a cell) of the ball a warm-started iteration searches a listed query in", warm_extra),
  CILHIP_FIELD(CILHIP_OPT_PAIR_RECORDS, "pair_records", 1, 0, 1, "streaming accumulation gathers a match's point and normal from one 32-byte record (A/B)", pair_records),
  CILHIP_FIELD(CILHIP_OPT_TILE_RECORDS, "tile_records", 1, 0, 1, "the accumulating tile kernel writes the warm-started form's match records itself (A/B)", tile_records),
  CILHIP_FIELD(CILHIP_OPT_WARM_ENTER_FRACTION, "warm_enter_fraction", 0.15, 1e-9, 1e9, "the warm-started form is entered once an update moves no source point by more than this fraction of a cell", warm_enter),
  CILHIP_ROW(CILHIP_OPT_POINT_WEIGHT_EVALUATOR, "point_weight_evaluator", 0, 0, 2, "combined metric, point-to-point terms: 0 = UnityWeightEvaluator, 1 = DistanceEvaluator, 2 = RBFKernelWeightEvaluator", o.cw_point_kind,
             if (!option_rows::whole_up_to(v, 2)) return option_rows::kEvaluatorKinds;
             o.cw_point_kind = (int)v;),
  CILHIP_ROW(CILHIP_OPT_PLANE_WEIGHT_EVALUATOR, "plane_weight_evaluator", 0, 0, 2, "combined metric, point-to-plane terms: 0 = Unity, 1 = Identity (distance), 2 = RBF kernel", o.cw_plane_kind,
             if (!option_rows::whole_up_to(v, 2)) return option_rows::kEvaluatorKinds;
             o.cw_plane_kind = (int)v;),
  CILHIP_FIELD(CILHIP_OPT_POINT_WEIGHT_SIGMA, "point_weight_sigma", 1, 1e-30, 1e30, "sigma of the RBF evaluator of the point-to-point terms", cw_point_sigma),
  CILHIP_FIELD(CILHIP_OPT_PLANE_WEIGHT_SIGMA, "plane_weight_sigma", 1, 1e-30, 1e30, "sigma of the RBF evaluator of the point-to-plane terms", cw_plane_sigma),
  CILHIP_ROW(CILHIP_OPT_TILE_ACCUMULATION, "tile_accumulation", 1, 0, 2, "first Gauss-Newton step accumulated inside the LDS tiles: 0 = never, 1 = unless the source is far from alignment, 2 = always",
             (o.tile_acc ? (o.tile_acc_adaptive ? 1 : 2) : 0),
             o.tile_acc = v != 0.0; o.tile_acc_adaptive = v != 2.0;),
  CILHIP_ROW(CILHIP_OPT_SEARCH_DIRECTION, "search_direction", 0, 0, 2, "CorrespondenceSearchDirection: 0 = SECOND_TO_FIRST, 1 = FIRST_TO_SECOND, 2 = BOTH", o.search_dir,
             if (!option_rows::whole_up_to(v, 2)) return "search_direction: 0 = SECOND_TO_FIRST, 1 = FIRST_TO_SECOND, 2 = BOTH";
             o.search_dir = (int)v; *stale |= STALE_CORRESPONDENCES;),
  CILHIP_ROW(CILHIP_OPT_FEATURE_NORMAL_WEIGHT, "feature_normal_weight", 0, 0, 1e30, "PointNormalFeaturesAdaptor's normal weight (> 0: the search runs on 6-D features)", o.normal_weight,
             if (o.normal_weight != (float)v) *stale |= STALE_FEAT_ORDER;
             o.normal_weight = (float)v; *stale |= STALE_CORRESPONDENCES;),
  CILHIP_ROW(CILHIP_OPT_FEATURE_KIND, "feature_kind", 0, 0, 2, "second feature block: 0 = normals (follow the transform), 1 = colours (do not), 2 = normals + colours (9-D)", o.feature_kind,
             if (!option_rows::whole_up_to(v, 2)) return "feature_kind: 0 = normals (follow the transform), 1 = colours (do not), 2 = normals + colours (9-D)";
             if ((int)v != o.feature_kind) *stale |= STALE_SRC_GRID | STALE_FEAT_ORDER;
             o.feature_kind = (int)v; *stale |= STALE_CORRESPONDENCES;),
  CILHIP_ROW(CILHIP_OPT_FEATURE_COLOR_WEIGHT, "feature_color_weight", 0, 0, 1e30, "PointNormalColorFeaturesAdaptor's colour weight (feature_kind 2)", o.color_weight,
             if (o.color_weight != (float)v) *stale |= STALE_FEAT_ORDER;
             o.color_weight = (float)v; *stale |= STALE_CORRESPONDENCES;),
  CILHIP_FIELD(CILHIP_OPT_SYMMETRIC_METRIC, "symmetric_metric", 1, 0, 1, "source normals, when set, switch the combined metric to the symmetric objective", symmetric),
  CILHIP_ROW(CILHIP_OPT_TRANSFORM_MODE, "transform_mode", 0, 0, 1, "ICP instance family: 0 = rigid, 1 = affine", o.transform_mode,
             if (!option_rows::whole_up_to(v, 1)) return "transform_mode: 0 = rigid, 1 = affine";
             o.transform_mode = (int)v;),
  CILHIP_ROW(CILHIP_OPT_REQUIRE_RECIPROCALITY, "require_reciprocality", 0, 0, 1, "setRequireReciprocality (search_direction BOTH)", o.reciprocal,
             o.reciprocal = v != 0.0; *stale |= STALE_CORRESPONDENCES;),
  CILHIP_FIELD(CILHIP_OPT_CELL_OCCUPANCY, "cell_occupancy", 1, 1e-3, 1e6, "target points per grid cell the next cilhip_set_target aims at", cell_occupancy),
  CILHIP_FIELD(CILHIP_OPT_REFINED_OCCUPANCY_FACTOR, "refined_occupancy_factor", 3, 1, 64, "how much denser than that a grid that had to be refined (surface, clusters) may stay", refined_occupancy),
  CILHIP_FIELD(CILHIP_OPT_KERNEL_TIMING, "kernel_timing", 0, 0, 1, "hipEvents around the search / accumulation kernels (cilhip_enable_kernel_timing)", kernel_timing),
  CILHIP_FIELD(CILHIP_OPT_KERNEL_TIMING_STRIDE, "kernel_timing_stride", 1, 1, 4096, "with kernel timing on: iterations 0..2 and every stride-th one carry events", timing_stride),
  CILHIP_FIELD(CILHIP_OPT_REVERSE_WARM_START, "reverse_warm_start", 1, 0, 1, "device-resident FIRST_TO_SECOND / BOTH loops: reverse searches after the first start from the previous reverse matches (margin test over the source; A/B)", reverse_warm),
  CILHIP_FIELD(CILHIP_OPT_FEATURE_WARM_START, "feature_warm_start", 1, 0, 1, "feature adaptors (SECOND_TO_FIRST loops): searches warm-started from the previous matches once the loop moves little (margin test with the feature distance; A/B)", feat_warm),
  CILHIP_FIELD(CILHIP_OPT_AFFINE_DEVICE_LOOP, "affine_device_loop", 1, 0, 1, "affine classes: 1 = device-resident loop (one-pass moments, solve in the epilogue kernel), 0 = host-driven loop (three passes + host solve; A/B)", affine_device_loop),
};
#undef CILHIP_FIELD
#undef CILHIP_ROW
constexpr int N_OPTIONS = (int)(sizeof(kOptionRows) / sizeof(kOptionRows[0]));
static_assert(N_OPTIONS == CILHIP_OPT_COUNT, "one table row per enum cilhip_option value, in the enum's order");

inline CtxOptions::CtxOptions() {
  unsigned stale = 0;
  for (const OptionRow& r : kOptionRows) r.set(*this, r.info.default_value, &stale);
}

}  // namespace cilhip

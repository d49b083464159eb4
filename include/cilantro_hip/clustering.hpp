// cilantro_hip/clustering.hpp -- C++ host-side mirrors of cilantro's connected-component segmentation and mean-shift clustering,
// header-only on top of the C ABI (c_api.h: cilhip_connected_components3f and cilhip_mean_shift3f, which state the contracts; DESIGN.md
// sections 11 and 13):
//
//   MeanShift3f                                clustering/mean_shift.hpp:12-140 (the end of this file)
//   Unity / Identity / RBFKernel WeightEvaluator               core/common_pair_evaluators.hpp:13-79
//   ConnectedComponentExtraction3f             clustering/connected_component_extraction.hpp:368-428 (segment :394-422)
//   the ClusteringBase accessors               clustering/clustering_base.hpp:60-97
//   RadiusNeighborhoodSpecification<float>     core/nearest_neighbors.hpp (the radius is a SQUARED distance)
//   AlwaysTrueEvaluator and the seven proximity evaluators      core/common_pair_evaluators.hpp:84-259, constructor arguments in the reference's order
//
// Clouds go in as non-owning (pointer, count) views.  An evaluator here is a description of its clauses, evaluated on the device; other
// neighbourhood kinds and user functors go through cilhip_connected_components_lists (lists of cilhip_radius_search3f / cilhip_knn3f and
// a byte mask the caller's functor filled).  No CPU fallback: a failing C-ABI call throws.
#pragma once

#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "c_api.h"
#include "icp.hpp"

namespace cilantro_hip {

template <typename ScalarT = float>
struct RadiusNeighborhoodSpecification {
  ScalarT radius;      // squared
  explicit RadiusNeighborhoodSpecification(ScalarT radius_sq = (ScalarT)0) : radius(radius_sq) {}
};

// what an evaluator asks of a pair: the clauses of cilhip_cc_params and the arrays they read
struct PointSimilarityClauses {
  const float* normals = nullptr;
  const float* colors = nullptr;
  size_t count = 0;      // rows of the arrays (0: no array)
  bool use_distance = false, use_normals = false, use_colors = false, angle_inclusive = false;
  float max_distance = 0.0f, max_angle = 0.0f, color_thresh = 0.0f;
};

namespace detail {
inline PointSimilarityClauses clauses(const ConstPointsView* normals, const ConstPointsView* colors, const float* dist, const float* angle, const float* color, bool inclusive) {
  PointSimilarityClauses c;
  if (normals) { c.normals = normals->data(); c.count = normals->cols(); }
  if (colors) { c.colors = colors->data(); c.count = colors->cols(); }
  if (normals && colors && normals->cols() != colors->cols()) throw std::invalid_argument("evaluator: normals and colors differ in size");
  if (dist) { c.use_distance = true; c.max_distance = *dist; }
  if (angle) { c.use_normals = true; c.max_angle = *angle; c.angle_inclusive = inclusive; }
  if (color) { c.use_colors = true; c.color_thresh = *color; }
  return c;
}
}  // namespace detail

struct AlwaysTrueEvaluator {      // :87-88
  PointSimilarityClauses clauses() const { return PointSimilarityClauses(); }
};
class PointsProximityEvaluator {      // :92-104
public:
  explicit PointsProximityEvaluator(float dist_thresh) : d_(dist_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(nullptr, nullptr, &d_, nullptr, nullptr, false); }
private:
  float d_;
};
class NormalsProximityEvaluator {      // :106-128 -- the one class whose angle test is <= (:119-121)
public:
  NormalsProximityEvaluator(const ConstPointsView& normals, float angle_thresh) : n_(normals), a_(angle_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, nullptr, nullptr, &a_, nullptr, true); }
private:
  ConstPointsView n_;
  float a_;
};
class ColorsProximityEvaluator {      // :130-146
public:
  ColorsProximityEvaluator(const ConstPointsView& colors, float dist_thresh) : c_(colors), t_(dist_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(nullptr, &c_, nullptr, nullptr, &t_, false); }
private:
  ConstPointsView c_;
  float t_;
};
class PointsNormalsProximityEvaluator {      // :148-172
public:
  PointsNormalsProximityEvaluator(const ConstPointsView& normals, float dist_thresh, float angle_thresh) : n_(normals), d_(dist_thresh), a_(angle_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, nullptr, &d_, &a_, nullptr, false); }
private:
  ConstPointsView n_;
  float d_, a_;
};
class PointsColorsProximityEvaluator {      // :174-193
public:
  PointsColorsProximityEvaluator(const ConstPointsView& colors, float dist_thresh, float color_thresh) : c_(colors), d_(dist_thresh), t_(color_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(nullptr, &c_, &d_, nullptr, &t_, false); }
private:
  ConstPointsView c_;
  float d_, t_;
};
class NormalsColorsProximityEvaluator {      // :195-224
public:
  NormalsColorsProximityEvaluator(const ConstPointsView& normals, const ConstPointsView& colors, float angle_thresh, float color_thresh)
      : n_(normals), c_(colors), a_(angle_thresh), t_(color_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, &c_, nullptr, &a_, &t_, false); }
private:
  ConstPointsView n_, c_;
  float a_, t_;
};
class PointsNormalsColorsProximityEvaluator {      // :226-259
public:
  PointsNormalsColorsProximityEvaluator(const ConstPointsView& normals, const ConstPointsView& colors, float dist_thresh, float angle_thresh, float color_thresh)
      : n_(normals), c_(colors), d_(dist_thresh), a_(angle_thresh), t_(color_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, &c_, &d_, &a_, &t_, false); }
private:
  ConstPointsView n_, c_;
  float d_, a_, t_;
};

// (a template as in the reference, where the name is an alias template: `ConnectedComponentExtraction3f<> cce(points);`)
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class ConnectedComponentExtraction3f {
public:
  typedef std::vector<std::vector<PointIndexT>> ClusterToPointIndicesMap;      // clustering_base.hpp:67-68
  typedef std::vector<ClusterIndexT> PointToClusterIndexMap;

  explicit ConnectedComponentExtraction3f(const ConstPointsView& points, int device = 0) : points_(points), device_(device) {}

  // :409-422 -- every point is a seed
  template <class PointSimilarityEvaluator = AlwaysTrueEvaluator>
  ConnectedComponentExtraction3f& segment(const RadiusNeighborhoodSpecification<float>& nh, const PointSimilarityEvaluator& evaluator = PointSimilarityEvaluator(),
                                          size_t min_segment_size = 1, size_t max_segment_size = std::numeric_limits<size_t>::max()) {
    return run(nh, nullptr, evaluator.clauses(), min_segment_size, max_segment_size);
  }
  // :394-407 -- only the components that hold a seed
  template <class PointSimilarityEvaluator = AlwaysTrueEvaluator>
  ConnectedComponentExtraction3f& segment(const RadiusNeighborhoodSpecification<float>& nh, const std::vector<PointIndexT>& seeds_ind,
                                          const PointSimilarityEvaluator& evaluator = PointSimilarityEvaluator(), size_t min_segment_size = 1,
                                          size_t max_segment_size = std::numeric_limits<size_t>::max()) {
    return run(nh, &seeds_ind, evaluator.clauses(), min_segment_size, max_segment_size);
  }

  const ClusterToPointIndicesMap& getClusterToPointIndicesMap() const { return cluster_to_point_indices_map_; }
  const PointToClusterIndexMap& getPointToClusterIndexMap() const { return point_to_cluster_index_map_; }
  size_t getNumberOfClusters() const { return cluster_to_point_indices_map_.size(); }
  size_t getNumberOfPoints() const { return point_to_cluster_index_map_.size(); }
  std::vector<PointIndexT> getLabeledPointIndices() const { return select(true); }        // clustering_base.hpp:36-45
  std::vector<PointIndexT> getUnlabeledPointIndices() const { return select(false); }     // :49-58

private:
  ConnectedComponentExtraction3f& run(const RadiusNeighborhoodSpecification<float>& nh, const std::vector<PointIndexT>* seeds, const PointSimilarityClauses& c, size_t min_size,
                                      size_t max_size) {
    const size_t n = points_.cols();
    if (c.count != 0 && c.count != n) throw std::invalid_argument("segment: the evaluator's arrays and the points differ in size");
    cilhip_cc_params prm;
    cilhip_cc_default_params(&prm);
    prm.radius_sq = nh.radius;
    prm.use_distance = c.use_distance; prm.max_distance = c.max_distance;
    prm.use_normals = c.use_normals; prm.max_angle = c.max_angle; prm.angle_inclusive = c.angle_inclusive;
    prm.use_colors = c.use_colors; prm.color_thresh = c.color_thresh;
    prm.min_segment_size = min_size; prm.max_segment_size = max_size;
    std::vector<uint32_t> seed32(seeds ? seeds->size() + 1 : 0);      // (+ 1: an empty list is still a list)
    if (seeds)
      for (size_t k = 0; k < seeds->size(); ++k) {
        if ((size_t)(*seeds)[k] >= n) throw std::invalid_argument("segment: a seed index is not below the number of points");
        seed32[k] = (uint32_t)(*seeds)[k];
      }
    std::vector<uint32_t> labels(n + 1), offsets(n + 1), members(n + 1);
    size_t nseg = 0;
    const int rc = cilhip_connected_components3f(device_, points_.data(), c.normals, c.colors, n, CILHIP_MEM_HOST, &prm, seeds ? seed32.data() : nullptr, seeds ? seeds->size() : 0,
                                                 labels.data(), offsets.data(), members.data(), &nseg);
    if (rc != CILHIP_OK) throw std::runtime_error("cilhip_connected_components3f failed (rc " + std::to_string(rc) + "): " + cilhip_last_error(nullptr));
    cluster_to_point_indices_map_.assign(nseg, std::vector<PointIndexT>());
    for (size_t k = 0; k < nseg; ++k) cluster_to_point_indices_map_[k].assign(members.begin() + offsets[k], members.begin() + offsets[k + 1]);
    point_to_cluster_index_map_.assign(labels.begin(), labels.begin() + n);
    return *this;
  }
  std::vector<PointIndexT> select(bool labeled) const {
    std::vector<PointIndexT> res;
    const size_t k = getNumberOfClusters();
    for (size_t i = 0; i < point_to_cluster_index_map_.size(); ++i)
      if (((size_t)point_to_cluster_index_map_[i] < k) == labeled) res.push_back((PointIndexT)i);
    return res;
  }

  ConstPointsView points_;
  int device_;
  ClusterToPointIndicesMap cluster_to_point_indices_map_;
  PointToClusterIndexMap point_to_cluster_index_map_;
};

// ---- MeanShift3f -----------------------------------------------------------------------------------------------------------------
// The three kernel evaluators the device knows (a description, evaluated on the device; a caller's functor is not supported).
template <typename ScalarT = float, typename WeightT = ScalarT>
struct UnityWeightEvaluator {      // :30-43
  int kind() const { return 0; }
  float sigma() const { return 1.0f; }
};
template <typename ScalarT = float, typename WeightT = ScalarT>
struct IdentityWeightEvaluator {      // :14-27
  int kind() const { return 1; }
  float sigma() const { return 1.0f; }
};
template <typename ScalarT = float, typename WeightT = ScalarT>
class RBFKernelWeightEvaluator {      // :46-80
public:
  explicit RBFKernelWeightEvaluator(ScalarT sigma = (ScalarT)1) : sigma_((float)sigma) {}
  int kind() const { return 2; }
  float sigma() const { return sigma_; }
private:
  float sigma_;
};

template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class MeanShift3f {
public:
  typedef std::vector<std::vector<PointIndexT>> ClusterToPointIndicesMap;
  typedef std::vector<ClusterIndexT> PointToClusterIndexMap;

  // (max_leaf_size: the reference's kd-tree parameter, accepted and unused)
  explicit MeanShift3f(const ConstPointsView& points, size_t max_leaf_size = 10, int device = 0) : points_(points), device_(device) { (void)max_leaf_size; }

  // :38-115 -- given seeds
  template <class KernelEvaluatorT = UnityWeightEvaluator<float>>
  MeanShift3f& cluster(const ConstPointsView& seeds, float kernel_radius, size_t max_iter, float cluster_tol, float convergence_tol = std::numeric_limits<float>::epsilon(),
                       const KernelEvaluatorT& evaluator = KernelEvaluatorT()) {
    return run(&seeds, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator.kind(), evaluator.sigma());
  }
  // :118-124 -- every point is a seed
  template <class KernelEvaluatorT = UnityWeightEvaluator<float>>
  MeanShift3f& cluster(float kernel_radius, size_t max_iter, float cluster_tol, float convergence_tol = std::numeric_limits<float>::epsilon(),
                       const KernelEvaluatorT& evaluator = KernelEvaluatorT()) {
    return run(nullptr, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator.kind(), evaluator.sigma());
  }

  const std::vector<float>& getShiftedSeeds() const { return shifted_seeds_; }      // xyz per seed
  const std::vector<float>& getClusterModes() const { return cluster_modes_; }      // xyz per cluster
  size_t getNumberOfPerformedIterations() const { return iteration_count_; }
  const ClusterToPointIndicesMap& getClusterToPointIndicesMap() const { return cluster_to_point_indices_map_; }
  const PointToClusterIndexMap& getPointToClusterIndexMap() const { return point_to_cluster_index_map_; }
  size_t getNumberOfClusters() const { return cluster_to_point_indices_map_.size(); }
  size_t getNumberOfPoints() const { return point_to_cluster_index_map_.size(); }

private:
  MeanShift3f& run(const ConstPointsView* seeds, float kernel_radius, size_t max_iter, float cluster_tol, float convergence_tol, int kind, float sigma) {
    const size_t ns = seeds ? seeds->cols() : points_.cols();
    cilhip_ms_params prm;
    cilhip_ms_default_params(&prm);
    prm.kernel_radius = kernel_radius; prm.max_iter = max_iter; prm.cluster_tol = cluster_tol; prm.convergence_tol = convergence_tol;
    prm.kernel_kind = kind; prm.kernel_sigma = sigma;
    std::vector<float> shifted(3 * ns + 3), modes(3 * ns + 3), no_seed(3);
    std::vector<uint32_t> labels(ns + 1), offsets(ns + 1), members(ns + 1);
    size_t nc = 0, iters = 0;
    const float* sp = seeds ? (seeds->cols() ? seeds->data() : no_seed.data()) : nullptr;      // (an empty list is still a list)
    const int rc = cilhip_mean_shift3f(device_, points_.data(), points_.cols(), sp, seeds ? ns : 0, CILHIP_MEM_HOST, &prm, shifted.data(), labels.data(), modes.data(),
                                       offsets.data(), members.data(), &nc, &iters);
    if (rc != CILHIP_OK) throw std::runtime_error("cilhip_mean_shift3f failed (rc " + std::to_string(rc) + "): " + cilhip_last_error(nullptr));
    shifted_seeds_.assign(shifted.begin(), shifted.begin() + 3 * ns);
    cluster_modes_.assign(modes.begin(), modes.begin() + 3 * nc);
    iteration_count_ = iters;
    cluster_to_point_indices_map_.assign(nc, std::vector<PointIndexT>());
    for (size_t k = 0; k < nc; ++k) cluster_to_point_indices_map_[k].assign(members.begin() + offsets[k], members.begin() + offsets[k + 1]);
    point_to_cluster_index_map_.assign(labels.begin(), labels.begin() + ns);
    return *this;
  }

  ConstPointsView points_;
  int device_;
  size_t iteration_count_ = 0;
  std::vector<float> shifted_seeds_, cluster_modes_;
  ClusterToPointIndicesMap cluster_to_point_indices_map_;
  PointToClusterIndexMap point_to_cluster_index_map_;
};

}  // namespace cilantro_hip

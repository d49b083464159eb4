// cilantro_hip/clustering.hpp -- C++ host-side mirrors of cilantro's connected-component segmentation and mean-shift clustering,
// header-only on top of the C ABI (c_api.h: cilhip_connected_components3f and cilhip_mean_shift3f, which state the contracts; DESIGN.md
// sections 11 and 13):
//
//   SpectralClusteringXf / 2f / 3f, KMeansXf, getNNGraphFunctionValueSparseMatrix, estimateNumberOfClustersEigengap, GraphLaplacianType
//                                              clustering/spectral_clustering.hpp, kmeans.hpp:67-194, utilities/nearest_neighbor_graph_utilities.hpp:89-118
//                                              (the end of this file; cilhip_nn_graph_matrix, cilhip_spectral_embedding, cilhip_kmeans_nd)
//   MeanShift3f                                clustering/mean_shift.hpp:12-140 (before that)
//   MeanShiftXf, MeanShift2f                   clustering/mean_shift.hpp:142-164, over cilhip_mean_shift_nd (c_api.h rules M1-M7)
//   Unity / Identity / RBFKernel WeightEvaluator               core/common_pair_evaluators.hpp:13-79
//   ConnectedComponentExtraction3f             clustering/connected_component_extraction.hpp:368-428 (segment :394-422)
//   ConnectedComponentExtractionXf, 2f         clustering/connected_component_extraction.hpp:368-457, over cilhip_connected_components_nd (c_api.h rules C1-C5)
//   the ClusteringBase accessors               clustering/clustering_base.hpp:60-97 (detail::ClusterMaps, abi.hpp: the base of all six classes)
//   RadiusNeighborhoodSpecification<float>     core/nearest_neighbors.hpp (the radius is a SQUARED distance; abi.hpp)
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

#include "abi.hpp"
#include "c_api.h"
#include "icp.hpp"

namespace cilantro_hip {

// (RadiusNeighborhoodSpecification and ConstDataView, the non-owning view of a dim x n column-major float matrix: abi.hpp)

// what an evaluator asks of a pair: the clauses of cilhip_cc_params and the arrays they read
struct PointSimilarityClauses {
  const float* normals = nullptr;
  const float* colors = nullptr;
  size_t count = 0;      // rows of the arrays (0: no array)
  size_t normals_dim = 3;      // components of a normal: 3 (a ConstPointsView) or the rows of a ConstDataView (ConnectedComponentExtractionXf)
  bool use_distance = false, use_normals = false, use_colors = false, angle_inclusive = false;
  float max_distance = 0.0f, max_angle = 0.0f, color_thresh = 0.0f;
};

namespace detail {
// an evaluator's normals: a 3 x n view, or the N-D view of a dim x n matrix
struct NormalsRef {
  const float* data_;
  size_t dim_, cols_;
  NormalsRef(const ConstPointsView& v) : data_(v.data()), dim_(3), cols_(v.cols()) {}
  NormalsRef(const ConstDataView& v) : data_(v.data()), dim_(v.rows()), cols_(v.cols()) {}
  const float* data() const { return data_; }
  size_t cols() const { return cols_; }
};
inline PointSimilarityClauses clauses(const NormalsRef* normals, const ConstPointsView* colors, const float* dist, const float* angle, const float* color, bool inclusive) {
  PointSimilarityClauses c;
  if (normals) { c.normals = normals->data(); c.count = normals->cols(); c.normals_dim = normals->dim_; }
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
  NormalsProximityEvaluator(const ConstDataView& normals, float angle_thresh) : n_(normals), a_(angle_thresh) {}      // dim-component normals
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, nullptr, nullptr, &a_, nullptr, true); }
private:
  detail::NormalsRef n_;
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
  PointsNormalsProximityEvaluator(const ConstDataView& normals, float dist_thresh, float angle_thresh) : n_(normals), d_(dist_thresh), a_(angle_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, nullptr, &d_, &a_, nullptr, false); }
private:
  detail::NormalsRef n_;
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
  NormalsColorsProximityEvaluator(const ConstDataView& normals, const ConstPointsView& colors, float angle_thresh, float color_thresh)
      : n_(normals), c_(colors), a_(angle_thresh), t_(color_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, &c_, nullptr, &a_, &t_, false); }
private:
  detail::NormalsRef n_;
  ConstPointsView c_;
  float a_, t_;
};
class PointsNormalsColorsProximityEvaluator {      // :226-259
public:
  PointsNormalsColorsProximityEvaluator(const ConstPointsView& normals, const ConstPointsView& colors, float dist_thresh, float angle_thresh, float color_thresh)
      : n_(normals), c_(colors), d_(dist_thresh), a_(angle_thresh), t_(color_thresh) {}
  PointsNormalsColorsProximityEvaluator(const ConstDataView& normals, const ConstPointsView& colors, float dist_thresh, float angle_thresh, float color_thresh)
      : n_(normals), c_(colors), d_(dist_thresh), a_(angle_thresh), t_(color_thresh) {}
  PointSimilarityClauses clauses() const { return detail::clauses(&n_, &c_, &d_, &a_, &t_, false); }
private:
  detail::NormalsRef n_;
  ConstPointsView c_;
  float d_, a_, t_;
};

namespace detail {
// ConnectedComponentExtraction<float, EigenDim>::segment up to and after the C call (connected_component_extraction.hpp:368-457).  Derived
// supplies check_normals(clauses), the dimension check of an evaluator's normals, and call(...), its one entry (which throws when it fails).
template <class Derived, class ViewT, typename PointIndexT, typename ClusterIndexT>
class ConnectedComponentsBase : public ClusterMaps<PointIndexT, ClusterIndexT> {
public:
  // :409-422 -- every point is a seed
  template <class PointSimilarityEvaluator = AlwaysTrueEvaluator>
  Derived& segment(const RadiusNeighborhoodSpecification<float>& nh, const PointSimilarityEvaluator& evaluator = PointSimilarityEvaluator(), size_t min_segment_size = 1,
                   size_t max_segment_size = std::numeric_limits<size_t>::max()) {
    return run(nh, nullptr, evaluator.clauses(), min_segment_size, max_segment_size);
  }
  // :394-407 -- only the components that hold a seed
  template <class PointSimilarityEvaluator = AlwaysTrueEvaluator>
  Derived& segment(const RadiusNeighborhoodSpecification<float>& nh, const std::vector<PointIndexT>& seeds_ind, const PointSimilarityEvaluator& evaluator = PointSimilarityEvaluator(),
                   size_t min_segment_size = 1, size_t max_segment_size = std::numeric_limits<size_t>::max()) {
    return run(nh, &seeds_ind, evaluator.clauses(), min_segment_size, max_segment_size);
  }

  std::vector<PointIndexT> getLabeledPointIndices() const { return this->select(true); }        // clustering_base.hpp:36-45
  std::vector<PointIndexT> getUnlabeledPointIndices() const { return this->select(false); }     // :49-58

protected:
  ConnectedComponentsBase(const ViewT& points, int device) : points_(points), device_(device) {}

  // (protected for the hooks of the thin class only: not an interface for a user's subclass)
  ViewT points_;
  int device_;

private:
  Derived& run(const RadiusNeighborhoodSpecification<float>& nh, const std::vector<PointIndexT>* seeds, const PointSimilarityClauses& c, size_t min_size, size_t max_size) {
    Derived& self = static_cast<Derived&>(*this);
    const size_t n = points_.cols();
    if (c.count != 0 && c.count != n) throw std::invalid_argument("segment: the evaluator's arrays and the points differ in size");
    self.check_normals(c);
    cilhip_cc_params prm;
    cilhip_cc_default_params(&prm);
    prm.radius_sq = nh.radius;
    prm.use_distance = c.use_distance; prm.max_distance = c.max_distance;
    prm.use_normals = c.use_normals; prm.max_angle = c.max_angle; prm.angle_inclusive = c.angle_inclusive;
    prm.use_colors = c.use_colors; prm.color_thresh = c.color_thresh;
    prm.min_segment_size = min_size; prm.max_segment_size = max_size;
    std::vector<uint32_t> seed32(seeds ? room(seeds->size()) : 0);      // (an empty list is still a list)
    if (seeds)
      for (size_t k = 0; k < seeds->size(); ++k) {
        if ((size_t)(*seeds)[k] >= n) throw std::invalid_argument("segment: a seed index is not below the number of points");
        seed32[k] = (uint32_t)(*seeds)[k];
      }
    std::vector<uint32_t> labels(room(n)), offsets(n + 1), members(room(n));
    size_t nseg = 0;
    self.call(c, prm, seeds ? seed32.data() : nullptr, seeds ? seeds->size() : 0, labels.data(), offsets.data(), members.data(), &nseg);
    this->assign_csr(labels, n, offsets, members, nseg);
    return self;
  }
};
}  // namespace detail

// (a template as in the reference, where the name is an alias template: `ConnectedComponentExtraction3f<> cce(points);`)
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class ConnectedComponentExtraction3f : public detail::ConnectedComponentsBase<ConnectedComponentExtraction3f<PointIndexT, ClusterIndexT>, ConstPointsView, PointIndexT, ClusterIndexT> {
  typedef detail::ConnectedComponentsBase<ConnectedComponentExtraction3f, ConstPointsView, PointIndexT, ClusterIndexT> Base;
  friend Base;

public:
  explicit ConnectedComponentExtraction3f(const ConstPointsView& points, int device = 0) : Base(points, device) {}

private:
  void check_normals(const PointSimilarityClauses& c) const {
    if (c.use_normals && c.normals_dim != 3) throw std::invalid_argument("segment: the evaluator's normals are not 3 x n");
  }
  void call(const PointSimilarityClauses& c, const cilhip_cc_params& prm, const uint32_t* seeds, size_t n_seeds, uint32_t* labels, uint32_t* offsets, uint32_t* members, size_t* nseg) {
    detail::check(cilhip_connected_components3f(this->device_, this->points_.data(), c.normals, c.colors, this->points_.cols(), CILHIP_MEM_HOST, &prm, seeds, n_seeds, labels, offsets,
                                                members, nseg),
                  "cilhip_connected_components3f");
  }
};

// ---- ConnectedComponentExtractionXf / 2f (connected_component_extraction.hpp:368-457; c_api.h rules C1-C5) --------
// ConnectedComponentExtraction<float, Dynamic>: ConnectedComponentExtraction3f's interface over a dim x n view, 1 <= dim <= 16.  An
// evaluator's normals are a ConstDataView of dim x n, its colours a ConstPointsView (3 x n).  form: 0 the code decides, 1 the exhaustive
// triangle, 2 sweep and prune -- the same words (rule C4).
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class ConnectedComponentExtractionXf : public detail::ConnectedComponentsBase<ConnectedComponentExtractionXf<PointIndexT, ClusterIndexT>, ConstDataView, PointIndexT, ClusterIndexT> {
  typedef detail::ConnectedComponentsBase<ConnectedComponentExtractionXf, ConstDataView, PointIndexT, ClusterIndexT> Base;
  friend Base;

public:
  explicit ConnectedComponentExtractionXf(const ConstDataView& points, int device = 0, int form = 0) : Base(points, device), form_(form) {}

  size_t getDimension() const { return this->points_.rows(); }
  const cilhip_ccn_stats& getLastStats() const { return stats_; }      // what the last segment() did (zeros before one, and after one over no point)

private:
  void check_normals(const PointSimilarityClauses& c) const {
    if (c.use_normals && c.normals_dim != this->points_.rows()) throw std::invalid_argument("segment: the evaluator's normals are not dim x n");
  }
  void call(const PointSimilarityClauses& c, const cilhip_cc_params& prm, const uint32_t* seeds, size_t n_seeds, uint32_t* labels, uint32_t* offsets, uint32_t* members, size_t* nseg) {
    const size_t n = this->points_.cols();
    detail::check(cilhip_connected_components_nd(this->device_, this->points_.data(), c.normals, c.colors, n, this->points_.rows(), CILHIP_MEM_HOST, &prm, form_, seeds, n_seeds, labels,
                                                 offsets, members, nseg),
                  "cilhip_connected_components_nd");
    stats_ = cilhip_ccn_stats();
    if (n) cilhip_ccn_last_stats(&stats_);
  }

  int form_;
  cilhip_ccn_stats stats_ = cilhip_ccn_stats();
};

// ConnectedComponentExtraction<float, 2>
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class ConnectedComponentExtraction2f : public ConnectedComponentExtractionXf<PointIndexT, ClusterIndexT> {
public:
  explicit ConnectedComponentExtraction2f(const ConstDataView& points, int device = 0, int form = 0) : ConnectedComponentExtractionXf<PointIndexT, ClusterIndexT>(points, device, form) {
    if (points.rows() != 2) throw std::invalid_argument("ConnectedComponentExtraction2f: the points are a 2 x n matrix");
  }
  ConnectedComponentExtraction2f(const float* xy, size_t n, int device = 0) : ConnectedComponentExtractionXf<PointIndexT, ClusterIndexT>(ConstDataView(xy, 2, n), device, 0) {}
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

namespace detail {
// MeanShift<float, EigenDim>::cluster up to and after the C call (clustering/mean_shift.hpp:38-124); the dimension is the view's rows().
// Derived supplies check_seeds(seeds), the dimension check of a seed set, and call(...), its one entry (which throws when it fails).
template <class Derived, class ViewT, typename PointIndexT, typename ClusterIndexT>
class MeanShiftBase : public ClusterMaps<PointIndexT, ClusterIndexT> {
public:
  // :38-115 -- given seeds
  template <class KernelEvaluatorT = UnityWeightEvaluator<float>>
  Derived& cluster(const ViewT& seeds, float kernel_radius, size_t max_iter, float cluster_tol, float convergence_tol = std::numeric_limits<float>::epsilon(),
                   const KernelEvaluatorT& evaluator = KernelEvaluatorT()) {
    static_cast<Derived&>(*this).check_seeds(seeds);
    return run(&seeds, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator.kind(), evaluator.sigma());
  }
  // :118-124 -- every point is a seed
  template <class KernelEvaluatorT = UnityWeightEvaluator<float>>
  Derived& cluster(float kernel_radius, size_t max_iter, float cluster_tol, float convergence_tol = std::numeric_limits<float>::epsilon(),
                   const KernelEvaluatorT& evaluator = KernelEvaluatorT()) {
    return run(nullptr, kernel_radius, max_iter, cluster_tol, convergence_tol, evaluator.kind(), evaluator.sigma());
  }

  const std::vector<float>& getShiftedSeeds() const { return shifted_seeds_; }      // rows() floats per seed
  const std::vector<float>& getClusterModes() const { return cluster_modes_; }      // rows() floats per cluster
  size_t getNumberOfPerformedIterations() const { return iteration_count_; }

protected:
  MeanShiftBase(const ViewT& points, int device) : points_(points), device_(device) {}

  // (protected for the hooks of the thin class only: not an interface for a user's subclass)
  ViewT points_;
  int device_;

private:
  Derived& run(const ViewT* seeds, float kernel_radius, size_t max_iter, float cluster_tol, float convergence_tol, int kind, float sigma) {
    Derived& self = static_cast<Derived&>(*this);
    const size_t dim = points_.rows(), ns = seeds ? seeds->cols() : points_.cols();
    cilhip_ms_params prm;
    cilhip_ms_default_params(&prm);
    prm.kernel_radius = kernel_radius; prm.max_iter = max_iter; prm.cluster_tol = cluster_tol; prm.convergence_tol = convergence_tol;
    prm.kernel_kind = kind; prm.kernel_sigma = sigma;
    std::vector<float> shifted(room(dim * ns)), modes(room(dim * ns)), no_seed(room(dim));
    std::vector<uint32_t> labels(room(ns)), offsets(ns + 1), members(room(ns));
    size_t nc = 0, iters = 0;
    const float* sp = seeds ? (seeds->cols() ? seeds->data() : no_seed.data()) : nullptr;      // (an empty list is still a list)
    self.call(sp, seeds ? ns : 0, prm, shifted.data(), labels.data(), modes.data(), offsets.data(), members.data(), &nc, &iters);
    shifted_seeds_.assign(shifted.begin(), shifted.begin() + dim * ns);
    cluster_modes_.assign(modes.begin(), modes.begin() + dim * nc);
    iteration_count_ = iters;
    this->assign_csr(labels, ns, offsets, members, nc);
    return self;
  }

  size_t iteration_count_ = 0;
  std::vector<float> shifted_seeds_, cluster_modes_;
};
}  // namespace detail

template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class MeanShift3f : public detail::MeanShiftBase<MeanShift3f<PointIndexT, ClusterIndexT>, ConstPointsView, PointIndexT, ClusterIndexT> {
  typedef detail::MeanShiftBase<MeanShift3f, ConstPointsView, PointIndexT, ClusterIndexT> Base;
  friend Base;

public:
  // (max_leaf_size: the reference's kd-tree parameter, accepted and unused)
  explicit MeanShift3f(const ConstPointsView& points, size_t max_leaf_size = 10, int device = 0) : Base(points, device) { (void)max_leaf_size; }

private:
  void check_seeds(const ConstPointsView&) const {}
  void call(const float* seeds, size_t n_seeds, const cilhip_ms_params& prm, float* shifted, uint32_t* labels, float* modes, uint32_t* offsets, uint32_t* members, size_t* nc,
            size_t* iters) {
    detail::check(cilhip_mean_shift3f(this->device_, this->points_.data(), this->points_.cols(), seeds, n_seeds, CILHIP_MEM_HOST, &prm, shifted, labels, modes, offsets, members, nc, iters),
                  "cilhip_mean_shift3f");
  }
};

// ---- MeanShiftXf / MeanShift2f (clustering/mean_shift.hpp:142-164; c_api.h rules M1-M7) ---------------------
// MeanShift<float, Dynamic>: MeanShift3f's interface over a dim x n view, 1 <= dim <= 16; seeds, shifted seeds and modes are dim floats each.
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class MeanShiftXf : public detail::MeanShiftBase<MeanShiftXf<PointIndexT, ClusterIndexT>, ConstDataView, PointIndexT, ClusterIndexT> {
  typedef detail::MeanShiftBase<MeanShiftXf, ConstDataView, PointIndexT, ClusterIndexT> Base;
  friend Base;

public:
  // (max_leaf_size: the reference's kd-tree parameter, accepted and unused)
  explicit MeanShiftXf(const ConstDataView& points, size_t max_leaf_size = 10, int device = 0) : Base(points, device) { (void)max_leaf_size; }

  size_t getDimension() const { return this->points_.rows(); }

private:
  void check_seeds(const ConstDataView& seeds) const {
    if (seeds.rows() != this->points_.rows()) throw std::invalid_argument("MeanShiftXf: the seeds have another dimension than the points");
  }
  void call(const float* seeds, size_t n_seeds, const cilhip_ms_params& prm, float* shifted, uint32_t* labels, float* modes, uint32_t* offsets, uint32_t* members, size_t* nc,
            size_t* iters) {
    detail::check(cilhip_mean_shift_nd(this->device_, this->points_.data(), this->points_.cols(), this->points_.rows(), seeds, n_seeds, CILHIP_MEM_HOST, &prm, shifted, labels, modes,
                                       offsets, members, nc, iters),
                  "cilhip_mean_shift_nd");
  }
};

// MeanShift<float, 2>
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class MeanShift2f : public MeanShiftXf<PointIndexT, ClusterIndexT> {
public:
  explicit MeanShift2f(const ConstDataView& points, size_t max_leaf_size = 10, int device = 0) : MeanShiftXf<PointIndexT, ClusterIndexT>(points, max_leaf_size, device) {
    if (points.rows() != 2) throw std::invalid_argument("MeanShift2f: the points are a 2 x n matrix");
  }
  MeanShift2f(const float* xy, size_t n, int device = 0) : MeanShiftXf<PointIndexT, ClusterIndexT>(ConstDataView(xy, 2, n), 10, device) {}
};

// ---- SpectralClustering (clustering/spectral_clustering.hpp; c_api.h rules S1-S6) ---------------------------
enum struct GraphLaplacianType { UNNORMALIZED, NORMALIZED_SYMMETRIC, NORMALIZED_RANDOM_WALK };      // :44

// :46-68, literally
template <class VectorT>
size_t estimateNumberOfClustersEigengap(const VectorT& eigenvalues, size_t max_num_clusters) {
  typedef typename VectorT::value_type ScalarT;
  const size_t rows = eigenvalues.size();
  ScalarT min_val = std::numeric_limits<ScalarT>::infinity();
  ScalarT max_val = -std::numeric_limits<ScalarT>::infinity();
  ScalarT max_diff = eigenvalues[0];
  size_t max_ind = 0;
  for (size_t i = 0; i + 1 < rows; i++) {
    ScalarT diff = eigenvalues[i + 1] - eigenvalues[i];
    if (diff > max_diff) {
      max_diff = diff;
      max_ind = i;
    }
    if (eigenvalues[i] < min_val) min_val = eigenvalues[i];
    if (eigenvalues[i] > max_val) max_val = eigenvalues[i];
  }
  if (eigenvalues[rows - 1] < min_val) min_val = eigenvalues[rows - 1];
  if (eigenvalues[rows - 1] > max_val) max_val = eigenvalues[rows - 1];
  if (max_val - min_val < std::numeric_limits<ScalarT>::epsilon()) return max_num_clusters;
  return max_ind + 1;
}

// a sparse affinity matrix on the device (the owner of a cilhip_sparse handle): the place of Eigen::SparseMatrix<float> in the reference
class SparseAffinities {
public:
  SparseAffinities() = default;
  explicit SparseAffinities(cilhip_sparse* h) : h_(h) {}
  SparseAffinities(const SparseAffinities&) = delete;
  SparseAffinities& operator=(const SparseAffinities&) = delete;
  SparseAffinities(SparseAffinities&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  SparseAffinities& operator=(SparseAffinities&& o) noexcept {
    if (this != &o) { cilhip_sparse_destroy(h_); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  ~SparseAffinities() { cilhip_sparse_destroy(h_); }
  // a CSR matrix of the caller's: columns strictly ascending per row
  static SparseAffinities fromCSR(size_t n, const std::vector<uint64_t>& offsets, const std::vector<uint32_t>& columns, const std::vector<float>& values, int device = 0) {
    if (offsets.size() != n + 1 || columns.size() != values.size()) throw std::invalid_argument("SparseAffinities: offsets need n + 1 entries, columns and values one per entry");
    const uint32_t no_col = 0;
    const float no_val = 0.0f;
    cilhip_sparse* h = nullptr;
    detail::check(cilhip_sparse_from_csr(device, n, offsets.data(), columns.empty() ? &no_col : columns.data(), values.empty() ? &no_val : values.data(), CILHIP_MEM_HOST, &h),
                  "cilhip_sparse_from_csr");
    return SparseAffinities(h);
  }
  const cilhip_sparse* handle() const { return h_; }
  size_t rows() const { size_t n = 0; if (h_) cilhip_sparse_info(h_, &n, nullptr, nullptr); return n; }
  size_t cols() const { return rows(); }
  size_t nonZeros() const { size_t z = 0; if (h_) cilhip_sparse_info(h_, nullptr, &z, nullptr); return z; }

private:
  cilhip_sparse* h_ = nullptr;
};

// utilities/nearest_neighbor_graph_utilities.hpp:89-118 (the first entry of a list, the point itself, is kept; duplicates summed)
template <class PairEvaluatorT = UnityWeightEvaluator<float>>
SparseAffinities getNNGraphFunctionValueSparseMatrix(const NeighborhoodSet& adj_list, const PairEvaluatorT& evaluator = PairEvaluatorT(), bool force_symmetry = false,
                                                     int device = 0) {
  std::vector<uint64_t> off(adj_list.size() + 1, 0);
  for (size_t i = 0; i < adj_list.size(); ++i) off[i + 1] = off[i] + adj_list[i].size();
  std::vector<uint32_t> idx(detail::room((size_t)off.back()));
  std::vector<float> d2(detail::room((size_t)off.back()));
  for (size_t i = 0; i < adj_list.size(); ++i)
    for (size_t j = 0; j < adj_list[i].size(); ++j) {
      if (adj_list[i][j].index >= adj_list.size()) throw std::invalid_argument("getNNGraphFunctionValueSparseMatrix: a neighbour index is not below the number of lists");
      idx[(size_t)off[i] + j] = (uint32_t)adj_list[i][j].index;
      d2[(size_t)off[i] + j] = adj_list[i][j].value;
    }
  cilhip_sparse* h = nullptr;
  detail::check(cilhip_nn_graph_matrix(device, adj_list.size(), off.data(), idx.data(), d2.data(), (size_t)off.back(), CILHIP_MEM_HOST, evaluator.kind(), evaluator.sigma(),
                                       force_symmetry ? 1 : 0, 0, &h),
                "cilhip_nn_graph_matrix");
  return SparseAffinities(h);
}

// KMeans<float, Dynamic> (kmeans.hpp:67-194), brute-force branch, 1 <= dim <= 16.  The points are a non-owning dim x n column-major view
// (point-major floats); use_kd_tree is accepted and changes nothing (the kd-tree branch is not built in D dimensions).
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class KMeansXf : public detail::ClusterMaps<PointIndexT, ClusterIndexT> {
public:
  KMeansXf() = default;
  KMeansXf(const float* data, size_t num_points, size_t dim, int device = 0) : data_(data), n_(num_points), dim_(dim), device_(device) {}

  // kmeans.hpp:24-30
  KMeansXf& cluster(const std::vector<float>& centroids, size_t max_iter = 100, float tol = std::numeric_limits<float>::epsilon(), bool use_kd_tree = false) {
    (void)use_kd_tree;
    if (dim_ == 0 || centroids.size() % dim_ != 0) throw std::invalid_argument("KMeansXf: the centroids are dim floats each");
    cluster_centroids_ = centroids;
    const size_t k = centroids.size() / dim_;
    std::vector<uint32_t> labels(detail::room(n_));
    detail::check(cilhip_kmeans_nd(device_, data_, n_, dim_, CILHIP_MEM_HOST, cluster_centroids_.data(), k, max_iter, tol, labels.data(), &iteration_count_), "cilhip_kmeans_nd");
    this->assign_labels(labels, n_, k);
    return *this;
  }
  // the centroids start at the given points (the reference draws them with std::random_device, :32-53)
  KMeansXf& cluster(const std::vector<size_t>& initial_centroid_indices, size_t max_iter = 100, float tol = std::numeric_limits<float>::epsilon(), bool use_kd_tree = false) {
    std::vector<float> c;
    for (size_t i : initial_centroid_indices) {
      if (i >= n_) throw std::invalid_argument("KMeansXf: an initial centroid index is not below the number of points");
      c.insert(c.end(), data_ + i * dim_, data_ + (i + 1) * dim_);
    }
    return cluster(c, max_iter, tol, use_kd_tree);
  }

  const std::vector<float>& getClusterCentroids() const { return cluster_centroids_; }      // dim floats per cluster
  size_t getNumberOfPerformedIterations() const { return iteration_count_; }

protected:
  const float* data_ = nullptr;
  size_t n_ = 0, dim_ = 0;
  int device_ = 0;
  size_t iteration_count_ = 0;
  std::vector<float> cluster_centroids_;
};

// spectral_clustering.hpp:316-416, sparse input.  EigenDim > 0: the number of clusters (:377-391); EigenDim = -1 (Eigen::Dynamic): set at
// run time, optionally estimated from the eigenvalues (:397-416).  The reference starts k-means from random points; here from
// `initial_centroid_indices`, or from num_clusters points spread evenly over the index range when the list is empty.
template <ptrdiff_t EigenDim = -1, typename PointIndexT = size_t, typename ClusterIndexT = size_t>
class SpectralClustering : public KMeansXf<PointIndexT, ClusterIndexT> {
  typedef KMeansXf<PointIndexT, ClusterIndexT> Clusterer;

public:
  enum { EmbeddingDimension = EigenDim };

  // compile-time number of clusters
  explicit SpectralClustering(const SparseAffinities& affinities, const GraphLaplacianType& laplacian_type = GraphLaplacianType::NORMALIZED_RANDOM_WALK,
                              size_t kmeans_max_iter = 100, float kmeans_conv_tol = std::numeric_limits<float>::epsilon(), bool kmeans_use_kd_tree = false,
                              const std::vector<size_t>& initial_centroid_indices = std::vector<size_t>()) {
    static_assert(EigenDim > 0, "this constructor takes the number of clusters from EigenDim");
    run(affinities, (size_t)EigenDim, false, laplacian_type, kmeans_max_iter, kmeans_conv_tol, kmeans_use_kd_tree, initial_centroid_indices);
  }
  // run-time number of clusters
  SpectralClustering(const SparseAffinities& affinities, size_t max_num_clusters, bool estimate_num_clusters = false,
                     const GraphLaplacianType& laplacian_type = GraphLaplacianType::NORMALIZED_RANDOM_WALK, size_t kmeans_max_iter = 100,
                     float kmeans_conv_tol = std::numeric_limits<float>::epsilon(), bool kmeans_use_kd_tree = false,
                     const std::vector<size_t>& initial_centroid_indices = std::vector<size_t>()) {
    static_assert(EigenDim == -1, "this constructor belongs to the dynamic-dimension class");
    run(affinities, max_num_clusters, estimate_num_clusters, laplacian_type, kmeans_max_iter, kmeans_conv_tol, kmeans_use_kd_tree, initial_centroid_indices);
  }

  // spectral_embedding_base.hpp: dim floats per point (the reference's dim x n, column-major)
  const std::vector<float>& getEmbeddedPoints() const { return embedded_points_; }
  const std::vector<float>& getComputedEigenValues() const { return computed_eigenvalues_; }
  size_t getEmbeddingDimension() const { return this->dim_; }
  const cilhip_spectral_result& getSolverResult() const { return result_; }

private:
  void run(const SparseAffinities& affinities, size_t max_num_clusters, bool estimate, const GraphLaplacianType& type, size_t max_iter, float tol, bool use_kd_tree,
           const std::vector<size_t>& start) {
    if (!affinities.handle()) throw std::invalid_argument("SpectralClustering: the affinity matrix is empty");
    const size_t n = affinities.rows();
    cilhip_spectral_params prm;
    cilhip_spectral_default_params(&prm);
    prm.max_num_clusters = max_num_clusters; prm.estimate_num_clusters = estimate ? 1 : 0; prm.laplacian_type = (int)type;
    const size_t width = max_num_clusters >= 2 && max_num_clusters <= 16 ? max_num_clusters : 2;
    embedded_points_.assign(detail::room(n * width), 0.0f);
    computed_eigenvalues_.assign(width + 1, 0.0f);      // (c_api.h: room for max_num_clusters + 1)
    detail::check(cilhip_spectral_embedding(affinities.handle(), &prm, embedded_points_.data(), computed_eigenvalues_.data(), CILHIP_MEM_HOST, &result_), "cilhip_spectral_embedding");
    if (result_.n_converged < result_.num_eigenvalues)
      throw std::runtime_error("cilhip_spectral_embedding: " + std::to_string(result_.n_converged) + " of " + std::to_string(result_.num_eigenvalues) + " eigenpairs converged");
    const size_t k = result_.num_clusters;
    embedded_points_.resize(n * k);
    computed_eigenvalues_.resize(result_.num_eigenvalues);
    this->data_ = embedded_points_.data(); this->n_ = n; this->dim_ = k;
    std::vector<size_t> idx(start.begin(), start.begin() + (start.size() < k ? start.size() : k));
    if (idx.size() < k) { idx.clear(); for (size_t c = 0; c < k; ++c) idx.push_back(c * n / k); }
    Clusterer::cluster(idx, max_iter, tol, use_kd_tree);
  }

  std::vector<float> embedded_points_, computed_eigenvalues_;
  cilhip_spectral_result result_{};
};

template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
using SpectralClustering2f = SpectralClustering<2, PointIndexT, ClusterIndexT>;
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
using SpectralClustering3f = SpectralClustering<3, PointIndexT, ClusterIndexT>;
template <typename PointIndexT = size_t, typename ClusterIndexT = size_t>
using SpectralClusteringXf = SpectralClustering<-1, PointIndexT, ClusterIndexT>;

}  // namespace cilantro_hip

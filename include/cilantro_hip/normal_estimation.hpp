// cilantro_hip/normal_estimation.hpp -- C++ host-side mirrors of the k-NN side of cilantro's KDTree3f and of
// NormalEstimation3f, header-only on top of the C ABI (c_api.h):
//
//   KDTree3f              core/kd_tree.hpp:144-388     kNNSearch :216-256, radiusSearch :251-282, kNNInRadiusSearch :286-318
//   NormalEstimation3f    core/normal_estimation.hpp   get/estimate Normals[AndCurvature]KNN[InRadius] :72-221
//   RobustNormalEstimation3f   NormalEstimation<float, 3, MinimumCovarianceDeterminant<float, 3>> (core/covariance.hpp:185-371): the same getters over
//                         k-NN lists, covarianceMethod() for the trials / refinements / inlier ratio / chi-square threshold (and the seed)
//
// Same method names, argument meaning and defaults as the reference -- including its asymmetry: KDTree's radii are
// SQUARED distances (kd_tree.hpp:286-318), NormalEstimation takes a plain radius and squares it itself
// (normal_estimation.hpp:126, :174).  Clouds are non-owning (pointer, count) views.
// No CPU fallback: a failing C-ABI call throws.
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "abi.hpp"
#include "c_api.h"
#include "icp.hpp"

namespace cilantro_hip {

// (Neighbor / Neighborhood / NeighborhoodSet, core/nearest_neighbors.hpp:7-47, and the list helpers KDTreeXf shares: abi.hpp)

class KDTree3f {
public:
  explicit KDTree3f(const ConstPointsView& points, int device = 0) : points_(points), device_(device) {}

  // kd_tree.hpp:233-240 / :303-311: one Neighborhood per query, ascending distance
  NeighborhoodSet kNNSearch(const ConstPointsView& queries, size_t k) const { return search(queries, k, std::numeric_limits<float>::infinity()); }
  NeighborhoodSet kNNInRadiusSearch(const ConstPointsView& queries, size_t k, float radius) const { return search(queries, k, radius); }
  // kd_tree.hpp:266-282: every neighbour with squared distance < radius, ascending distance (equal distances by index)
  NeighborhoodSet radiusSearch(const ConstPointsView& queries, float radius) const {
    const size_t nq = queries.cols();
    return detail::radius_lists(nq, "cilhip_radius_search3f", [&](uint64_t* off, uint32_t* idx, float* d2, size_t capacity, size_t* total) {
      return cilhip_radius_search3f(device_, points_.data(), points_.cols(), queries.data(), nq, CILHIP_MEM_HOST, radius, off, idx, d2, capacity, total);
    });
  }
  const ConstPointsView& getPointsMatrixMap() const { return points_; }

private:
  NeighborhoodSet search(const ConstPointsView& queries, size_t k, float radius) const {
    const size_t nq = queries.cols();
    std::vector<uint32_t> idx(detail::room(nq * k)), cnt(detail::room(nq));
    std::vector<float> d2(detail::room(nq * k));
    detail::check(cilhip_knn3f(device_, points_.data(), points_.cols(), queries.data(), nq, CILHIP_MEM_HOST, k, radius, idx.data(), d2.data(), cnt.data()), "cilhip_knn3f");
    return detail::lists_from_rows(idx, d2, cnt, nq, k);
  }
  ConstPointsView points_;
  int device_;
};

namespace detail {
// NormalEstimation<float, 3, CovarianceT> (core/normal_estimation.hpp:72-221): the view point and the nine getters.  Derived supplies the
// two neighbourhoods as const members: knn(normals, curvature_or_null, k, radius_sq) and radius(normals, curvature_or_null, radius_sq).
template <class Derived>
class NormalEstimationBase {
public:
  const float* getViewPoint() const { return view_point_; }
  Derived& setViewPoint(const float vp[3]) { for (int i = 0; i < 3; ++i) view_point_[i] = vp[i]; return static_cast<Derived&>(*this); }
  Derived& setViewPoint(float x, float y, float z) { view_point_[0] = x; view_point_[1] = y; view_point_[2] = z; return static_cast<Derived&>(*this); }

  // normals: packed xyz per point (VectorSet<float,3>), curvature: one float per point
  const Derived& getNormalsAndCurvatureKNN(std::vector<float>& normals, std::vector<float>& curvature, size_t k) const {
    self().knn(normals, &curvature, k, std::numeric_limits<float>::infinity());
    return self();
  }
  std::vector<float> getNormalsKNN(size_t k) const { std::vector<float> n; self().knn(n, nullptr, k, std::numeric_limits<float>::infinity()); return n; }
  std::vector<float> getCurvatureKNN(size_t k) const { std::vector<float> n, c; self().knn(n, &c, k, std::numeric_limits<float>::infinity()); return c; }
  const Derived& getNormalsAndCurvatureKNNInRadius(std::vector<float>& normals, std::vector<float>& curvature, size_t k, float radius) const {
    self().knn(normals, &curvature, k, radius * radius);
    return self();
  }
  std::vector<float> getNormalsKNNInRadius(size_t k, float radius) const { std::vector<float> n; self().knn(n, nullptr, k, radius * radius); return n; }
  std::vector<float> getCurvatureKNNInRadius(size_t k, float radius) const { std::vector<float> n, c; self().knn(n, &c, k, radius * radius); return c; }
  // :120-162: every point inside the radius takes part
  const Derived& getNormalsAndCurvatureRadius(std::vector<float>& normals, std::vector<float>& curvature, float radius) const {
    self().radius(normals, &curvature, radius * radius);
    return self();
  }
  std::vector<float> getNormalsRadius(float radius) const { std::vector<float> n; self().radius(n, nullptr, radius * radius); return n; }
  std::vector<float> getCurvatureRadius(float radius) const { std::vector<float> n, c; self().radius(n, &c, radius * radius); return c; }

protected:
  NormalEstimationBase(const ConstPointsView& points, int device) : points_(points), device_(device) {
    const float nan = std::numeric_limits<float>::quiet_NaN();   // normal_estimation.hpp:24: no view point by default
    view_point_[0] = view_point_[1] = view_point_[2] = nan;
  }
  // the outputs at their sizes, zeroed; the number of points
  size_t size_outputs(std::vector<float>& normals, std::vector<float>* curvature) const {
    const size_t n = points_.cols();
    normals.assign(3 * n, 0.0f);
    if (curvature) curvature->assign(n, 0.0f);
    return n;
  }
  const Derived& self() const { return static_cast<const Derived&>(*this); }

  // (protected for the hooks of the thin class only: not an interface for a user's subclass)
  ConstPointsView points_;
  int device_;
  float view_point_[3];
};
}  // namespace detail

class NormalEstimation3f : public detail::NormalEstimationBase<NormalEstimation3f> {
  friend class detail::NormalEstimationBase<NormalEstimation3f>;

public:
  explicit NormalEstimation3f(const ConstPointsView& points, int device = 0) : NormalEstimationBase(points, device) {}

private:
  void knn(std::vector<float>& normals, std::vector<float>* curvature, size_t k, float radius_sq) const {
    const size_t n = size_outputs(normals, curvature);
    detail::check(cilhip_normals_knn3f(device_, points_.data(), n, CILHIP_MEM_HOST, k, radius_sq, view_point_, normals.data(), curvature ? curvature->data() : nullptr),
                  "cilhip_normals_knn3f");
  }
  // (an unbounded neighbourhood; moments accumulated without listing it)
  void radius(std::vector<float>& normals, std::vector<float>* curvature, float radius_sq) const {
    const size_t n = size_outputs(normals, curvature);
    detail::check(cilhip_normals_radius3f(device_, points_.data(), n, CILHIP_MEM_HOST, radius_sq, view_point_, normals.data(), curvature ? curvature->data() : nullptr),
                  "cilhip_normals_radius3f");
  }
};

// core/covariance.hpp:185-371: the settings of MinimumCovarianceDeterminant<float, 3>, same names and defaults (:365-369).  setSeed: the reference seeds
// its trials from std::random_device; here the draws follow from a stated seed (c_api.h: cilhip_robust_normals_knn3f), so runs repeat.
class MinimumCovarianceDeterminant3f {
public:
  int getNumberOfTrials() const { return num_trials_; }
  MinimumCovarianceDeterminant3f& setNumberOfTrials(int num_trials) { num_trials_ = num_trials; return *this; }
  int getNumberOfRefinements() const { return num_refinements_; }
  MinimumCovarianceDeterminant3f& setNumberOfRefinements(int num_refinements) { num_refinements_ = num_refinements; return *this; }
  float getInlierRatio() const { return inlier_ratio_; }
  MinimumCovarianceDeterminant3f& setInlierRatio(float inlier_ratio) { inlier_ratio_ = inlier_ratio; return *this; }
  float getChiSquareThreshold() const { return chi_square_threshold_; }
  MinimumCovarianceDeterminant3f& setChiSquareThreshold(float chi_square_threshold) { chi_square_threshold_ = chi_square_threshold; return *this; }
  uint64_t getSeed() const { return seed_; }
  MinimumCovarianceDeterminant3f& setSeed(uint64_t seed) { seed_ = seed; return *this; }

private:
  int num_trials_ = 6;
  int num_refinements_ = 3;
  float inlier_ratio_ = 0.75f;
  float chi_square_threshold_ = -1.0f;   // > 0: the covariance ellipsoid labels the point itself an in- or outlier (an outlier's normal is NaN)
  uint64_t seed_ = 0;
};

class RobustNormalEstimation3f : public detail::NormalEstimationBase<RobustNormalEstimation3f> {
  friend class detail::NormalEstimationBase<RobustNormalEstimation3f>;

public:
  explicit RobustNormalEstimation3f(const ConstPointsView& points, int device = 0) : NormalEstimationBase(points, device) {}

  const MinimumCovarianceDeterminant3f& covarianceMethod() const { return mcd_; }   // normal_estimation.hpp:62-64
  MinimumCovarianceDeterminant3f& covarianceMethod() { return mcd_; }

  // the decisions behind the normals: per point the final subset (bit j: list position j is in it) and the inlier flag of the chi-square test
  void getSubsetMasksAndInliersKNN(std::vector<uint32_t>& subset_masks, std::vector<uint8_t>& inliers, size_t k) const {
    std::vector<float> n;
    knn(n, nullptr, k, std::numeric_limits<float>::infinity(), &subset_masks, &inliers);
  }
  void getSubsetMasksAndInliersKNNInRadius(std::vector<uint32_t>& subset_masks, std::vector<uint8_t>& inliers, size_t k, float radius) const {
    std::vector<float> n;
    knn(n, nullptr, k, radius * radius, &subset_masks, &inliers);
  }

private:
  // A radius-only neighbourhood is unbounded: the engine accumulates its moments without listing it (cilhip_normals_radius3f), and the
  // trials need the list.  Bound it: ...KNNInRadius(k <= 32, radius).  The three ...Radius getters throw this.
  void radius(std::vector<float>&, std::vector<float>*, float) const {
    throw std::invalid_argument("RobustNormalEstimation3f: a radius-only neighbourhood keeps no neighbour list on the device, and the MCD trials rank a list; "
                                "use the ...KNNInRadius getters (k <= 32)");
  }
  void knn(std::vector<float>& normals, std::vector<float>* curvature, size_t k, float radius_sq, std::vector<uint32_t>* masks = nullptr,
           std::vector<uint8_t>* inliers = nullptr) const {
    const size_t n = size_outputs(normals, curvature);
    if (masks) masks->assign(n, 0u);
    if (inliers) inliers->assign(n, 0);
    cilhip_mcd_params p;
    cilhip_mcd_params_default(&p);
    p.k = k; p.max_sq_dist = radius_sq;
    p.num_trials = mcd_.getNumberOfTrials(); p.num_refinements = mcd_.getNumberOfRefinements();
    p.inlier_ratio = mcd_.getInlierRatio(); p.chi_square_threshold = mcd_.getChiSquareThreshold(); p.seed = mcd_.getSeed();
    float none = 0.0f;      // (an empty array still needs an address: this entry refuses a null normals_out whatever n is)
    detail::check(cilhip_robust_normals_knn3f(device_, points_.data(), n, CILHIP_MEM_HOST, &p, view_point_, n ? normals.data() : &none, curvature ? curvature->data() : nullptr,
                                              masks ? masks->data() : nullptr, inliers ? inliers->data() : nullptr),
                  "cilhip_robust_normals_knn3f");
  }
  MinimumCovarianceDeterminant3f mcd_;
};

}  // namespace cilantro_hip

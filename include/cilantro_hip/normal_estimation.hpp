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

#include "c_api.h"
#include "icp.hpp"

namespace cilantro_hip {

// (Neighbor / Neighborhood / NeighborhoodSet, core/nearest_neighbors.hpp:7-47: icp.hpp, which the warp-field classes share them with)

class KDTree3f {
public:
  explicit KDTree3f(const ConstPointsView& points, int device = 0) : points_(points), device_(device) {}

  // kd_tree.hpp:233-240 / :303-311: one Neighborhood per query, ascending distance
  NeighborhoodSet kNNSearch(const ConstPointsView& queries, size_t k) const { return search(queries, k, std::numeric_limits<float>::infinity()); }
  NeighborhoodSet kNNInRadiusSearch(const ConstPointsView& queries, size_t k, float radius) const { return search(queries, k, radius); }
  // kd_tree.hpp:266-282: every neighbour with squared distance < radius, ascending distance (equal distances by index)
  NeighborhoodSet radiusSearch(const ConstPointsView& queries, float radius) const {
    const size_t nq = queries.cols();
    std::vector<uint64_t> off(nq + 1, 0);
    size_t total = 0;
    int rc = cilhip_radius_search3f(device_, points_.data(), points_.cols(), queries.data(), nq, CILHIP_MEM_HOST, radius, off.data(), nullptr, nullptr, 0, &total);
    if (rc != CILHIP_OK) throw std::runtime_error("cilhip_radius_search3f failed (rc " + std::to_string(rc) + ")");
    std::vector<uint32_t> idx(total ? total : 1);
    std::vector<float> d2(total ? total : 1);
    if (total) {
      rc = cilhip_radius_search3f(device_, points_.data(), points_.cols(), queries.data(), nq, CILHIP_MEM_HOST, radius, off.data(), idx.data(), d2.data(), total, &total);
      if (rc != CILHIP_OK) throw std::runtime_error("cilhip_radius_search3f failed (rc " + std::to_string(rc) + ")");
    }
    NeighborhoodSet out(nq);
    for (size_t i = 0; i < nq; ++i) {
      out[i].resize((size_t)(off[i + 1] - off[i]));
      for (size_t j = 0; j < out[i].size(); ++j) out[i][j] = Neighbor{(size_t)idx[off[i] + j], d2[off[i] + j]};
    }
    return out;
  }
  const ConstPointsView& getPointsMatrixMap() const { return points_; }

private:
  NeighborhoodSet search(const ConstPointsView& queries, size_t k, float radius) const {
    const size_t nq = queries.cols();
    std::vector<uint32_t> idx(nq * k ? nq * k : 1), cnt(nq ? nq : 1);
    std::vector<float> d2(nq * k ? nq * k : 1);
    const int rc = cilhip_knn3f(device_, points_.data(), points_.cols(), queries.data(), nq, CILHIP_MEM_HOST, k, radius, idx.data(), d2.data(),
                                cnt.data());
    if (rc != CILHIP_OK) throw std::runtime_error("cilhip_knn3f failed (rc " + std::to_string(rc) + ")");
    NeighborhoodSet out(nq);
    for (size_t i = 0; i < nq; ++i) {
      out[i].resize(cnt[i]);
      for (size_t j = 0; j < cnt[i]; ++j) out[i][j] = Neighbor{(size_t)idx[i * k + j], d2[i * k + j]};
    }
    return out;
  }
  ConstPointsView points_;
  int device_;
};

class NormalEstimation3f {
public:
  explicit NormalEstimation3f(const ConstPointsView& points, int device = 0) : points_(points), device_(device) {
    const float nan = std::numeric_limits<float>::quiet_NaN();   // normal_estimation.hpp:24: no view point by default
    view_point_[0] = view_point_[1] = view_point_[2] = nan;
  }

  const float* getViewPoint() const { return view_point_; }
  NormalEstimation3f& setViewPoint(const float vp[3]) { for (int i = 0; i < 3; ++i) view_point_[i] = vp[i]; return *this; }
  NormalEstimation3f& setViewPoint(float x, float y, float z) { view_point_[0] = x; view_point_[1] = y; view_point_[2] = z; return *this; }

  // normals: packed xyz per point (VectorSet<float,3>), curvature: one float per point
  const NormalEstimation3f& getNormalsAndCurvatureKNN(std::vector<float>& normals, std::vector<float>& curvature, size_t k) const {
    run(normals, &curvature, k, std::numeric_limits<float>::infinity());
    return *this;
  }
  std::vector<float> getNormalsKNN(size_t k) const { std::vector<float> n; run(n, nullptr, k, std::numeric_limits<float>::infinity()); return n; }
  std::vector<float> getCurvatureKNN(size_t k) const { std::vector<float> n, c; run(n, &c, k, std::numeric_limits<float>::infinity()); return c; }
  const NormalEstimation3f& getNormalsAndCurvatureKNNInRadius(std::vector<float>& normals, std::vector<float>& curvature, size_t k, float radius) const {
    run(normals, &curvature, k, radius * radius);
    return *this;
  }
  std::vector<float> getNormalsKNNInRadius(size_t k, float radius) const { std::vector<float> n; run(n, nullptr, k, radius * radius); return n; }
  std::vector<float> getCurvatureKNNInRadius(size_t k, float radius) const { std::vector<float> n, c; run(n, &c, k, radius * radius); return c; }
  // :120-162: every point inside the radius takes part (unbounded neighbourhood; moments accumulated without listing it)
  const NormalEstimation3f& getNormalsAndCurvatureRadius(std::vector<float>& normals, std::vector<float>& curvature, float radius) const {
    run_radius(normals, &curvature, radius * radius);
    return *this;
  }
  std::vector<float> getNormalsRadius(float radius) const { std::vector<float> n; run_radius(n, nullptr, radius * radius); return n; }
  std::vector<float> getCurvatureRadius(float radius) const { std::vector<float> n, c; run_radius(n, &c, radius * radius); return c; }

private:
  void run(std::vector<float>& normals, std::vector<float>* curvature, size_t k, float radius) const {
    const size_t n = points_.cols();
    normals.assign(3 * n, 0.0f);
    if (curvature) curvature->assign(n, 0.0f);
    const int rc = cilhip_normals_knn3f(device_, points_.data(), n, CILHIP_MEM_HOST, k, radius, view_point_, normals.data(),
                                        curvature ? curvature->data() : nullptr);
    if (rc != CILHIP_OK) throw std::runtime_error("cilhip_normals_knn3f failed (rc " + std::to_string(rc) + ")");
  }
  void run_radius(std::vector<float>& normals, std::vector<float>* curvature, float radius_sq) const {
    const size_t n = points_.cols();
    normals.assign(3 * n, 0.0f);
    if (curvature) curvature->assign(n, 0.0f);
    const int rc = cilhip_normals_radius3f(device_, points_.data(), n, CILHIP_MEM_HOST, radius_sq, view_point_, normals.data(),
                                           curvature ? curvature->data() : nullptr);
    if (rc != CILHIP_OK) throw std::runtime_error("cilhip_normals_radius3f failed (rc " + std::to_string(rc) + ")");
  }
  ConstPointsView points_;
  int device_;
  float view_point_[3];
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

class RobustNormalEstimation3f {
public:
  explicit RobustNormalEstimation3f(const ConstPointsView& points, int device = 0) : points_(points), device_(device) {
    const float nan = std::numeric_limits<float>::quiet_NaN();
    view_point_[0] = view_point_[1] = view_point_[2] = nan;
  }

  const MinimumCovarianceDeterminant3f& covarianceMethod() const { return mcd_; }   // normal_estimation.hpp:62-64
  MinimumCovarianceDeterminant3f& covarianceMethod() { return mcd_; }

  const float* getViewPoint() const { return view_point_; }
  RobustNormalEstimation3f& setViewPoint(const float vp[3]) { for (int i = 0; i < 3; ++i) view_point_[i] = vp[i]; return *this; }
  RobustNormalEstimation3f& setViewPoint(float x, float y, float z) { view_point_[0] = x; view_point_[1] = y; view_point_[2] = z; return *this; }

  const RobustNormalEstimation3f& getNormalsAndCurvatureKNN(std::vector<float>& normals, std::vector<float>& curvature, size_t k) const {
    run(normals, &curvature, k, std::numeric_limits<float>::infinity());
    return *this;
  }
  std::vector<float> getNormalsKNN(size_t k) const { std::vector<float> n; run(n, nullptr, k, std::numeric_limits<float>::infinity()); return n; }
  std::vector<float> getCurvatureKNN(size_t k) const { std::vector<float> n, c; run(n, &c, k, std::numeric_limits<float>::infinity()); return c; }
  const RobustNormalEstimation3f& getNormalsAndCurvatureKNNInRadius(std::vector<float>& normals, std::vector<float>& curvature, size_t k, float radius) const {
    run(normals, &curvature, k, radius * radius);
    return *this;
  }
  std::vector<float> getNormalsKNNInRadius(size_t k, float radius) const { std::vector<float> n; run(n, nullptr, k, radius * radius); return n; }
  std::vector<float> getCurvatureKNNInRadius(size_t k, float radius) const { std::vector<float> n, c; run(n, &c, k, radius * radius); return c; }
  // A radius-only neighbourhood is unbounded: the engine accumulates its moments without listing it (cilhip_normals_radius3f), and the
  // trials need the list.  Bound it: ...KNNInRadius(k <= 32, radius).
  const RobustNormalEstimation3f& getNormalsAndCurvatureRadius(std::vector<float>&, std::vector<float>&, float) const { throw std::invalid_argument(radius_only()); }
  std::vector<float> getNormalsRadius(float) const { throw std::invalid_argument(radius_only()); }
  std::vector<float> getCurvatureRadius(float) const { throw std::invalid_argument(radius_only()); }

  // the decisions behind the normals: per point the final subset (bit j: list position j is in it) and the inlier flag of the chi-square test
  void getSubsetMasksAndInliersKNN(std::vector<uint32_t>& subset_masks, std::vector<uint8_t>& inliers, size_t k) const {
    std::vector<float> n;
    run(n, nullptr, k, std::numeric_limits<float>::infinity(), &subset_masks, &inliers);
  }
  void getSubsetMasksAndInliersKNNInRadius(std::vector<uint32_t>& subset_masks, std::vector<uint8_t>& inliers, size_t k, float radius) const {
    std::vector<float> n;
    run(n, nullptr, k, radius * radius, &subset_masks, &inliers);
  }

private:
  static const char* radius_only() {
    return "RobustNormalEstimation3f: a radius-only neighbourhood keeps no neighbour list on the device, and the MCD trials rank a list; "
           "use the ...KNNInRadius getters (k <= 32)";
  }
  void run(std::vector<float>& normals, std::vector<float>* curvature, size_t k, float radius_sq, std::vector<uint32_t>* masks = nullptr,
           std::vector<uint8_t>* inliers = nullptr) const {
    const size_t n = points_.cols();
    normals.assign(3 * n, 0.0f);
    if (curvature) curvature->assign(n, 0.0f);
    if (masks) masks->assign(n, 0u);
    if (inliers) inliers->assign(n, 0);
    cilhip_mcd_params p;
    cilhip_mcd_params_default(&p);
    p.k = k; p.max_sq_dist = radius_sq;
    p.num_trials = mcd_.getNumberOfTrials(); p.num_refinements = mcd_.getNumberOfRefinements();
    p.inlier_ratio = mcd_.getInlierRatio(); p.chi_square_threshold = mcd_.getChiSquareThreshold(); p.seed = mcd_.getSeed();
    float dummy[3];
    const int rc = cilhip_robust_normals_knn3f(device_, points_.data(), n, CILHIP_MEM_HOST, &p, view_point_, n ? normals.data() : dummy,
                                               curvature ? curvature->data() : nullptr, masks ? masks->data() : nullptr, inliers ? inliers->data() : nullptr);
    if (rc != CILHIP_OK) throw std::runtime_error(std::string("cilhip_robust_normals_knn3f failed (rc ") + std::to_string(rc) + "): " + cilhip_last_error(nullptr));
  }
  ConstPointsView points_;
  int device_;
  float view_point_[3];
  MinimumCovarianceDeterminant3f mcd_;
};

}  // namespace cilantro_hip

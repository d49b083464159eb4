// cilantro_hip/principal_component_analysis.hpp -- header-only C++ mirror of cilantro's core/principal_component_analysis.hpp (with
// core/covariance.hpp) on top of the C ABI (cilhip_pca_fit / _project / _reconstruct; c_api.h rules P1-P5):
//   PrincipalComponentAnalysis<float, Dim> / 2f / 3f / Xf
// Points are point-major float arrays on the host: n x dim, the reference's column-major dim x n.
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "abi.hpp"
#include "c_api.h"

namespace cilantro_hip {

// EigenDim > 0: the dimension; -1 (Eigen::Dynamic): given at run time.  ScalarT: float.
template <typename ScalarT = float, std::ptrdiff_t EigenDim = -1>
class PrincipalComponentAnalysis {
  static_assert(sizeof(ScalarT) == sizeof(float), "the device path is built for float");

 public:
  // all points (principal_component_analysis.hpp:17-22); `dim` must equal EigenDim when that is fixed
  PrincipalComponentAnalysis(const float* points, size_t n, size_t dim = (EigenDim > 0 ? (size_t)EigenDim : 0), int device = 0) : dim_(dim), device_(device) {
    fit(points, n, nullptr, 0);
  }
  // the points a subset names (:24-30)
  PrincipalComponentAnalysis(const float* points, size_t n, const std::vector<uint32_t>& subset, size_t dim = (EigenDim > 0 ? (size_t)EigenDim : 0), int device = 0)
      : dim_(dim), device_(device) {
    fit(points, n, subset.empty() ? &zero_ : subset.data(), subset.size());
  }

  const std::vector<float>& getDataMean() const { return mean_; }
  // dim x dim, symmetric
  const std::vector<float>& getDataCovariance() const { return covariance_; }
  // descending
  const std::vector<float>& getEigenValues() const { return eigenvalues_; }
  // the reference's column-major matrix: eigenvector c is [c * dim, (c + 1) * dim)
  const std::vector<float>& getEigenVectors() const { return eigenvectors_; }
  // false: fewer than two samples, every output is NaN (covariance.hpp:35-39)
  bool isValid() const { return valid_; }

  // :46-49 -> m x target_dim, point-major
  std::vector<float> project(const float* points, size_t m, size_t target_dim) const {
    std::vector<float> out(m * target_dim);
    detail::check(cilhip_pca_project(device_, points, m, dim_, CILHIP_MEM_HOST, mean_.data(), eigenvectors_.data(), target_dim, out.data()), "cilhip_pca_project");
    return out;
  }
  // :59-62: m x source_dim -> m x dim
  std::vector<float> reconstruct(const float* points, size_t m, size_t source_dim) const {
    std::vector<float> out(m * dim_);
    detail::check(cilhip_pca_reconstruct(device_, points, m, source_dim, dim_, CILHIP_MEM_HOST, mean_.data(), eigenvectors_.data(), out.data()), "cilhip_pca_reconstruct");
    return out;
  }

 private:
  size_t dim_;
  int device_;
  bool valid_ = false;
  uint32_t zero_ = 0;
  std::vector<float> mean_, covariance_, eigenvalues_, eigenvectors_;

  void fit(const float* points, size_t n, const uint32_t* subset, size_t n_subset) {
    if (EigenDim > 0 && dim_ != (size_t)EigenDim) throw std::invalid_argument("PrincipalComponentAnalysis: dim differs from the fixed dimension");
    if (dim_ == 0 || dim_ > 16) throw std::invalid_argument("PrincipalComponentAnalysis: dim must lie in [1, 16]");
    mean_.assign(dim_, 0.0f); covariance_.assign(dim_ * dim_, 0.0f); eigenvalues_.assign(dim_, 0.0f); eigenvectors_.assign(dim_ * dim_, 0.0f);
    int valid = 0;
    detail::check(cilhip_pca_fit(device_, points, n, dim_, subset, n_subset, CILHIP_MEM_HOST, mean_.data(), covariance_.data(), eigenvalues_.data(), eigenvectors_.data(), &valid),
                  "cilhip_pca_fit");
    valid_ = valid != 0;
  }
};

using PrincipalComponentAnalysis2f = PrincipalComponentAnalysis<float, 2>;
using PrincipalComponentAnalysis3f = PrincipalComponentAnalysis<float, 3>;
using PrincipalComponentAnalysisXf = PrincipalComponentAnalysis<float, -1>;

}  // namespace cilantro_hip

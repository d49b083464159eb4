// cilantro_hip/multidimensional_scaling.hpp -- header-only C++ mirror of cilantro's utilities/multidimensional_scaling.hpp on top of the
// C ABI (cilhip_mds_embedding; c_api.h rules M1-M5):
//   MultidimensionalScaling<float, Dim> / 2f / 3f / Xf, estimateEmbeddingDimensionEigengap
// Distances are a row-major n x n float array on the host (the reference's column-major matrix of a symmetric input is the same bytes).
#pragma once

#include <cstddef>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "abi.hpp"
#include "c_api.h"

namespace cilantro_hip {

// utilities/multidimensional_scaling.hpp:10-31
inline size_t estimateEmbeddingDimensionEigengap(const std::vector<float>& eigenvalues, size_t max_dim) {
  float min_val = std::numeric_limits<float>::infinity(), max_val = -min_val, max_diff = -std::numeric_limits<float>::infinity();
  size_t max_ind = 0;
  for (size_t i = 0; i + 1 < eigenvalues.size(); i++) {
    const float diff = eigenvalues[i] - eigenvalues[i + 1];
    if (diff > max_diff) { max_diff = diff; max_ind = i; }
    if (eigenvalues[i] < min_val) min_val = eigenvalues[i];
    if (eigenvalues[i] > max_val) max_val = eigenvalues[i];
  }
  if (eigenvalues.back() < min_val) min_val = eigenvalues.back();
  if (eigenvalues.back() > max_val) max_val = eigenvalues.back();
  if (max_val - min_val < std::numeric_limits<float>::epsilon()) return max_dim;
  return max_ind + 1;
}

// If positive, EigenDim is the embedding dimension; -1 (Eigen::Dynamic): set at run time (:86-120).  ScalarT: float.
template <typename ScalarT = float, std::ptrdiff_t EigenDim = -1>
class MultidimensionalScaling {
  static_assert(sizeof(ScalarT) == sizeof(float), "the device path is built for float");

 public:
  // Embedding dimension set at compile time
  template <std::ptrdiff_t Dim = EigenDim, class = typename std::enable_if<Dim != -1>::type>
  MultidimensionalScaling(const float* distances, size_t n, bool distances_are_squared = true, int device = 0) {
    compute(distances, n, (size_t)EigenDim, false, distances_are_squared, device);
  }
  // Embedding dimension set at run time: with estimate_dim it is chosen in [1, max_dim] from the eigenvalue distribution
  template <std::ptrdiff_t Dim = EigenDim, class = typename std::enable_if<Dim == -1>::type>
  MultidimensionalScaling(const float* distances, size_t n, size_t max_dim, bool estimate_dim = false, bool distances_are_squared = true, int device = 0) {
    compute(distances, n, max_dim, estimate_dim, distances_are_squared, device);
  }

  // core/spectral_embedding_base.hpp: point-major n x dim (the reference's column-major dim x n)
  const std::vector<float>& getEmbeddedPoints() const { return embedded_points_; }
  const std::vector<float>& getComputedEigenValues() const { return computed_eigenvalues_; }
  size_t getEmbeddingDimension() const { return result_.dim; }
  const cilhip_mds_result& getSolverResult() const { return result_; }

 private:
  std::vector<float> embedded_points_, computed_eigenvalues_;
  cilhip_mds_result result_{};

  void compute(const float* distances, size_t n, size_t max_dim, bool estimate_dim, bool distances_are_squared, int device) {
    cilhip_mds_params prm;
    cilhip_mds_default_params(&prm);
    prm.max_dim = max_dim; prm.estimate_dim = estimate_dim ? 1 : 0; prm.distances_are_squared = distances_are_squared ? 1 : 0;
    const size_t room = (max_dim == 0 || max_dim >= n) ? 2 : max_dim;
    embedded_points_.assign(n * room, 0.0f);
    computed_eigenvalues_.assign(room + 1, 0.0f);
    detail::check(cilhip_mds_embedding(device, distances, n, CILHIP_MEM_HOST, &prm, embedded_points_.data(), computed_eigenvalues_.data(), &result_), "cilhip_mds_embedding");
    if (result_.n_converged < result_.num_eigenvalues)
      throw std::runtime_error("cilhip_mds_embedding: " + std::to_string(result_.n_converged) + " of " + std::to_string(result_.num_eigenvalues) + " eigenpairs converged");
    embedded_points_.resize(n * result_.dim);
    computed_eigenvalues_.resize(result_.num_eigenvalues);
  }
};

using MultidimensionalScaling2f = MultidimensionalScaling<float, 2>;
using MultidimensionalScaling3f = MultidimensionalScaling<float, 3>;
using MultidimensionalScalingXf = MultidimensionalScaling<float, -1>;

}  // namespace cilantro_hip

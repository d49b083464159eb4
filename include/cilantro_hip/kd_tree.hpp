// cilantro_hip/kd_tree.hpp -- C++ host-side mirrors of cilantro's dimension-generic KDTree (core/kd_tree.hpp:144-406), header-only on top
// of the C ABI (c_api.h: cilhip_knn_nd, cilhip_radius_search_nd):
//
//   KDTreeXf     KDTree<float, Eigen::Dynamic, KDTreeDistanceAdaptors::L2>     any dimension from 1 to 16, taken from the view
//   KDTree2f     KDTree<float, 2, KDTreeDistanceAdaptors::L2>
//
// kNNSearch, kNNInRadiusSearch, radiusSearch, nearestNeighborSearch and search(queries, specification): same names and argument meaning as
// the reference -- radii are SQUARED distances.  A point set is a non-owning view of a dim x n column-major float matrix (the reference's
// ConstVectorSetMatrixMap: one point after the other).  The search is exhaustive and exact; lists ascend by (distance, index), so among
// exactly equal distances the lowest index is named (the reference: whichever its traversal meets first).  KDTree3f
// (normal_estimation.hpp) keeps the 3-D grid path.  No CPU fallback: a failing C-ABI call throws.
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "abi.hpp"
#include "c_api.h"
#include "clustering.hpp"
#include "icp.hpp"

namespace cilantro_hip {

// (ConstDataView, the non-owning view of a dim x n column-major float matrix, and the list helpers KDTree3f shares: abi.hpp)

// core/nearest_neighbors.hpp:49-77
struct KNNNeighborhoodSpecification {
  size_t maxNumberOfNeighbors;
  explicit KNNNeighborhoodSpecification(size_t k = 0) : maxNumberOfNeighbors(k) {}
};
template <typename ScalarT = float>
struct KNNInRadiusNeighborhoodSpecification {
  size_t maxNumberOfNeighbors;
  ScalarT radius;
  KNNInRadiusNeighborhoodSpecification(size_t k = 0, ScalarT radius_sq = (ScalarT)0) : maxNumberOfNeighbors(k), radius(radius_sq) {}
};

class KDTreeXf {
public:
  explicit KDTreeXf(const ConstDataView& points, int device = 0) : points_(points), device_(device) {}

  NeighborhoodSet kNNSearch(const ConstDataView& queries, size_t k) const { return knn(queries, k, std::numeric_limits<float>::infinity()); }
  NeighborhoodSet kNNInRadiusSearch(const ConstDataView& queries, size_t k, float radius) const { return knn(queries, k, radius); }
  // one query point (dim floats)
  Neighborhood kNNInRadiusSearch(const float* query, size_t k, float radius) const { return knn(ConstDataView(query, points_.rows(), 1), k, radius)[0]; }
  Neighborhood kNNSearch(const float* query, size_t k) const { return kNNInRadiusSearch(query, k, std::numeric_limits<float>::infinity()); }
  // the nearest point of every query; a query without one (a non-finite query, an empty tree) is left out of the set's list
  NeighborhoodSet nearestNeighborSearch(const ConstDataView& queries) const { return kNNSearch(queries, 1); }

  // every neighbour with squared distance < radius, ascending by (distance, index)
  NeighborhoodSet radiusSearch(const ConstDataView& queries, float radius) const {
    check(queries);
    const size_t nq = queries.cols();
    return detail::radius_lists(nq, "cilhip_radius_search_nd", [&](uint64_t* off, uint32_t* idx, float* d2, size_t capacity, size_t* total) {
      return cilhip_radius_search_nd(device_, points_.data(), points_.cols(), queries.data(), nq, points_.rows(), CILHIP_MEM_HOST, radius, off, idx, d2, capacity, total);
    });
  }

  // kd_tree.hpp:320-388: dispatch on the neighbourhood specification
  NeighborhoodSet search(const ConstDataView& queries, const KNNNeighborhoodSpecification& nh) const { return kNNSearch(queries, nh.maxNumberOfNeighbors); }
  NeighborhoodSet search(const ConstDataView& queries, const KNNInRadiusNeighborhoodSpecification<float>& nh) const {
    return kNNInRadiusSearch(queries, nh.maxNumberOfNeighbors, nh.radius);
  }
  NeighborhoodSet search(const ConstDataView& queries, const RadiusNeighborhoodSpecification<float>& nh) const { return radiusSearch(queries, nh.radius); }

  const ConstDataView& getPointsMatrixMap() const { return points_; }

private:
  void check(const ConstDataView& queries) const {
    if (queries.rows() != points_.rows()) throw std::invalid_argument("KDTree: the queries' dimension is not the tree's");
  }
  NeighborhoodSet knn(const ConstDataView& queries, size_t k, float radius) const {
    check(queries);
    const size_t nq = queries.cols();
    std::vector<uint32_t> idx(detail::room(nq * k)), cnt(detail::room(nq));
    std::vector<float> d2(detail::room(nq * k));
    detail::check(cilhip_knn_nd(device_, points_.data(), points_.cols(), queries.data(), nq, points_.rows(), CILHIP_MEM_HOST, k, radius, idx.data(), d2.data(), cnt.data()), "cilhip_knn_nd");
    return detail::lists_from_rows(idx, d2, cnt, nq, k);
  }
  ConstDataView points_;
  int device_;
};

class KDTree2f : public KDTreeXf {
public:
  explicit KDTree2f(const ConstDataView& points, int device = 0) : KDTreeXf(points, device) {
    if (points.rows() != 2) throw std::invalid_argument("KDTree2f: the points are not 2-D");
  }
  // n points as x0 y0 x1 y1 ...
  KDTree2f(const float* xy, size_t n, int device = 0) : KDTreeXf(ConstDataView(xy, 2, n), device) {}
};

}  // namespace cilantro_hip

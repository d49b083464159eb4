// cilantro_hip/abi.hpp -- what every header of this directory needs to cross the C ABI (c_api.h), written once; nothing here depends on
// more than c_api.h and the standard library:
//
//   ConstPointsView, ConstDataView                   the non-owning views of a 3 x n and of a dim x n column-major float matrix
//   Neighbor / Neighborhood / NeighborhoodSet        core/nearest_neighbors.hpp:7-47
//   RadiusNeighborhoodSpecification<float>           core/nearest_neighbors.hpp (the radius is a SQUARED distance)
//   detail::check                                    a return code of a call without a context -> std::runtime_error with the library's text
//   detail::room                                     the size of a buffer that must have an address even when it holds nothing
//   detail::ClusterMaps                              the ClusteringBase accessors (clustering/clustering_base.hpp:7-97) and the two ways labels arrive
//   detail::lists_from_rows / lists_from_csr / to_lists / radius_lists        a NeighborhoodSet from and to the arrays of the search entries
//
// (internal::check(ctx, ...) and internal::check_stateless, which map INVALID and UNSUPPORTED to std::invalid_argument, stay in icp.hpp.)
#pragma once

#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "c_api.h"

namespace cilantro_hip {

// core/data_containers.hpp:73-122: non-owning view of a 3xN column-major float matrix
struct ConstPointsView {
  const float* data_ = nullptr;
  size_t cols_ = 0;
  ConstPointsView() = default;
  ConstPointsView(const float* d, size_t n) : data_(d), cols_(n) {}
  ConstPointsView(const std::vector<float>& xyz) : data_(xyz.data()), cols_(xyz.size() / 3) {}
  const float* data() const { return data_; }
  size_t cols() const { return cols_; }
  static constexpr size_t rows() { return 3; }
};

// core/data_containers.hpp:73-122: non-owning view of a dim x n column-major float matrix
struct ConstDataView {
  const float* data_ = nullptr;
  size_t rows_ = 0, cols_ = 0;
  ConstDataView() = default;
  ConstDataView(const float* d, size_t dim, size_t n) : data_(d), rows_(dim), cols_(n) {}
  ConstDataView(const std::vector<float>& v, size_t dim) : data_(v.data()), rows_(dim), cols_(dim ? v.size() / dim : 0) {}
  const float* data() const { return data_; }
  size_t rows() const { return rows_; }
  size_t cols() const { return cols_; }
};

template <typename ScalarT = float>
struct RadiusNeighborhoodSpecification {
  ScalarT radius;      // squared
  explicit RadiusNeighborhoodSpecification(ScalarT radius_sq = (ScalarT)0) : radius(radius_sq) {}
};

// core/nearest_neighbors.hpp:7-47 (what the k-NN mirrors return and the warp-field classes take)
struct Neighbor {
  size_t index;
  float value;
};
typedef std::vector<Neighbor> Neighborhood;
typedef std::vector<Neighborhood> NeighborhoodSet;

namespace detail {

// A call that takes `int device` failed: std::runtime_error whatever the code, with the text the entry left for the calling thread.
inline void check(int rc, const char* entry) {
  if (rc != CILHIP_OK) throw std::runtime_error(std::string(entry) + " failed (rc " + std::to_string(rc) + "): " + cilhip_last_error(nullptr));
}

// An empty array still needs an address: the length of a buffer for n elements.
inline size_t room(size_t n) { return n ? n : 1; }

// clustering/clustering_base.hpp:7-97: the two maps of a clustering and their accessors
template <typename PointIndexT, typename ClusterIndexT>
class ClusterMaps {
public:
  typedef std::vector<std::vector<PointIndexT>> ClusterToPointIndicesMap;      // clustering_base.hpp:67-68
  typedef std::vector<ClusterIndexT> PointToClusterIndexMap;

  const ClusterToPointIndicesMap& getClusterToPointIndicesMap() const { return cluster_to_point_indices_map_; }
  const PointToClusterIndexMap& getPointToClusterIndexMap() const { return point_to_cluster_index_map_; }
  size_t getNumberOfClusters() const { return cluster_to_point_indices_map_.size(); }
  size_t getNumberOfPoints() const { return point_to_cluster_index_map_.size(); }

protected:
  // n labels and `count` clusters as CSR lists: cluster k is members[offsets[k] .. offsets[k + 1])
  void assign_csr(const std::vector<uint32_t>& labels, size_t n, const std::vector<uint32_t>& offsets, const std::vector<uint32_t>& members, size_t count) {
    cluster_to_point_indices_map_.assign(count, std::vector<PointIndexT>());
    for (size_t k = 0; k < count; ++k) cluster_to_point_indices_map_[k].assign(members.begin() + offsets[k], members.begin() + offsets[k + 1]);
    point_to_cluster_index_map_.assign(labels.begin(), labels.begin() + n);
  }
  // n labels below k: the lists follow from them, members ascending (clustering_base.hpp:22-33)
  void assign_labels(const std::vector<uint32_t>& labels, size_t n, size_t k) {
    point_to_cluster_index_map_.assign(labels.begin(), labels.begin() + n);
    cluster_to_point_indices_map_.assign(k, std::vector<PointIndexT>());
    for (size_t i = 0; i < n; ++i) cluster_to_point_indices_map_[labels[i]].push_back((PointIndexT)i);
  }
  // the points in a cluster (labeled) or in none: clustering_base.hpp:36-58
  std::vector<PointIndexT> select(bool labeled) const {
    std::vector<PointIndexT> res;
    const size_t k = getNumberOfClusters();
    for (size_t i = 0; i < point_to_cluster_index_map_.size(); ++i)
      if (((size_t)point_to_cluster_index_map_[i] < k) == labeled) res.push_back((PointIndexT)i);
    return res;
  }

  ClusterToPointIndicesMap cluster_to_point_indices_map_;
  PointToClusterIndexMap point_to_cluster_index_map_;
};

// the padded rows cilhip_knn3f / cilhip_knn_nd write (k entries per query, cnt[i] of them filled) as lists
inline NeighborhoodSet lists_from_rows(const std::vector<uint32_t>& idx, const std::vector<float>& d2, const std::vector<uint32_t>& cnt, size_t nq, size_t k) {
  NeighborhoodSet out(nq);
  for (size_t i = 0; i < nq; ++i) {
    out[i].resize(cnt[i]);
    for (size_t j = 0; j < cnt[i]; ++j) out[i][j] = Neighbor{(size_t)idx[i * k + j], d2[i * k + j]};
  }
  return out;
}

// the CSR lists cilhip_radius_search3f / _nd write as lists
inline NeighborhoodSet lists_from_csr(const std::vector<uint64_t>& off, const std::vector<uint32_t>& idx, const std::vector<float>& d2, size_t nq) {
  NeighborhoodSet out(nq);
  for (size_t i = 0; i < nq; ++i) {
    out[i].resize((size_t)(off[i + 1] - off[i]));
    for (size_t j = 0; j < out[i].size(); ++j) out[i][j] = Neighbor{(size_t)idx[off[i] + j], d2[off[i] + j]};
  }
  return out;
}

// the inverse of lists_from_rows: a NeighborhoodSet as padded rows (k = the longest list, at least 1; the padding names no point)
inline size_t to_lists(const NeighborhoodSet& nh, std::vector<uint32_t>& idx, std::vector<float>& d2) {
  size_t k = 1;
  for (const auto& l : nh) k = l.size() > k ? l.size() : k;
  idx.assign(room(nh.size() * k), 0xFFFFFFFFu);
  d2.assign(idx.size(), 0.0f);
  for (size_t i = 0; i < nh.size(); ++i)
    for (size_t j = 0; j < nh[i].size(); ++j) { idx[i * k + j] = (uint32_t)nh[i][j].index; d2[i * k + j] = nh[i][j].value; }
  return k;
}

// A radius search in its two passes: the counts, then (unless nothing was found) the lists.
// search(offsets, idx_or_null, d2_or_null, capacity, &total) is the entry with everything else bound.
template <class SearchT>
NeighborhoodSet radius_lists(size_t nq, const char* entry, const SearchT& search) {
  std::vector<uint64_t> off(nq + 1, 0);
  size_t total = 0;
  check(search(off.data(), (uint32_t*)nullptr, (float*)nullptr, (size_t)0, &total), entry);
  std::vector<uint32_t> idx(room(total));
  std::vector<float> d2(room(total));
  if (total) check(search(off.data(), idx.data(), d2.data(), total, &total), entry);
  return lists_from_csr(off, idx, d2, nq);
}

}  // namespace detail

}  // namespace cilantro_hip

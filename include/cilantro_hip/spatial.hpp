// cilantro_hip/spatial.hpp -- header-only C++ mirror of cilantro's spatial module (spatial/convex_polytope.hpp, flat_convex_hull_3d.hpp,
// space_region.hpp) for float in 2 and 3 dimensions, on top of the C ABI (cilhip_convex_hull_* and cilhip_polytope(s)_*; c_api.h rules
// H1-H5 and Q1-Q2):
//   ConvexPolytope<float, Dim> / 2f / 3f, also named ConvexHull2f / 3f;  FlatConvexHull3f;  SpaceRegion<float, Dim> / 2f / 3f
// Points are point-major float arrays on the host: n x dim, the reference's column-major dim x n.  Halfspaces are (dim + 1) x F
// column-major as in the reference: halfspace k is [k * (dim + 1), (k + 1) * (dim + 1)).
// Not built: the halfspace constructor's vertex enumeration, intersectionWith, SpaceRegion::complement / relativeComplement / getVolume --
// they need the QP of convex_hull_utilities.hpp:12-193 and a dual hull; these throw.  fromHalfspaces gives a polytope for queries only.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "abi.hpp"
#include "c_api.h"
#include "principal_component_analysis.hpp"

namespace cilantro_hip {

namespace spatial_detail {
inline const char* not_built() { return "not built: it needs the QP of convex_hull_utilities.hpp:12-193 and a dual hull"; }
}  // namespace spatial_detail

template <typename ScalarT = float, std::ptrdiff_t EigenDim = 3, typename IndexT = size_t>
class ConvexPolytope {
  static_assert(sizeof(ScalarT) == sizeof(float), "the device path is built for float");
  static_assert(EigenDim == 2 || EigenDim == 3, "built for 2 and 3 dimensions");

 public:
  static constexpr size_t Dim = (size_t)EigenDim;

  // the empty polytope (convex_polytope.hpp:14-25)
  ConvexPolytope() { build(nullptr, 0, false, false, 0.0); }
  // the points constructor (:40-45)
  ConvexPolytope(const float* points, size_t n, bool compute_topology = false, bool simplicial_facets = false, double merge_tol = 0.0, int device = 0) : device_(device) {
    build(points, n, compute_topology, simplicial_facets, merge_tol);
  }
  ConvexPolytope(const std::vector<float>& points, bool compute_topology = false, bool simplicial_facets = false, double merge_tol = 0.0, int device = 0)
      : ConvexPolytope(points.data(), points.size() / Dim, compute_topology, simplicial_facets, merge_tol, device) {}
  // (dim + 1) x F halfspaces, nrm . x + off <= 0 inside: for the point queries and transform only
  static ConvexPolytope fromHalfspaces(const std::vector<float>& halfspaces, int device = 0) {
    ConvexPolytope p;
    p.device_ = device; p.queries_only_ = true; p.is_empty_ = false; p.is_bounded_ = false;
    p.halfspaces_ = halfspaces;
    p.area_ = p.volume_ = std::numeric_limits<double>::quiet_NaN();
    return p;
  }

  ConvexPolytope intersectionWith(const ConvexPolytope&, bool = false, bool = false, double = 0.0, double = 0.0) const {
    throw std::runtime_error(std::string("ConvexPolytope::intersectionWith is ") + spatial_detail::not_built());
  }

  size_t getSpaceDimension() const { return Dim; }
  bool isEmpty() const { return is_empty_; }
  bool isBounded() const { no_vertices(); return is_bounded_; }
  double getArea() const { no_vertices(); return area_; }
  double getVolume() const { no_vertices(); return volume_; }
  const std::vector<float>& getVertices() const { no_vertices(); return vertices_; }
  const std::vector<float>& getFacetHyperplanes() const { return halfspaces_; }
  const std::vector<float>& getInteriorPoint() const { no_vertices(); return interior_point_; }
  const std::vector<std::vector<IndexT>>& getFacetVertexIndices() const { return faces_; }
  const std::vector<std::vector<IndexT>>& getVertexNeighborFacets() const { return vertex_neighbor_faces_; }
  const std::vector<std::vector<IndexT>>& getFacetNeighborFacets() const { return face_neighbor_faces_; }
  const std::vector<IndexT>& getVertexPointIndices() const { return vertex_point_indices_; }
  size_t numFacets() const { return halfspaces_.size() / (Dim + 1); }
  // what the device did: rounds, survivors of the first cull, plane tests ...
  const cilhip_hull_info& getInfo() const { return info_; }

  // :109-115, on the host
  bool containsPoint(const float* p, float offset = 0.0f) const {
    for (size_t k = 0; k < numFacets(); ++k) {
      const float* h = halfspaces_.data() + k * (Dim + 1);
      volatile float v = h[0] * p[0];
      volatile float w = h[1] * p[1];
      v = v + w;
      if (Dim == 3) { w = h[2] * p[2]; v = v + w; }
      v = v + h[Dim];
      if (v > -offset) return false;
    }
    return true;
  }
  // :117-121 -> F x n, row-major
  std::vector<float> getPointSignedDistancesFromFacets(const float* points, size_t n) const {
    std::vector<float> out(numFacets() * n);
    detail::check(cilhip_polytope_signed_distances(device_, halfspaces_.data(), numFacets(), points, n, Dim, CILHIP_MEM_HOST, out.data()), "cilhip_polytope_signed_distances");
    return out;
  }
  std::vector<bool> getInteriorPointsIndexMask(const float* points, size_t n, float offset = 0.0f) const {
    const uint32_t offs[2] = {0u, (uint32_t)numFacets()};
    std::vector<uint8_t> m(n);
    detail::check(cilhip_polytopes_interior_mask(device_, halfspaces_.data(), offs, 1, points, n, Dim, CILHIP_MEM_HOST, offset, m.data()), "cilhip_polytopes_interior_mask");
    return std::vector<bool>(m.begin(), m.end());
  }
  template <typename IdxT = IndexT> std::vector<IdxT> getInteriorPointIndices(const float* points, size_t n, float offset = 0.0f) const {
    const uint32_t offs[2] = {0u, (uint32_t)numFacets()};
    std::vector<uint32_t> idx(detail::room(n));
    size_t count = 0;
    detail::check(cilhip_polytopes_interior_indices(device_, halfspaces_.data(), offs, 1, points, n, Dim, CILHIP_MEM_HOST, offset, idx.data(), idx.size(), &count),
                          "cilhip_polytopes_interior_indices");
    return std::vector<IdxT>(idx.begin(), idx.begin() + count);
  }

  // :155-174, host f32: rotation is Dim x Dim row-major, translation Dim
  ConvexPolytope& transform(const float* R, const float* t) {
    if (is_empty_) return *this;
    auto apply = [&](float* p) {
      float q[3] = {0, 0, 0};
      for (size_t r = 0; r < Dim; ++r) { for (size_t c = 0; c < Dim; ++c) q[r] += R[r * Dim + c] * p[c]; q[r] += t[r]; }
      for (size_t r = 0; r < Dim; ++r) p[r] = q[r];
    };
    for (size_t k = 0; k < vertices_.size() / Dim; ++k) apply(vertices_.data() + k * Dim);
    if (interior_point_.size() == Dim) apply(interior_point_.data());
    float tr[3] = {0, 0, 0};      // -t^T R
    for (size_t c = 0; c < Dim; ++c) { for (size_t r = 0; r < Dim; ++r) tr[c] += t[r] * R[r * Dim + c]; tr[c] = -tr[c]; }
    for (size_t k = 0; k < numFacets(); ++k) {
      float* h = halfspaces_.data() + k * (Dim + 1);
      float q[4] = {0, 0, 0, 0};
      for (size_t r = 0; r < Dim; ++r) for (size_t c = 0; c < Dim; ++c) q[r] += R[r * Dim + c] * h[c];
      for (size_t c = 0; c < Dim; ++c) q[Dim] += tr[c] * h[c];
      q[Dim] += h[Dim];
      for (size_t r = 0; r <= Dim; ++r) h[r] = q[r];
    }
    return *this;
  }
  // a (Dim + 1) x (Dim + 1) row-major matrix (:176-181)
  ConvexPolytope& transform(const float* T) {
    float R[9], t[3];
    for (size_t r = 0; r < Dim; ++r) { for (size_t c = 0; c < Dim; ++c) R[r * Dim + c] = T[r * (Dim + 1) + c]; t[r] = T[r * (Dim + 1) + Dim]; }
    return transform(R, t);
  }
  ConvexPolytope transformed(const float* T) const { ConvexPolytope r = *this; r.transform(T); return r; }
  ConvexPolytope transformed(const float* R, const float* t) const { ConvexPolytope r = *this; r.transform(R, t); return r; }

 private:
  int device_ = 0;
  bool is_empty_ = true, is_bounded_ = true, queries_only_ = false;
  double area_ = 0.0, volume_ = 0.0;
  std::vector<float> vertices_, halfspaces_, interior_point_;
  std::vector<std::vector<IndexT>> faces_, vertex_neighbor_faces_, face_neighbor_faces_;
  std::vector<IndexT> vertex_point_indices_;
  cilhip_hull_info info_{};

  void no_vertices() const {
    if (queries_only_) throw std::runtime_error(std::string("a polytope given by halfspaces has no vertices here: the vertex enumeration is ") + spatial_detail::not_built());
  }

  void build(const float* points, size_t n, bool compute_topology, bool simplicial_facets, double merge_tol) {
    const float none = 0.0f;
    cilhip_hull* h = nullptr;
    detail::check(cilhip_convex_hull_create(device_, n ? points : &none, n, Dim, CILHIP_MEM_HOST, simplicial_facets ? 1 : 0, merge_tol, &h, &info_), "cilhip_convex_hull_create");
    const size_t V = info_.n_vertices, F = info_.n_facets;
    std::vector<uint32_t> vpi(V), fo(F + 1), fi(info_.n_facet_indices), fn(info_.n_facet_indices), vo(V + 1), vf(info_.n_vertex_facets);
    vertices_.assign(V * Dim, 0.0f);
    halfspaces_.assign(info_.n_halfspaces * (Dim + 1), 0.0f);
    const int rc = cilhip_convex_hull_get(h, vpi.data(), vertices_.data(), halfspaces_.data(), fo.data(), fi.data(), fn.data(), vo.data(), vf.data(), nullptr);
    cilhip_convex_hull_destroy(h);
    detail::check(rc, "cilhip_convex_hull_get");
    is_empty_ = info_.is_empty != 0;
    area_ = info_.area; volume_ = info_.volume;
    interior_point_.assign(info_.interior_point, info_.interior_point + Dim);
    if (!compute_topology) return;
    vertex_point_indices_.assign(vpi.begin(), vpi.end());
    faces_.resize(F); face_neighbor_faces_.resize(F); vertex_neighbor_faces_.resize(V);
    for (size_t k = 0; k < F; ++k) { faces_[k].assign(fi.begin() + fo[k], fi.begin() + fo[k + 1]); face_neighbor_faces_[k].assign(fn.begin() + fo[k], fn.begin() + fo[k + 1]); }
    for (size_t v = 0; v < V; ++v) vertex_neighbor_faces_[v].assign(vf.begin() + vo[v], vf.begin() + vo[v + 1]);
  }
};

using ConvexPolytope2f = ConvexPolytope<float, 2>;
using ConvexPolytope3f = ConvexPolytope<float, 3>;
template <typename ScalarT, std::ptrdiff_t EigenDim, typename IndexT = size_t> using ConvexHull = ConvexPolytope<ScalarT, EigenDim, IndexT>;
using ConvexHull2f = ConvexPolytope2f;
using ConvexHull3f = ConvexPolytope3f;

// flat_convex_hull_3d.hpp: the 2-D hull of the projection on the two leading principal directions
class FlatConvexHull3f {
 public:
  FlatConvexHull3f(const float* points, size_t n, bool compute_topology = true, bool simplicial_facets = true, double merge_tol = 0.0, int device = 0)
      : pca_(points, n, 3, device), flat_(pca_.project(points, n, 2)), hull_(flat_.data(), n, compute_topology, simplicial_facets, merge_tol, device) {
    const std::vector<float>& v2 = hull_.getVertices();
    if (!v2.empty()) vertices_3d_ = pca_.reconstruct(v2.data(), v2.size() / 2, 2);
  }
  const ConvexHull2f& getHull2D() const { return hull_; }
  const std::vector<float>& getVertices2D() const { return hull_.getVertices(); }
  const std::vector<float>& getVertices3D() const { return vertices_3d_; }
  const std::vector<size_t>& getVertexPointIndices() const { return hull_.getVertexPointIndices(); }
  bool isEmpty() const { return hull_.isEmpty(); }
  double getArea() const { return hull_.getArea(); }
  double getVolume() const { return hull_.getVolume(); }
  // the 3-D vertices by (R, t); the 2-D hull lives in the plane's own frame and stays
  FlatConvexHull3f& transform(const float* R, const float* t) {
    for (size_t k = 0; k < vertices_3d_.size() / 3; ++k) {
      float* p = vertices_3d_.data() + 3 * k;
      float q[3];
      for (int r = 0; r < 3; ++r) q[r] = R[3 * r] * p[0] + R[3 * r + 1] * p[1] + R[3 * r + 2] * p[2] + t[r];
      p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
    return *this;
  }

 private:
  PrincipalComponentAnalysis3f pca_;
  std::vector<float> flat_;
  ConvexHull2f hull_;
  std::vector<float> vertices_3d_;
};

template <typename ScalarT = float, std::ptrdiff_t EigenDim = 3, typename IndexT = size_t>
class SpaceRegion {
 public:
  using Polytope = ConvexPolytope<ScalarT, EigenDim, IndexT>;
  static constexpr size_t Dim = (size_t)EigenDim;

  SpaceRegion() = default;
  explicit SpaceRegion(const std::vector<Polytope>& polytopes, int device = 0) : device_(device), polytopes_(polytopes) {}
  explicit SpaceRegion(const Polytope& polytope, int device = 0) : device_(device), polytopes_(1, polytope) {}

  SpaceRegion unionWith(const SpaceRegion& sr) const {
    std::vector<Polytope> res(polytopes_);
    res.insert(res.end(), sr.polytopes_.begin(), sr.polytopes_.end());
    return SpaceRegion(res, device_);
  }
  SpaceRegion intersectionWith(const SpaceRegion&, bool = false, bool = false, double = 0.0, double = 0.0) const {
    throw std::runtime_error(std::string("SpaceRegion::intersectionWith is ") + spatial_detail::not_built());
  }
  SpaceRegion complement(bool = false, bool = false, double = 0.0, double = 0.0) const { throw std::runtime_error(std::string("SpaceRegion::complement is ") + spatial_detail::not_built()); }
  SpaceRegion relativeComplement(const SpaceRegion&, bool = false, bool = false, double = 0.0, double = 0.0) const {
    throw std::runtime_error(std::string("SpaceRegion::relativeComplement is ") + spatial_detail::not_built());
  }
  double getVolume(double = 0.0, double = 0.0) const { throw std::runtime_error(std::string("SpaceRegion::getVolume is ") + spatial_detail::not_built()); }

  size_t getSpaceDimension() const { return Dim; }
  bool isEmpty() const { for (const Polytope& p : polytopes_) if (!p.isEmpty()) return false; return true; }
  bool isBounded() const { for (const Polytope& p : polytopes_) if (!p.isBounded()) return false; return true; }
  const std::vector<Polytope>& getConvexPolytopes() const { return polytopes_; }
  std::vector<float> getInteriorPoint() const {
    for (const Polytope& p : polytopes_) if (!p.isEmpty()) return p.getInteriorPoint();
    return std::vector<float>(Dim, std::numeric_limits<float>::quiet_NaN());
  }
  bool containsPoint(const float* point, float offset = 0.0f) const {
    for (const Polytope& p : polytopes_) if (p.containsPoint(point, offset)) return true;
    return false;
  }
  std::vector<bool> getInteriorPointsIndexMask(const float* points, size_t n, float offset = 0.0f) const {
    std::vector<float> hs;
    std::vector<uint32_t> offs;
    pack(hs, offs);
    std::vector<uint8_t> m(n);
    detail::check(cilhip_polytopes_interior_mask(device_, hs.data(), offs.data(), polytopes_.size(), points, n, Dim, CILHIP_MEM_HOST, offset, m.data()), "cilhip_polytopes_interior_mask");
    return std::vector<bool>(m.begin(), m.end());
  }
  template <typename IdxT = IndexT> std::vector<IdxT> getInteriorPointIndices(const float* points, size_t n, float offset = 0.0f) const {
    std::vector<float> hs;
    std::vector<uint32_t> offs;
    pack(hs, offs);
    std::vector<uint32_t> idx(detail::room(n));
    size_t count = 0;
    detail::check(cilhip_polytopes_interior_indices(device_, hs.data(), offs.data(), polytopes_.size(), points, n, Dim, CILHIP_MEM_HOST, offset, idx.data(), idx.size(), &count),
                          "cilhip_polytopes_interior_indices");
    return std::vector<IdxT>(idx.begin(), idx.begin() + count);
  }
  SpaceRegion& transform(const float* R, const float* t) { for (Polytope& p : polytopes_) p.transform(R, t); return *this; }
  SpaceRegion& transform(const float* T) { for (Polytope& p : polytopes_) p.transform(T); return *this; }
  SpaceRegion transformed(const float* T) const { SpaceRegion r = *this; r.transform(T); return r; }
  SpaceRegion transformed(const float* R, const float* t) const { SpaceRegion r = *this; r.transform(R, t); return r; }

 private:
  int device_ = 0;
  std::vector<Polytope> polytopes_;

  void pack(std::vector<float>& hs, std::vector<uint32_t>& offs) const {
    offs.assign(1, 0u);
    for (const Polytope& p : polytopes_) {
      hs.insert(hs.end(), p.getFacetHyperplanes().begin(), p.getFacetHyperplanes().end());
      offs.push_back((uint32_t)(hs.size() / (Dim + 1)));
    }
    if (hs.empty()) hs.push_back(0.0f);
  }
};

using SpaceRegion2f = SpaceRegion<float, 2>;
using SpaceRegion3f = SpaceRegion<float, 3>;

}  // namespace cilantro_hip

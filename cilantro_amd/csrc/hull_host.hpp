// hull_host.hpp -- the combinatorial half of the convex hull: plain C++, no HIP.  The device finds the few extreme
// points among n (convex_hull.hip); everything here runs over that candidate list, in f64 on the f32 coordinates.
//   hull_tol          the band: max(merge_tol, 2^-44 M)
//   hull_plane3 / 2   the facet plane of (a, b, c) / the outward line of the edge (a, b); hull_dist: nrm . p + off, positive outside
//   hull_build        candidates -> HullResult: exact duplicates dropped (the lowest index stays), an incremental hull with the band
//                     (a point is added iff some facet has d > tol; the facets it replaces are those reached from the farthest one with
//                     d >= -tol, so that a point in a neighbour's plane never leaves a sliver), the merge of coplanar triangles into
//                     polygons, the removal of vertices only two polygons meet at, the canonical order, area and volume
//                     Candidates of rank < dim give `bootstrap` instead: planes through their flat, both ways, for the device to find
//                     a point off it.
// Every expression that decides something is written out (no fma, fixed association) and is evaluated the same way on the device.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <unordered_map>
#include <vector>

namespace cilhip {

struct HullPlane { double n[3]; double off; };

inline double hull_tol(double merge_tol, double M) { return std::max(merge_tol, std::ldexp(M, -44)); }

inline double hull_dist(const HullPlane& h, const double* p) { return ((h.n[0] * p[0] + h.n[1] * p[1]) + h.n[2] * p[2]) + h.off; }

inline HullPlane hull_plane3(const double* a, const double* b, const double* c) {
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const double x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
  const double len = std::sqrt((x * x + y * y) + z * z);
  HullPlane h;
  h.n[0] = x / len; h.n[1] = y / len; h.n[2] = z / len;
  h.off = -((h.n[0] * a[0] + h.n[1] * a[1]) + h.n[2] * a[2]);
  return h;
}
// the edge a -> b of a counter-clockwise polygon: the interior on its left, the normal to its right
inline HullPlane hull_plane2(const double* a, const double* b) {
  const double x = b[1] - a[1], y = -(b[0] - a[0]);
  const double len = std::sqrt(x * x + y * y);
  HullPlane h;
  h.n[0] = x / len; h.n[1] = y / len; h.n[2] = 0.0;
  h.off = -(h.n[0] * a[0] + h.n[1] * a[1]);
  return h;
}
inline HullPlane hull_plane_through(const double* a, double nx, double ny, double nz) {
  HullPlane h;
  h.n[0] = nx; h.n[1] = ny; h.n[2] = nz;
  h.off = -((nx * a[0] + ny * a[1]) + nz * a[2]);
  return h;
}

struct HullResult {
  int dim = 3;
  bool empty = true;
  bool failed = false;                        // the builder met a surface it cannot order (never seen; reported, not hidden)
  int rank = 0;                               // of the candidates: dim = full
  std::vector<HullPlane> bootstrap;           // rank < dim: planes through the candidates' flat
  std::vector<uint32_t> vertex_ids;           // positions in the candidate list, ascending
  std::vector<uint32_t> facet_offsets, facet_indices, facet_neighbors, vertex_facet_offsets, vertex_facets;
  std::vector<HullPlane> planes;              // one per facet
  double area = 0.0, volume = 0.0;
  float interior[3] = {0, 0, 0};
};

namespace hull_detail {

using Poly = std::vector<uint32_t>;

inline uint64_t ekey(uint32_t a, uint32_t b) { return ((uint64_t)a << 32) | b; }

// polygons (counter-clockwise from outside, positions in the candidate list) -> the canonical lists of section 20
inline void finish3(const double* P, std::vector<Poly>& polys, bool simplicial, HullResult& r) {
  // the vertices, ascending
  std::vector<uint32_t> vs;
  for (const Poly& p : polys) vs.insert(vs.end(), p.begin(), p.end());
  std::sort(vs.begin(), vs.end());
  vs.erase(std::unique(vs.begin(), vs.end()), vs.end());
  r.vertex_ids = vs;
  auto local = [&](uint32_t v) { return (uint32_t)(std::lower_bound(vs.begin(), vs.end(), v) - vs.begin()); };
  std::vector<Poly> facets;
  for (Poly& p : polys) {
    for (uint32_t& v : p) v = local(v);
    std::rotate(p.begin(), std::min_element(p.begin(), p.end()), p.end());
    if (simplicial) {
      for (size_t i = 1; i + 1 < p.size(); ++i) facets.push_back({p[0], p[i], p[i + 1]});
    } else {
      facets.push_back(p);
    }
  }
  std::sort(facets.begin(), facets.end());
  const size_t F = facets.size(), V = vs.size();
  // interior point: the f32 mean of the vertices, summed in vertex order
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (size_t k = 0; k < V; ++k)
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (float)P[3 * (size_t)vs[k] + c];
  for (int c = 0; c < 3; ++c) r.interior[c] = acc[c] / (float)V;
  const double c0[3] = {(double)r.interior[0], (double)r.interior[1], (double)r.interior[2]};
  auto pt = [&](uint32_t lv) { return P + 3 * (size_t)vs[lv]; };
  r.facet_offsets.assign(1, 0u);
  r.area = 0.0; r.volume = 0.0;
  std::unordered_map<uint64_t, uint32_t> owner;
  for (size_t k = 0; k < F; ++k) {
    const Poly& f = facets[k];
    // the plane: of the fan triangle with the smallest sorted index triple (the facet itself when it is a triangle)
    size_t best = 1;
    for (size_t i = 2; i + 1 < f.size(); ++i) {
      const uint32_t lo = std::min(f[i], f[i + 1]), hi = std::max(f[i], f[i + 1]), blo = std::min(f[best], f[best + 1]), bhi = std::max(f[best], f[best + 1]);
      if (lo < blo || (lo == blo && hi < bhi)) best = i;
    }
    r.planes.push_back(hull_plane3(pt(f[0]), pt(f[best]), pt(f[best + 1])));
    for (size_t i = 1; i + 1 < f.size(); ++i) {
      const double *a = pt(f[0]), *b = pt(f[i]), *c = pt(f[i + 1]);
      const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
      const double x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
      r.area += 0.5 * std::sqrt((x * x + y * y) + z * z);
      const double A[3] = {a[0] - c0[0], a[1] - c0[1], a[2] - c0[2]}, B[3] = {b[0] - c0[0], b[1] - c0[1], b[2] - c0[2]}, C[3] = {c[0] - c0[0], c[1] - c0[1], c[2] - c0[2]};
      const double bx = B[1] * C[2] - B[2] * C[1], by = B[2] * C[0] - B[0] * C[2], bz = B[0] * C[1] - B[1] * C[0];
      r.volume += ((A[0] * bx + A[1] * by) + A[2] * bz) / 6.0;
    }
    for (size_t j = 0; j < f.size(); ++j) {
      r.facet_indices.push_back(f[j]);
      owner[ekey(f[j], f[(j + 1) % f.size()])] = (uint32_t)k;
    }
    r.facet_offsets.push_back((uint32_t)r.facet_indices.size());
  }
  std::vector<std::vector<uint32_t>> vf(V);
  for (size_t k = 0; k < F; ++k) {
    const Poly& f = facets[k];
    for (size_t j = 0; j < f.size(); ++j) {
      const auto it = owner.find(ekey(f[(j + 1) % f.size()], f[j]));
      if (it == owner.end()) { r.failed = true; return; }
      r.facet_neighbors.push_back(it->second);
      vf[f[j]].push_back((uint32_t)k);
    }
  }
  r.vertex_facet_offsets.assign(1, 0u);
  for (size_t v = 0; v < V; ++v) {
    r.vertex_facets.insert(r.vertex_facets.end(), vf[v].begin(), vf[v].end());
    r.vertex_facet_offsets.push_back((uint32_t)r.vertex_facets.size());
  }
  r.empty = false;
}

// triangles (counter-clockwise from outside) -> polygons: coplanar neighbours merged, vertices only two polygons meet at removed
inline bool merge3(const double* P, const std::vector<uint32_t>& tri, double tol, std::vector<Poly>& polys) {
  const size_t T = tri.size() / 3;
  std::unordered_map<uint64_t, uint32_t> owner;
  owner.reserve(3 * T);
  for (size_t t = 0; t < T; ++t)
    for (int j = 0; j < 3; ++j) owner[ekey(tri[3 * t + j], tri[3 * t + (j + 1) % 3])] = (uint32_t)(3 * t + j);
  std::vector<HullPlane> pl(T);
  for (size_t t = 0; t < T; ++t) pl[t] = hull_plane3(P + 3 * (size_t)tri[3 * t], P + 3 * (size_t)tri[3 * t + 1], P + 3 * (size_t)tri[3 * t + 2]);
  std::vector<uint32_t> parent(T);
  for (size_t t = 0; t < T; ++t) parent[t] = (uint32_t)t;
  auto find = [&](uint32_t x) { while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; } return x; };
  for (size_t t = 0; t < T; ++t)
    for (int j = 0; j < 3; ++j) {
      const auto it = owner.find(ekey(tri[3 * t + (j + 1) % 3], tri[3 * t + j]));
      if (it == owner.end()) return false;
      const size_t u = it->second / 3, ju = it->second % 3;
      if (u <= t) continue;
      const uint32_t opp_t = tri[3 * t + (j + 2) % 3], opp_u = tri[3 * u + (ju + 2) % 3];
      if (std::fabs(hull_dist(pl[u], P + 3 * (size_t)opp_t)) <= tol && std::fabs(hull_dist(pl[t], P + 3 * (size_t)opp_u)) <= tol) {
        const uint32_t a = find((uint32_t)t), b = find((uint32_t)u);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);
      }
    }
  // the boundary of every group: next vertex after a, per group
  std::unordered_map<uint32_t, std::unordered_map<uint32_t, uint32_t>> next;
  std::vector<uint32_t> roots;
  for (size_t t = 0; t < T; ++t) {
    const uint32_t g = find((uint32_t)t);
    if (g == t) roots.push_back(g);
    for (int j = 0; j < 3; ++j) {
      const uint32_t a = tri[3 * t + j], b = tri[3 * t + (j + 1) % 3];
      const uint32_t u = owner[ekey(b, a)] / 3;
      if (find(u) == g) continue;
      auto& m = next[g];
      if (m.count(a)) return false;      // (a pinched boundary)
      m[a] = b;
    }
  }
  polys.clear();
  for (const uint32_t g : roots) {
    const auto& m = next[g];
    if (m.size() < 3) return false;
    uint32_t start = m.begin()->first;
    for (const auto& kv : m) start = std::min(start, kv.first);
    Poly p;
    uint32_t v = start;
    do {
      p.push_back(v);
      const auto it = m.find(v);
      if (it == m.end() || p.size() > m.size()) return false;
      v = it->second;
    } while (v != start);
    if (p.size() != m.size()) return false;      // (more than one boundary cycle)
    polys.push_back(std::move(p));
  }
  // a vertex only two polygons meet at lies on their common edge: not a vertex
  std::unordered_map<uint32_t, int> deg;
  for (const Poly& p : polys) for (const uint32_t v : p) ++deg[v];
  for (Poly& p : polys) {
    p.erase(std::remove_if(p.begin(), p.end(), [&](uint32_t v) { return deg[v] < 3; }), p.end());
    if (p.size() < 3) return false;
  }
  return true;
}

struct Tri { uint32_t v[3]; HullPlane pl; bool alive; };

inline void build3(const double* P, const std::vector<uint32_t>& act, double tol, bool simplicial, HullResult& r) {
  auto pt = [&](uint32_t i) { return P + 3 * (size_t)i; };
  // the initial simplex: lowest x, farthest from it, farthest from their line, farthest from their plane
  uint32_t a = act[0];
  for (const uint32_t i : act) if (pt(i)[0] < pt(a)[0]) a = i;
  auto d2 = [&](uint32_t i, uint32_t j) { const double x = pt(i)[0] - pt(j)[0], y = pt(i)[1] - pt(j)[1], z = pt(i)[2] - pt(j)[2]; return (x * x + y * y) + z * z; };
  uint32_t b = a;
  for (const uint32_t i : act) if (d2(i, a) > d2(b, a)) b = i;
  if (std::sqrt(d2(b, a)) <= tol) {
    r.rank = 0;
    for (int c = 0; c < 3; ++c)
      for (int sgn = 1; sgn >= -1; sgn -= 2) r.bootstrap.push_back(hull_plane_through(pt(a), c == 0 ? sgn : 0.0, c == 1 ? sgn : 0.0, c == 2 ? sgn : 0.0));
    return;
  }
  const double lab = std::sqrt(d2(b, a));
  const double u[3] = {(pt(b)[0] - pt(a)[0]) / lab, (pt(b)[1] - pt(a)[1]) / lab, (pt(b)[2] - pt(a)[2]) / lab};
  auto line_d = [&](uint32_t i) {
    const double w[3] = {pt(i)[0] - pt(a)[0], pt(i)[1] - pt(a)[1], pt(i)[2] - pt(a)[2]};
    const double x = u[1] * w[2] - u[2] * w[1], y = u[2] * w[0] - u[0] * w[2], z = u[0] * w[1] - u[1] * w[0];
    return std::sqrt((x * x + y * y) + z * z);
  };
  uint32_t c = a;
  double best = 0.0;
  for (const uint32_t i : act) { const double d = line_d(i); if (d > best) { best = d; c = i; } }
  if (best <= tol) {
    r.rank = 1;
    int ax = 0;
    for (int k = 1; k < 3; ++k) if (std::fabs(u[k]) < std::fabs(u[ax])) ax = k;
    const double e[3] = {ax == 0 ? 1.0 : 0.0, ax == 1 ? 1.0 : 0.0, ax == 2 ? 1.0 : 0.0};
    double n1[3] = {u[1] * e[2] - u[2] * e[1], u[2] * e[0] - u[0] * e[2], u[0] * e[1] - u[1] * e[0]};
    const double l1 = std::sqrt((n1[0] * n1[0] + n1[1] * n1[1]) + n1[2] * n1[2]);
    for (double& x : n1) x /= l1;
    const double n2[3] = {u[1] * n1[2] - u[2] * n1[1], u[2] * n1[0] - u[0] * n1[2], u[0] * n1[1] - u[1] * n1[0]};
    for (int sgn = 1; sgn >= -1; sgn -= 2) {
      r.bootstrap.push_back(hull_plane_through(pt(a), sgn * n1[0], sgn * n1[1], sgn * n1[2]));
      r.bootstrap.push_back(hull_plane_through(pt(a), sgn * n2[0], sgn * n2[1], sgn * n2[2]));
    }
    return;
  }
  HullPlane base = hull_plane3(pt(a), pt(b), pt(c));
  uint32_t d = a;
  best = 0.0;
  for (const uint32_t i : act) { const double h = std::fabs(hull_dist(base, pt(i))); if (h > best) { best = h; d = i; } }
  if (best <= tol) {
    r.rank = 2;
    r.bootstrap.push_back(base);
    r.bootstrap.push_back(hull_plane3(pt(a), pt(c), pt(b)));
    return;
  }
  r.rank = 3;
  if (hull_dist(base, pt(d)) > 0.0) std::swap(b, c);      // d below (a, b, c)

  std::vector<Tri> tris;
  std::vector<uint32_t> free_slots;
  std::unordered_map<uint64_t, uint32_t> owner;      // directed edge -> triangle
  auto add = [&](uint32_t x, uint32_t y, uint32_t z) {
    Tri t;
    t.v[0] = x; t.v[1] = y; t.v[2] = z;
    t.pl = hull_plane3(pt(x), pt(y), pt(z));
    t.alive = true;
    uint32_t id;
    if (!free_slots.empty()) { id = free_slots.back(); free_slots.pop_back(); tris[id] = t; } else { id = (uint32_t)tris.size(); tris.push_back(t); }
    for (int j = 0; j < 3; ++j) owner[ekey(t.v[j], t.v[(j + 1) % 3])] = id;
  };
  add(a, b, c); add(a, d, b); add(b, d, c); add(c, d, a);

  std::vector<uint32_t> stack, visible;
  std::vector<int> seen;      // per slot: the insertion that last visited it (0: none), negative: visited and not visible
  std::vector<std::pair<uint32_t, uint32_t>> horizon;
  int stamp = 0;
  for (const uint32_t p : act) {
    if (p == a || p == b || p == c || p == d) continue;
    int far = -1;
    double dfar = tol;
    for (size_t t = 0; t < tris.size(); ++t)
      if (tris[t].alive) { const double h = hull_dist(tris[t].pl, pt(p)); if (h > dfar) { dfar = h; far = (int)t; } }
    if (far < 0) continue;
    ++stamp;
    seen.resize(tris.size(), 0);
    stack.assign(1, (uint32_t)far);
    visible.clear();
    horizon.clear();
    seen[far] = stamp;
    while (!stack.empty()) {
      const uint32_t t = stack.back();
      stack.pop_back();
      visible.push_back(t);
      for (int j = 0; j < 3; ++j) {
        const uint32_t x = tris[t].v[j], y = tris[t].v[(j + 1) % 3];
        const auto it = owner.find(ekey(y, x));
        if (it == owner.end()) { r.failed = true; return; }
        const uint32_t nb = it->second;
        if (seen[nb] == stamp) continue;
        if (seen[nb] == -stamp) { horizon.emplace_back(x, y); continue; }
        if (hull_dist(tris[nb].pl, pt(p)) >= -tol) { seen[nb] = stamp; stack.push_back(nb); }
        else { seen[nb] = -stamp; horizon.emplace_back(x, y); }
      }
    }
    if (horizon.size() < 3) { r.failed = true; return; }
    for (const uint32_t t : visible) {
      for (int j = 0; j < 3; ++j) owner.erase(ekey(tris[t].v[j], tris[t].v[(j + 1) % 3]));
      tris[t].alive = false;
      free_slots.push_back(t);
    }
    for (const auto& e : horizon) add(e.first, e.second, p);
    seen.resize(tris.size(), 0);
  }
  std::vector<uint32_t> flat;
  for (const Tri& t : tris) if (t.alive) { flat.push_back(t.v[0]); flat.push_back(t.v[1]); flat.push_back(t.v[2]); }
  std::vector<Poly> polys;
  if (!merge3(P, flat, tol, polys)) { r.failed = true; return; }
  finish3(P, polys, simplicial, r);
}

inline void build2(const double* P, std::vector<uint32_t> act, double tol, HullResult& r) {
  auto pt = [&](uint32_t i) { return P + 3 * (size_t)i; };
  std::sort(act.begin(), act.end(), [&](uint32_t i, uint32_t j) {
    if (pt(i)[0] != pt(j)[0]) return pt(i)[0] < pt(j)[0];
    if (pt(i)[1] != pt(j)[1]) return pt(i)[1] < pt(j)[1];
    return i < j;
  });
  const uint32_t first = act.front(), last = act.back();
  if (pt(first)[0] == pt(last)[0] && pt(first)[1] == pt(last)[1]) {      // one point (duplicates are gone already)
    r.rank = 0;
    r.bootstrap = {hull_plane_through(pt(first), 1, 0, 0), hull_plane_through(pt(first), -1, 0, 0), hull_plane_through(pt(first), 0, 1, 0), hull_plane_through(pt(first), 0, -1, 0)};
    return;
  }
  // Andrew's chain with the band: the middle one of three consecutive points stays iff it lies more than tol outside the line of the others
  std::vector<uint32_t> h;
  auto push = [&](uint32_t p, size_t floor_size) {
    while (h.size() >= floor_size + 2 && hull_dist(hull_plane2(pt(h[h.size() - 2]), pt(p)), pt(h.back())) <= tol) h.pop_back();
    h.push_back(p);
  };
  for (size_t i = 0; i < act.size(); ++i) push(act[i], 0);
  const size_t lower = h.size() - 1;
  for (size_t i = act.size() - 1; i-- > 0;) push(act[i], lower);
  h.pop_back();      // (the first point again)
  if (h.size() < 3) {
    r.rank = 1;
    r.bootstrap = {hull_plane2(pt(first), pt(last)), hull_plane2(pt(last), pt(first))};
    return;
  }
  r.rank = 2;
  std::vector<uint32_t> vs(h);
  std::sort(vs.begin(), vs.end());
  r.vertex_ids = vs;
  const size_t V = vs.size();
  std::vector<std::pair<uint32_t, uint32_t>> edges;
  for (size_t i = 0; i < h.size(); ++i) {
    const uint32_t x = (uint32_t)(std::lower_bound(vs.begin(), vs.end(), h[i]) - vs.begin()), y = (uint32_t)(std::lower_bound(vs.begin(), vs.end(), h[(i + 1) % h.size()]) - vs.begin());
    edges.emplace_back(x, y);
  }
  std::sort(edges.begin(), edges.end());
  float acc[2] = {0.0f, 0.0f};
  for (size_t k = 0; k < V; ++k)
    for (int c = 0; c < 2; ++c) acc[c] = acc[c] + (float)pt(vs[k])[c];
  r.interior[0] = acc[0] / (float)V; r.interior[1] = acc[1] / (float)V; r.interior[2] = 0.0f;
  const double c0[2] = {(double)r.interior[0], (double)r.interior[1]};
  std::vector<uint32_t> starts(V), ends(V);      // the edge that starts / ends at a vertex
  for (size_t k = 0; k < edges.size(); ++k) { starts[edges[k].first] = (uint32_t)k; ends[edges[k].second] = (uint32_t)k; }
  r.facet_offsets.assign(1, 0u);
  r.vertex_facet_offsets.assign(1, 0u);
  for (size_t k = 0; k < edges.size(); ++k) {
    const double *p = pt(vs[edges[k].first]), *q = pt(vs[edges[k].second]);
    r.planes.push_back(hull_plane2(p, q));
    const double x = q[0] - p[0], y = q[1] - p[1];
    r.area += std::sqrt(x * x + y * y);
    r.volume += 0.5 * ((p[0] - c0[0]) * (q[1] - c0[1]) - (p[1] - c0[1]) * (q[0] - c0[0]));
    r.facet_indices.push_back(edges[k].first); r.facet_indices.push_back(edges[k].second);
    r.facet_neighbors.push_back(ends[edges[k].first]); r.facet_neighbors.push_back(starts[edges[k].second]);
    r.facet_offsets.push_back((uint32_t)r.facet_indices.size());
  }
  for (size_t v = 0; v < V; ++v) {
    r.vertex_facets.push_back(std::min(starts[v], ends[v])); r.vertex_facets.push_back(std::max(starts[v], ends[v]));
    r.vertex_facet_offsets.push_back((uint32_t)r.vertex_facets.size());
  }
  r.empty = false;
}

}  // namespace hull_detail

// P: m candidates, 3 doubles each (z = 0 in 2-D), in ascending order of their input index; all finite
inline HullResult hull_build(const double* P, size_t m, int dim, double tol, bool simplicial) {
  HullResult r;
  r.dim = dim;
  if (m == 0) { r.rank = -1; return r; }
  // exact duplicates: the lowest position stays
  std::vector<uint32_t> order(m);
  for (size_t i = 0; i < m; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t i, uint32_t j) {
    for (int c = 0; c < 3; ++c) if (P[3 * (size_t)i + c] != P[3 * (size_t)j + c]) return P[3 * (size_t)i + c] < P[3 * (size_t)j + c];
    return i < j;
  });
  std::vector<uint32_t> act;
  for (size_t k = 0; k < m; ++k) {
    const uint32_t i = order[k];
    if (k > 0) {
      const uint32_t j = order[k - 1];
      if (P[3 * (size_t)i] == P[3 * (size_t)j] && P[3 * (size_t)i + 1] == P[3 * (size_t)j + 1] && P[3 * (size_t)i + 2] == P[3 * (size_t)j + 2]) continue;
    }
    act.push_back(i);
  }
  std::sort(act.begin(), act.end());
  if (dim == 2) hull_detail::build2(P, act, tol, r); else hull_detail::build3(P, act, tol, simplicial, r);
  return r;
}

}  // namespace cilhip

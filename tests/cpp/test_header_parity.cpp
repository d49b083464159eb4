// tests/cpp/test_header_parity.cpp -- every class of include/cilantro_hip/ that sits on a shared base (the clustering classes, the kd-trees,
// the normal estimators, the RANSAC estimators) against a direct call of its C entry with the same inputs, on the device.  The headers only
// marshal, so every output must agree bit for bit: labels, the cluster lists, modes, shifted seeds, iteration counts, neighbour indices and
// squared distances, normals, curvature, masks, inlier flags, inliers, models and residuals.  Each direct call is made twice first: a row
// whose two direct calls differ is reported as UNREPEATABLE (no entry here is expected to be).
// The shapes are those where marshalling can go wrong: n = 0, 1 and 200 points off the origin with one exact duplicate; dim 1, 2 and 16;
// k = 1 and k above n; a seed list that is absent, empty and of one element; segment sizes that drop a segment; a radius search with no
// neighbour at all and one with some; RANSAC from given samples, from a seed, with a residual no hypothesis meets, and through the lazy
// getters.  k-means over no point is refused by the entries: there the class's exception is compared with the entry's code and text.
// Driven by tests/test_gpu_header_parity.py; writes one line per family and "parity OK".
#include <cilantro_hip/clustering.hpp>
#include <cilantro_hip/kd_tree.hpp>
#include <cilantro_hip/model_estimation.hpp>
#include <cilantro_hip/normal_estimation.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace cilantro_hip;

typedef std::vector<float> Floats;
typedef std::vector<uint32_t> Words;
typedef std::vector<size_t> Indices;
typedef RadiusNeighborhoodSpecification<float> Radius;

static int g_bad = 0, g_rows = 0, g_unrepeatable = 0;
static const float kInf = std::numeric_limits<float>::infinity();

static void fail(const std::string& row, const char* what) {
  ++g_bad;
  std::printf("FAIL %s: %s differs\n", row.c_str(), what);
}
static void ok(int rc, const std::string& row) {
  if (rc != CILHIP_OK) throw std::runtime_error(row + ": the direct call failed (rc " + std::to_string(rc) + "): " + cilhip_last_error(nullptr));
}
template <class T>
static bool same_bits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(T)));
}
template <class T>
static void expect(const std::string& row, const char* what, const std::vector<T>& got, const std::vector<T>& want) {
  if (!same_bits(got, want)) fail(row, what);
}
static void expect(const std::string& row, const char* what, size_t got, size_t want) {
  if (got != want) fail(row, what);
}
// two direct calls of one entry gave `a` and `b`
template <class T>
static void repeatable(const std::string& row, const std::vector<T>& a, const std::vector<T>& b) {
  if (!same_bits(a, b)) { ++g_unrepeatable; std::printf("UNREPEATABLE %s\n", row.c_str()); }
}

// n points in dim dimensions off the origin: four groups of unequal size one unit apart on every axis, a jitter of at most 0.02 inside a
// group, and the last point an exact copy of the first
static Floats cloud(size_t n, size_t dim, unsigned salt = 0) {
  Floats p(n * dim);
  for (size_t i = 0; i < n; ++i) {
    const size_t r = i % 7, group = r < 3 ? 0 : r < 5 ? 1 : r == 5 ? 2 : 3;
    for (size_t a = 0; a < dim; ++a) p[i * dim + a] = 100.0f + (float)group + 0.02f * (float)(((i * dim + a + salt) * 2654435761u) % 1000u) / 1000.0f;
  }
  for (size_t a = 0; a < dim && n > 1; ++a) p[(n - 1) * dim + a] = p[a];
  return p;
}
static Floats unit_rows(size_t n, size_t dim) {      // unit vectors along axis (i mod dim), sign by i
  Floats v(n * dim, 0.0f);
  for (size_t i = 0; i < n; ++i) v[i * dim + i % dim] = (i % 3) ? 1.0f : -1.0f;
  return v;
}

template <class W, class T>
static std::vector<W> widen(const std::vector<T>& v, size_t n) { return std::vector<W>(v.begin(), v.begin() + n); }
static std::vector<Indices> lists(const Words& offsets, const Words& members, size_t count) {
  std::vector<Indices> m(count);
  for (size_t k = 0; k < count; ++k) m[k].assign(members.begin() + offsets[k], members.begin() + offsets[k + 1]);
  return m;
}
static void expect_lists(const std::string& row, const std::vector<Indices>& got, const std::vector<Indices>& want) {
  if (got != want) fail(row, "the cluster lists");
}

// ---- connected components ---------------------------------------------------------------------------------------------------------------
struct CcOut { Words labels, offsets, members; size_t nseg = 0; };
template <class ExtractorT>
static void cc_compare(const std::string& row, const ExtractorT& c, size_t n, const CcOut& d, const CcOut& again) {
  ++g_rows;
  repeatable(row, d.labels, again.labels);
  repeatable(row, d.members, again.members);
  expect(row, "the number of clusters", c.getNumberOfClusters(), d.nseg);
  expect(row, "the number of points", c.getNumberOfPoints(), n);
  expect(row, "the labels", c.getPointToClusterIndexMap(), widen<size_t>(d.labels, n));
  expect_lists(row, c.getClusterToPointIndicesMap(), lists(d.offsets, d.members, d.nseg));
  Indices in, out;
  for (size_t i = 0; i < n; ++i) (d.labels[i] < d.nseg ? in : out).push_back(i);
  expect(row, "the labelled points", c.getLabeledPointIndices(), in);
  expect(row, "the unlabelled points", c.getUnlabeledPointIndices(), out);
}
static cilhip_cc_params cc_params(float radius_sq, size_t min_size, size_t max_size) {
  cilhip_cc_params p;
  cilhip_cc_default_params(&p);
  p.radius_sq = radius_sq; p.min_segment_size = min_size; p.max_segment_size = max_size;
  return p;
}
static const size_t kNoLimit = std::numeric_limits<size_t>::max();

static void components(size_t n, size_t dim, bool nd) {
  const Floats p = cloud(n, dim), normals = unit_rows(n, dim), colors = cloud(n, 3, 17);
  const Radius nh(0.25f);
  struct SeedCase { const char* name; bool given; Indices seeds; };
  std::vector<SeedCase> seed_cases = {{"no seed list", false, {}}, {"an empty seed list", true, {}}};
  if (n) seed_cases.push_back({"one seed", true, {n - 1}});
  for (const SeedCase& sc : seed_cases)
    for (int variant = 0; variant < (n ? 3 : 2); ++variant) {      // 0: no clause; 1: sizes that drop segments; 2: a normals and a colours clause (the arrays of no point are null, which the entry refuses)
      const std::string row = std::string(nd ? "ConnectedComponentExtractionXf" : "ConnectedComponentExtraction3f") + " n=" + std::to_string(n) + " dim=" + std::to_string(dim) + ", " + sc.name +
                              ", variant " + std::to_string(variant);
      const size_t lo = variant == 1 ? 30 : 1, hi = variant == 1 ? 60 : kNoLimit;
      cilhip_cc_params prm = cc_params(0.25f, lo, hi);
      if (variant == 2) { prm.use_normals = 1; prm.max_angle = 0.5f; prm.angle_inclusive = 0; prm.use_colors = 1; prm.color_thresh = 0.9f; }
      const Words seed32(sc.seeds.begin(), sc.seeds.end());
      const uint32_t none = 0;
      const uint32_t* sp = sc.given ? (seed32.empty() ? &none : seed32.data()) : nullptr;
      CcOut d[2];
      for (CcOut& o : d) {
        o.labels.assign(n + 1, 0xDEADBEEFu); o.offsets.assign(n + 1, 0u); o.members.assign(n + 1, 0xDEADBEEFu);
        const float* nrm = variant == 2 ? normals.data() : nullptr;
        const float* col = variant == 2 ? colors.data() : nullptr;
        if (nd) ok(cilhip_connected_components_nd(0, p.data(), nrm, col, n, dim, CILHIP_MEM_HOST, &prm, 0, sp, seed32.size(), o.labels.data(), o.offsets.data(), o.members.data(), &o.nseg), row);
        else ok(cilhip_connected_components3f(0, p.data(), nrm, col, n, CILHIP_MEM_HOST, &prm, sp, seed32.size(), o.labels.data(), o.offsets.data(), o.members.data(), &o.nseg), row);
      }
      if (nd) {
        cilhip_ccn_stats want = cilhip_ccn_stats();
        if (n) cilhip_ccn_last_stats(&want);
        ConnectedComponentExtractionXf<> c{ConstDataView(p, dim)};
        const ConstDataView nv(normals, dim);
        const ConstPointsView cv(colors);
        if (variant == 2) { if (sc.given) c.segment(nh, sc.seeds, NormalsColorsProximityEvaluator(nv, cv, 0.5f, 0.9f)); else c.segment(nh, NormalsColorsProximityEvaluator(nv, cv, 0.5f, 0.9f)); }
        else if (sc.given) c.segment(nh, sc.seeds, AlwaysTrueEvaluator(), lo, hi);
        else c.segment(nh, AlwaysTrueEvaluator(), lo, hi);
        cc_compare(row, c, n, d[0], d[1]);
        const cilhip_ccn_stats& got = c.getLastStats();
        if (n == 200 && variant == 1 && !sc.given && (c.getLabeledPointIndices().empty() || c.getUnlabeledPointIndices().empty())) fail(row, "(the case) labelled and unlabelled points do not both occur;");
        if (got.form_used != want.form_used || got.axis != want.axis || got.tiles_total != want.tiles_total || got.tiles_tested != want.tiles_tested || c.getDimension() != dim) fail(row, "getLastStats");
      } else {
        ConnectedComponentExtraction3f<> c{ConstPointsView(p)};
        const ConstPointsView nv(normals), cv(colors);
        if (variant == 2) { if (sc.given) c.segment(nh, sc.seeds, NormalsColorsProximityEvaluator(nv, cv, 0.5f, 0.9f)); else c.segment(nh, NormalsColorsProximityEvaluator(nv, cv, 0.5f, 0.9f)); }
        else if (sc.given) c.segment(nh, sc.seeds, AlwaysTrueEvaluator(), lo, hi);
        else c.segment(nh, AlwaysTrueEvaluator(), lo, hi);
        cc_compare(row, c, n, d[0], d[1]);
        if (n == 200 && variant == 1 && !sc.given && (c.getLabeledPointIndices().empty() || c.getUnlabeledPointIndices().empty())) fail(row, "(the case) labelled and unlabelled points do not both occur;");
      }
    }
}

// ---- mean shift -------------------------------------------------------------------------------------------------------------------------
struct MsOut { Floats shifted, modes; Words labels, offsets, members; size_t nc = 0, iters = 0; };
template <class ClustererT>
static void ms_compare(const std::string& row, const ClustererT& m, size_t ns, size_t dim, const MsOut& d, const MsOut& again) {
  ++g_rows;
  repeatable(row, d.shifted, again.shifted);
  repeatable(row, d.modes, again.modes);
  repeatable(row, d.labels, again.labels);
  expect(row, "the number of clusters", m.getNumberOfClusters(), d.nc);
  expect(row, "the number of seeds", m.getNumberOfPoints(), ns);
  expect(row, "the iteration count", m.getNumberOfPerformedIterations(), d.iters);
  expect(row, "the shifted seeds", m.getShiftedSeeds(), Floats(d.shifted.begin(), d.shifted.begin() + dim * ns));
  expect(row, "the modes", m.getClusterModes(), Floats(d.modes.begin(), d.modes.begin() + dim * d.nc));
  expect(row, "the labels", m.getPointToClusterIndexMap(), widen<size_t>(d.labels, ns));
  expect_lists(row, m.getClusterToPointIndicesMap(), lists(d.offsets, d.members, d.nc));
}
static void mean_shift(size_t n, size_t dim, bool nd) {
  const Floats p = cloud(n, dim);
  struct SeedCase { const char* name; bool given; Floats seeds; };
  std::vector<SeedCase> cases = {{"no seed list", false, {}}, {"an empty seed list", true, {}}, {"one seed", true, cloud(1, dim, 5)}, {"nine seeds", true, cloud(9, dim, 9)}};
  for (const SeedCase& sc : cases)
    for (int kind = 0; kind < 3; kind += 2) {      // Unity and RBF
      const std::string row = std::string(nd ? "MeanShiftXf" : "MeanShift3f") + " n=" + std::to_string(n) + " dim=" + std::to_string(dim) + ", " + sc.name + ", kernel " + std::to_string(kind);
      const size_t ns = sc.given ? sc.seeds.size() / dim : n;
      cilhip_ms_params prm;
      cilhip_ms_default_params(&prm);
      prm.kernel_radius = 0.4f; prm.max_iter = 20; prm.cluster_tol = 0.05f; prm.convergence_tol = 1e-6f; prm.kernel_kind = kind; prm.kernel_sigma = 0.3f;
      const Floats none(dim, 0.0f);
      const float* sp = sc.given ? (ns ? sc.seeds.data() : none.data()) : nullptr;
      MsOut d[2];
      for (MsOut& o : d) {
        o.shifted.assign(dim * ns + 1, -1.0f); o.modes.assign(dim * ns + 1, -1.0f); o.labels.assign(ns + 1, 0u); o.offsets.assign(ns + 1, 0u); o.members.assign(ns + 1, 0u);
        if (nd) ok(cilhip_mean_shift_nd(0, p.data(), n, dim, sp, sc.given ? ns : 0, CILHIP_MEM_HOST, &prm, o.shifted.data(), o.labels.data(), o.modes.data(), o.offsets.data(), o.members.data(), &o.nc, &o.iters), row);
        else ok(cilhip_mean_shift3f(0, p.data(), n, sp, sc.given ? ns : 0, CILHIP_MEM_HOST, &prm, o.shifted.data(), o.labels.data(), o.modes.data(), o.offsets.data(), o.members.data(), &o.nc, &o.iters), row);
      }
      if (nd) {
        MeanShiftXf<> m{ConstDataView(p, dim)};
        const ConstDataView sv(sc.seeds, dim);
        if (kind) { if (sc.given) m.cluster(sv, 0.4f, 20, 0.05f, 1e-6f, RBFKernelWeightEvaluator<float>(0.3f)); else m.cluster(0.4f, 20, 0.05f, 1e-6f, RBFKernelWeightEvaluator<float>(0.3f)); }
        else if (sc.given) m.cluster(sv, 0.4f, 20, 0.05f, 1e-6f);
        else m.cluster(0.4f, 20, 0.05f, 1e-6f);
        ms_compare(row, m, ns, dim, d[0], d[1]);
        expect(row, "getDimension", m.getDimension(), dim);
      } else {
        MeanShift3f<> m{ConstPointsView(p)};
        const ConstPointsView sv(sc.seeds);
        if (kind) { if (sc.given) m.cluster(sv, 0.4f, 20, 0.05f, 1e-6f, RBFKernelWeightEvaluator<float>(0.3f)); else m.cluster(0.4f, 20, 0.05f, 1e-6f, RBFKernelWeightEvaluator<float>(0.3f)); }
        else if (sc.given) m.cluster(sv, 0.4f, 20, 0.05f, 1e-6f);
        else m.cluster(0.4f, 20, 0.05f, 1e-6f);
        ms_compare(row, m, ns, dim, d[0], d[1]);
      }
    }
}

// ---- k-means ----------------------------------------------------------------------------------------------------------------------------
static void kmeans_nd(size_t n, size_t dim, size_t k) {
  const std::string row = "KMeansXf n=" + std::to_string(n) + " dim=" + std::to_string(dim) + " k=" + std::to_string(k);
  const Floats p = cloud(n, dim);
  Indices start;
  for (size_t c = 0; c < k; ++c) start.push_back(c * n / k);
  Floats cent[2];
  Words labels[2];
  size_t iters[2] = {0, 0};
  for (int r = 0; r < 2; ++r) {
    for (size_t i : start) cent[r].insert(cent[r].end(), p.begin() + i * dim, p.begin() + (i + 1) * dim);
    labels[r].assign(n + 1, 0u);
    ok(cilhip_kmeans_nd(0, p.data(), n, dim, CILHIP_MEM_HOST, cent[r].data(), k, 50, 1e-6f, labels[r].data(), &iters[r]), row);
  }
  ++g_rows;
  repeatable(row, cent[0], cent[1]);
  repeatable(row, labels[0], labels[1]);
  KMeansXf<> km(p.data(), n, dim);
  km.cluster(start, 50, 1e-6f);
  expect(row, "the centroids", km.getClusterCentroids(), cent[0]);
  expect(row, "the iteration count", km.getNumberOfPerformedIterations(), iters[0]);
  expect(row, "the labels", km.getPointToClusterIndexMap(), widen<size_t>(labels[0], n));
  std::vector<Indices> want(k);
  for (size_t i = 0; i < n; ++i) want[labels[0][i]].push_back(i);
  expect_lists(row, km.getClusterToPointIndicesMap(), want);
  expect(row, "the number of clusters", km.getNumberOfClusters(), k);
  expect(row, "the number of points", km.getNumberOfPoints(), n);
}
static void kmeans_3f(size_t n, size_t k, bool use_kd_tree) {
  const std::string row = "KMeans3f n=" + std::to_string(n) + " k=" + std::to_string(k) + (use_kd_tree ? ", kd-tree rounding" : "");
  const Floats p = cloud(n, 3);
  Floats start;
  for (size_t c = 0; c < k; ++c) start.insert(start.end(), p.begin() + 3 * (c * n / k), p.begin() + 3 * (c * n / k) + 3);
  Floats cent[2] = {start, start};
  Words labels[2];
  size_t iters[2] = {0, 0};
  for (int r = 0; r < 2; ++r) {
    labels[r].assign(n + 1, 0u);
    ok(cilhip_kmeans3f_ex(0, p.data(), n, CILHIP_MEM_HOST, cent[r].data(), k, 50, 1e-6f, use_kd_tree ? 1 : 0, labels[r].data(), &iters[r]), row);
  }
  ++g_rows;
  repeatable(row, cent[0], cent[1]);
  repeatable(row, labels[0], labels[1]);
  KMeans3f km{ConstPointsView(p)};
  km.cluster(ConstPointsView(start), 50, 1e-6f, use_kd_tree);
  expect(row, "the centroids", km.getClusterCentroids(), cent[0]);
  expect(row, "the iteration count", km.getNumberOfPerformedIterations(), iters[0]);
  expect(row, "the labels", km.getPointToClusterIndexMap(), widen<size_t>(labels[0], n));
  std::vector<Indices> want(k);
  for (size_t i = 0; i < n; ++i) want[labels[0][i]].push_back(i);
  expect_lists(row, km.getClusterToPointIndicesMap(), want);
  expect(row, "the number of clusters", km.getNumberOfClusters(), k);
}

// no point at all: the entries refuse it (CILHIP_ERR_INVALID), and the classes say so with that code
static void kmeans_refused(size_t dim) {
  const std::string row = "k-means n=0 dim=" + std::to_string(dim);
  const Floats none, start(dim, 100.0f);
  Floats cent = start;
  uint32_t label = 0;
  size_t iters = 0;
  const float at = 0.0f;      // (an address: the refusal meant is the one of n = 0, not of a null array)
  const int rc = dim == 3 ? cilhip_kmeans3f_ex(0, &at, 0, CILHIP_MEM_HOST, cent.data(), 1, 50, 1e-6f, 0, &label, &iters) : cilhip_kmeans_nd(0, &at, 0, dim, CILHIP_MEM_HOST, cent.data(), 1, 50, 1e-6f, &label, &iters);
  ++g_rows;
  if (rc != CILHIP_ERR_INVALID) fail(row, "(the direct call's return code is not CILHIP_ERR_INVALID) the refusal");
  const std::string want = " failed (rc " + std::to_string(rc) + ")";      // (the code; the surface program pins the whole text)
  try {
    if (dim == 3) { KMeans3f km{ConstPointsView(&at, 0)}; km.cluster(ConstPointsView(start)); }
    else { KMeansXf<> km(&at, 0, dim); km.cluster(start); }
    fail(row, "(no exception) the refusal");
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).compare(0, 13, "cilhip_kmeans") != 0 || std::string(e.what()).find(want) == std::string::npos) fail(row, "the refusal's code");
  }
}

// ---- kd-trees ---------------------------------------------------------------------------------------------------------------------------
static void expect_rows(const std::string& row, const NeighborhoodSet& got, const Words& idx, const Floats& d2, const Words& cnt, size_t nq, size_t k) {
  if (got.size() != nq) { fail(row, "the number of lists"); return; }
  for (size_t i = 0; i < nq; ++i) {
    if (got[i].size() != cnt[i]) { fail(row, "a list's length"); return; }
    for (size_t j = 0; j < cnt[i]; ++j)
      if (got[i][j].index != idx[i * k + j] || std::memcmp(&got[i][j].value, &d2[i * k + j], sizeof(float))) { fail(row, "a neighbour"); return; }
  }
}
static void expect_csr(const std::string& row, const NeighborhoodSet& got, const std::vector<uint64_t>& off, const Words& idx, const Floats& d2, size_t nq) {
  if (got.size() != nq) { fail(row, "the number of lists"); return; }
  for (size_t i = 0; i < nq; ++i) {
    if (got[i].size() != off[i + 1] - off[i]) { fail(row, "a list's length"); return; }
    for (size_t j = 0; j < got[i].size(); ++j)
      if (got[i][j].index != idx[off[i] + j] || std::memcmp(&got[i][j].value, &d2[off[i] + j], sizeof(float))) { fail(row, "a neighbour"); return; }
  }
}
static void kd_tree(size_t n, size_t nq, size_t dim, bool nd) {
  const Floats p = cloud(n, dim), q = cloud(nq + 1, dim, 3);      // (one more than asked: a null query pointer means "the points are the queries")
  const ConstDataView qx(q.data(), dim, nq);
  const ConstPointsView q3(q.data(), nq);
  const std::string name = std::string(nd ? "KDTreeXf" : "KDTree3f") + " n=" + std::to_string(n) + " queries=" + std::to_string(nq) + " dim=" + std::to_string(dim);
  const KDTreeXf tx{ConstDataView(p, dim)};
  const KDTree3f t3{ConstPointsView(p.data(), nd ? 0 : n)};
  struct KnnCase { size_t k; float radius; };
  for (const KnnCase& kc : {KnnCase{1, kInf}, KnnCase{8, kInf}, KnnCase{n + 3 <= 32 ? n + 3 : 32, kInf}, KnnCase{5, 0.0004f}}) {
    const std::string row = name + ", k=" + std::to_string(kc.k) + (kc.radius < kInf ? " in a radius" : "");
    Words idx[2], cnt[2];
    Floats d2[2];
    for (int r = 0; r < 2; ++r) {
      idx[r].assign(nq * kc.k + 1, 0u); d2[r].assign(nq * kc.k + 1, 0.0f); cnt[r].assign(nq + 1, 0u);
      if (nd) ok(cilhip_knn_nd(0, p.data(), n, q.data(), nq, dim, CILHIP_MEM_HOST, kc.k, kc.radius, idx[r].data(), d2[r].data(), cnt[r].data()), row);
      else ok(cilhip_knn3f(0, p.data(), n, q.data(), nq, CILHIP_MEM_HOST, kc.k, kc.radius, idx[r].data(), d2[r].data(), cnt[r].data()), row);
    }
    ++g_rows;
    repeatable(row, idx[0], idx[1]);
    repeatable(row, d2[0], d2[1]);
    repeatable(row, cnt[0], cnt[1]);
    const NeighborhoodSet got = nd ? (kc.radius < kInf ? tx.kNNInRadiusSearch(qx, kc.k, kc.radius) : tx.kNNSearch(qx, kc.k))
                                   : (kc.radius < kInf ? t3.kNNInRadiusSearch(q3, kc.k, kc.radius) : t3.kNNSearch(q3, kc.k));
    expect_rows(row, got, idx[0], d2[0], cnt[0], nq, kc.k);
    if (nd && nq) {      // the one-query overloads and the specification dispatch
      const Neighborhood one = kc.radius < kInf ? tx.kNNInRadiusSearch(q.data(), kc.k, kc.radius) : tx.kNNSearch(q.data(), kc.k);
      expect_rows(row + ", one query", NeighborhoodSet(1, one), idx[0], d2[0], cnt[0], 1, kc.k);
      const NeighborhoodSet by_spec = kc.radius < kInf ? tx.search(qx, KNNInRadiusNeighborhoodSpecification<float>(kc.k, kc.radius)) : tx.search(qx, KNNNeighborhoodSpecification(kc.k));
      expect_rows(row + ", by specification", by_spec, idx[0], d2[0], cnt[0], nq, kc.k);
      if (kc.k == 1) expect_rows(row + ", nearestNeighborSearch", tx.nearestNeighborSearch(qx), idx[0], d2[0], cnt[0], nq, 1);
    }
  }
  for (float radius : {0.0f, 0.0004f * (float)dim, 0.3f}) {      // nothing found; a few; whole groups
    const std::string row = name + ", radius " + std::to_string(radius);
    std::vector<uint64_t> off[2];
    Words idx[2];
    Floats d2[2];
    size_t total[2] = {0, 0};
    for (int r = 0; r < 2; ++r) {
      off[r].assign(nq + 1, 0);
      auto search = [&](uint32_t* i, float* d, size_t cap) {
        return nd ? cilhip_radius_search_nd(0, p.data(), n, q.data(), nq, dim, CILHIP_MEM_HOST, radius, off[r].data(), i, d, cap, &total[r])
                  : cilhip_radius_search3f(0, p.data(), n, q.data(), nq, CILHIP_MEM_HOST, radius, off[r].data(), i, d, cap, &total[r]);
      };
      ok(search(nullptr, nullptr, 0), row);
      idx[r].assign(total[r] + 1, 0u); d2[r].assign(total[r] + 1, 0.0f);
      if (total[r]) ok(search(idx[r].data(), d2[r].data(), total[r]), row);
    }
    ++g_rows;
    repeatable(row, off[0], off[1]);
    repeatable(row, idx[0], idx[1]);
    repeatable(row, d2[0], d2[1]);
    if (n == 200 && nq > 1 && ((radius == 0.0f) != (total[0] == 0))) fail(row, "(the case) the total is not zero / non-zero as meant;");
    expect_csr(row, nd ? tx.radiusSearch(qx, radius) : t3.radiusSearch(q3, radius), off[0], idx[0], d2[0], nq);
    if (nd) expect_csr(row + ", by specification", tx.search(qx, Radius(radius)), off[0], idx[0], d2[0], nq);
  }
}

// ---- normal estimators ------------------------------------------------------------------------------------------------------------------
static void normals(size_t n) {
  const Floats p = cloud(n, 3);
  const ConstPointsView v(p);
  const float nan = std::numeric_limits<float>::quiet_NaN();
  for (int with_view_point = 0; with_view_point < 2; ++with_view_point) {
    const float vp[3] = {with_view_point ? 0.0f : nan, with_view_point ? 0.0f : nan, with_view_point ? 500.0f : nan};
    NormalEstimation3f e(v);
    if (with_view_point) e.setViewPoint(vp);
    struct Case { const char* name; size_t k; float radius; };      // k = 0: radius only
    for (const Case& c : {Case{"k-NN", 8, kInf}, Case{"k-NN in a radius", 12, 0.03f}, Case{"radius", 0, 0.03f}}) {
      const std::string row = std::string("NormalEstimation3f n=") + std::to_string(n) + ", " + c.name + (with_view_point ? ", view point" : "");
      Floats nrm[2], cur[2];
      for (int r = 0; r < 2; ++r) {
        nrm[r].assign(3 * n, 0.0f); cur[r].assign(n, 0.0f);
        const float r2 = c.radius < kInf ? c.radius * c.radius : kInf;
        if (c.k) ok(cilhip_normals_knn3f(0, p.data(), n, CILHIP_MEM_HOST, c.k, r2, vp, nrm[r].data(), cur[r].data()), row);
        else ok(cilhip_normals_radius3f(0, p.data(), n, CILHIP_MEM_HOST, r2, vp, nrm[r].data(), cur[r].data()), row);
      }
      ++g_rows;
      repeatable(row, nrm[0], nrm[1]);
      repeatable(row, cur[0], cur[1]);
      Floats gn(5, 1.0f), gc(7, 1.0f);
      if (!c.k) {
        e.getNormalsAndCurvatureRadius(gn, gc, c.radius);
        expect(row, "the normals (alone)", e.getNormalsRadius(c.radius), nrm[0]);
        expect(row, "the curvature (alone)", e.getCurvatureRadius(c.radius), cur[0]);
      } else if (c.radius < kInf) {
        e.getNormalsAndCurvatureKNNInRadius(gn, gc, c.k, c.radius);
        expect(row, "the normals (alone)", e.getNormalsKNNInRadius(c.k, c.radius), nrm[0]);
        expect(row, "the curvature (alone)", e.getCurvatureKNNInRadius(c.k, c.radius), cur[0]);
      } else {
        e.getNormalsAndCurvatureKNN(gn, gc, c.k);
        expect(row, "the normals (alone)", e.getNormalsKNN(c.k), nrm[0]);
        expect(row, "the curvature (alone)", e.getCurvatureKNN(c.k), cur[0]);
      }
      expect(row, "the normals", gn, nrm[0]);
      expect(row, "the curvature", gc, cur[0]);
    }
    // the robust estimator: a chi-square threshold, so that masks and inlier flags carry something
    RobustNormalEstimation3f re(v);
    re.covarianceMethod().setNumberOfTrials(4).setNumberOfRefinements(2).setInlierRatio(0.6f).setChiSquareThreshold(7.8f).setSeed(11);
    if (with_view_point) re.setViewPoint(vp[0], vp[1], vp[2]);
    for (float radius : {kInf, 0.03f}) {
      const std::string row = std::string("RobustNormalEstimation3f n=") + std::to_string(n) + (radius < kInf ? ", k-NN in a radius" : ", k-NN") + (with_view_point ? ", view point" : "");
      cilhip_mcd_params mp;
      cilhip_mcd_params_default(&mp);
      mp.k = 12; mp.max_sq_dist = radius < kInf ? radius * radius : kInf; mp.num_trials = 4; mp.num_refinements = 2; mp.inlier_ratio = 0.6f; mp.chi_square_threshold = 7.8f; mp.seed = 11;
      Floats nrm[2], cur[2];
      Words masks[2];
      std::vector<uint8_t> inl[2];
      for (int r = 0; r < 2; ++r) {
        nrm[r].assign(3 * n, 0.0f); cur[r].assign(n, 0.0f); masks[r].assign(n, 0u); inl[r].assign(n, 0);
        float none[3];
        ok(cilhip_robust_normals_knn3f(0, p.data(), n, CILHIP_MEM_HOST, &mp, vp, n ? nrm[r].data() : none, cur[r].data(), masks[r].data(), inl[r].data()), row);
      }
      ++g_rows;
      repeatable(row, nrm[0], nrm[1]);
      repeatable(row, cur[0], cur[1]);
      repeatable(row, masks[0], masks[1]);
      repeatable(row, inl[0], inl[1]);
      Floats gn(5, 1.0f), gc(7, 1.0f);
      Words gm(3, 1u);
      std::vector<uint8_t> gi(3, 1);
      if (radius < kInf) {
        re.getNormalsAndCurvatureKNNInRadius(gn, gc, 12, radius);
        re.getSubsetMasksAndInliersKNNInRadius(gm, gi, 12, radius);
        expect(row, "the normals (alone)", re.getNormalsKNNInRadius(12, radius), nrm[0]);
        expect(row, "the curvature (alone)", re.getCurvatureKNNInRadius(12, radius), cur[0]);
      } else {
        re.getNormalsAndCurvatureKNN(gn, gc, 12);
        re.getSubsetMasksAndInliersKNN(gm, gi, 12);
        expect(row, "the normals (alone)", re.getNormalsKNN(12), nrm[0]);
        expect(row, "the curvature (alone)", re.getCurvatureKNN(12), cur[0]);
      }
      expect(row, "the normals", gn, nrm[0]);
      expect(row, "the curvature", gc, cur[0]);
      expect(row, "the subset masks", gm, masks[0]);
      expect(row, "the inlier flags", gi, inl[0]);
    }
  }
}

// ---- RANSAC estimators ------------------------------------------------------------------------------------------------------------------
struct RansacCase { const char* name; bool samples; uint64_t seed; float residual; size_t target, max_iter; bool re_estimate, lazy; };
static const RansacCase kRansac[] = {
    {"from a seed", false, 7, 0.05f, 150, 40, true, false},
    {"from given samples", true, 0, 0.05f, 150, 12, true, false},
    {"from a seed, no re-estimation", false, 9, 0.05f, 60, 40, false, false},
    {"a residual no hypothesis meets", true, 0, -1.0f, 150, 12, false, false},      // (a negative bound: nothing is an inlier)
    {"a residual no hypothesis meets, re-estimation asked", false, 5, -1.0f, 150, 8, true, false},
    {"through the lazy getters", false, 3, 0.05f, 150, 40, true, true},
};
static Words sample_triples(size_t n, size_t max_iter) {
  Words s;
  for (size_t i = 0; i < max_iter; ++i)
    for (size_t j = 0; j < 3; ++j) s.push_back(n ? (uint32_t)((i * 37 + j * 61 + 1) % n) : 0u);
  return s;
}
// a plane z = 100 + small noise, every fifth point far off it
static Floats planar(size_t n) {
  Floats p = cloud(n, 3);
  for (size_t i = 0; i < n; ++i) p[3 * i + 2] = 100.0f + ((i % 5) ? 0.001f * (float)(i % 11) : 3.0f + (float)(i % 13));
  return p;
}
static void plane_ransac(size_t n) {
  const Floats p = planar(n);
  for (const RansacCase& c : kRansac) {
    const std::string row = "PlaneRANSACEstimator3f n=" + std::to_string(n) + ", " + c.name;
    const Words samples = c.samples ? sample_triples(n, c.max_iter) : Words();
    cilhip_plane_model d[2];
    Floats res[2];
    Words inl[2];
    for (int r = 0; r < 2; ++r) {
      res[r].assign(n, 0.0f); inl[r].assign(n + 1, 0u);
      ok(cilhip_plane_ransac3f(0, p.data(), n, CILHIP_MEM_HOST, c.samples ? samples.data() : nullptr, c.seed, c.residual, c.target, c.max_iter, c.re_estimate ? 1 : 0, &d[r], res[r].data(), inl[r].data()), row);
      inl[r].resize(d[r].n_inliers);
    }
    ++g_rows;
    repeatable(row, res[0], res[1]);
    repeatable(row, inl[0], inl[1]);
    repeatable(row, Floats(d[0].normal, d[0].normal + 3), Floats(d[1].normal, d[1].normal + 3));
    PlaneRANSACEstimator3f e{ConstPointsView(p)};
    e.setMaxInlierResidual(c.residual).setTargetInlierCount(c.target).setMaxNumberOfIterations(c.max_iter).setReEstimationStep(c.re_estimate).setSeed(c.seed);
    if (c.samples) e.setSamples(samples);
    if (!c.lazy) e.estimate();
    Hyperplane3f m;
    e.getModel(m);
    const Floats want = {d[0].normal[0], d[0].normal[1], d[0].normal[2], d[0].offset};
    expect(row, "the model", Floats(e.getModel().coeffs(), e.getModel().coeffs() + 4), want);
    expect(row, "the model (copied out)", Floats(m.coeffs(), m.coeffs() + 4), want);
    expect(row, "the residuals", e.getModelResiduals(), res[0]);
    expect(row, "the inliers", e.getModelInliers(), widen<size_t>(inl[0], inl[0].size()));
    expect(row, "the number of inliers", e.getNumberOfInliers(), d[0].n_inliers);
    expect(row, "the iteration count", e.getNumberOfPerformedIterations(), d[0].iterations);
    expect(row, "the target flag", (size_t)e.targetInlierCountAchieved(), (size_t)(d[0].target_reached != 0));
  }
  const std::string row = "PlaneRANSACEstimator3f::estimateModel n=" + std::to_string(n);
  float fit[2][4];
  for (auto& f : fit) ok(cilhip_plane_fit3f(0, p.data(), n, CILHIP_MEM_HOST, f), row);
  ++g_rows;
  repeatable(row, Floats(fit[0], fit[0] + 4), Floats(fit[1], fit[1] + 4));
  PlaneRANSACEstimator3f e{ConstPointsView(p)};
  const Hyperplane3f m = e.estimateModel();
  expect(row, "the model", Floats(m.coeffs(), m.coeffs() + 4), Floats(fit[0], fit[0] + 4));
}
static void rigid_ransac(size_t n) {
  const Floats dst = cloud(n, 3);
  Floats src(3 * n);      // dst turned about z by 0.3 rad and moved; every sixth pair is wrong
  for (size_t i = 0; i < n; ++i) {
    const float x = dst[3 * i] - 100.0f, y = dst[3 * i + 1] - 100.0f, z = dst[3 * i + 2] - 100.0f;
    src[3 * i] = std::cos(0.3f) * x - std::sin(0.3f) * y + 5.0f + ((i % 6) ? 0.0f : 2.0f);
    src[3 * i + 1] = std::sin(0.3f) * x + std::cos(0.3f) * y - 2.0f;
    src[3 * i + 2] = z + 1.0f;
  }
  bool cleared = false;
  for (const RansacCase& c : kRansac) {
    const std::string row = "RigidTransformRANSACEstimator3f n=" + std::to_string(n) + ", " + c.name;
    const Words samples = c.samples ? sample_triples(n, c.max_iter) : Words();
    cilhip_transform_model d[2];
    Floats res[2];
    Words inl[2];
    for (int r = 0; r < 2; ++r) {
      res[r].assign(n, 0.0f); inl[r].assign(n + 1, 0u);
      ok(cilhip_transform_ransac3f(0, dst.data(), src.data(), n, CILHIP_MEM_HOST, c.samples ? samples.data() : nullptr, c.seed, c.residual, c.target, c.max_iter, c.re_estimate ? 1 : 0, &d[r], res[r].data(), inl[r].data()), row);
      inl[r].resize(d[r].n_inliers);
      if (!d[r].have_model) res[r].clear();      // the rule of the class: no model, no residuals
    }
    ++g_rows;
    repeatable(row, res[0], res[1]);
    repeatable(row, inl[0], inl[1]);
    repeatable(row, Floats(d[0].T, d[0].T + 16), Floats(d[1].T, d[1].T + 16));
    cleared = cleared || !d[0].have_model;
    // (the three constructors gather the same pairs)
    Indices all(n);
    for (size_t i = 0; i < n; ++i) all[i] = i;
    CorrespondenceSet<float> corr(n);
    for (size_t i = 0; i < n; ++i) corr[i] = Correspondence<float>{i, i, 0.0f};
    const ConstPointsView dv(dst), sv(src);
    RigidTransformRANSACEstimator3f by_pairs(dv, sv), by_corr(dv, sv, corr), by_lists(dv, sv, all, all);
    for (RigidTransformRANSACEstimator3f* e : {&by_pairs, &by_corr, &by_lists}) {
      e->setSeed(c.seed).setReEstimationStep(c.re_estimate);
      if (c.samples) e->setSamples(samples);
      if (c.lazy) e->setMaxInlierResidual(c.residual).setTargetInlierCount(c.target).setMaxNumberOfIterations(c.max_iter);
      else e->estimate(c.residual, c.target, c.max_iter);
      expect(row, "the model", Floats(e->getModel().m, e->getModel().m + 16), Floats(d[0].T, d[0].T + 16));
      expect(row, "the residuals", e->getModelResiduals(), res[0]);
      expect(row, "the inliers", e->getModelInliers(), widen<size_t>(inl[0], inl[0].size()));
      expect(row, "the number of inliers", e->getNumberOfInliers(), d[0].n_inliers);
      expect(row, "the iteration count", e->getNumberOfPerformedIterations(), d[0].iterations);
      expect(row, "the target flag", (size_t)e->targetInlierCountAchieved(), (size_t)(d[0].target_reached != 0));
    }
  }
  if (n >= 3 && !cleared) fail("RigidTransformRANSACEstimator3f", "(the case) no run was left without a model, so the cleared residuals were never compared;");
  const std::string row = "RigidTransformRANSACEstimator3f::estimateModel n=" + std::to_string(n);
  float fit[2][16];
  for (auto& f : fit) ok(cilhip_transform_fit3f(0, dst.data(), src.data(), n, CILHIP_MEM_HOST, f), row);
  ++g_rows;
  repeatable(row, Floats(fit[0], fit[0] + 16), Floats(fit[1], fit[1] + 16));
  RigidTransformRANSACEstimator3f e{ConstPointsView(dst), ConstPointsView(src)};
  const RigidTransform3f m = e.estimateModel();
  expect(row, "the model", Floats(m.m, m.m + 16), Floats(fit[0], fit[0] + 16));
}

static void family(const char* name, int rows_before) { std::printf("%-28s %3d rows\n", name, g_rows - rows_before); std::fflush(stdout); }

int main() {
  try {
    int r = g_rows;
    for (size_t n : {0, 1, 200}) { components(n, 3, false); for (size_t dim : {1, 2, 16}) components(n, dim, true); }
    family("connected components", r); r = g_rows;
    for (size_t n : {0, 1, 200}) { mean_shift(n, 3, false); for (size_t dim : {1, 2, 16}) mean_shift(n, dim, true); }
    family("mean shift", r); r = g_rows;
    for (size_t dim : {1, 2, 16}) { kmeans_nd(200, dim, 3); kmeans_nd(1, dim, 1); }
    kmeans_3f(200, 4, false); kmeans_3f(200, 4, true); kmeans_3f(1, 1, false);
    for (size_t dim : {1, 2, 3, 16}) kmeans_refused(dim);
    family("k-means", r); r = g_rows;
    for (size_t n : {0, 1, 200}) for (size_t nq : {0, 1, 50}) { kd_tree(n, nq, 3, false); for (size_t dim : {1, 2, 16}) kd_tree(n, nq, dim, true); }
    family("kd-trees", r); r = g_rows;
    for (size_t n : {0, 1, 200}) normals(n);
    family("normal estimators", r); r = g_rows;
    for (size_t n : {0, 1, 200}) { plane_ransac(n); rigid_ransac(n); }
    family("RANSAC estimators", r);
  } catch (const std::exception& e) {
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
  if (g_unrepeatable) std::printf("%d rows are not repeatable\n", g_unrepeatable);
  if (g_bad || g_unrepeatable) { std::printf("FAIL: %d differences in %d rows\n", g_bad, g_rows); return 1; }
  std::printf("parity OK: %d rows\n", g_rows);
  return 0;
}

// tests/cpp/test_header_surface.cpp -- the public surface of the classes of include/cilantro_hip/ that share bases (the clustering classes,
// the kd-trees, the normal estimators, the RANSAC estimators), pinned at compile time, and what they throw, checked at run time without a
// device.  Driven by tests/test_header_surface_cpu.py:
//   test_header_surface host               the refusals that never reach the library, by type and text
//   test_header_surface nodevice [parent]  every wrapper that reports a failing entry, on a machine without a device: the exception type, the
//                                          "cilhip_x failed (rc N" prefix and N against the table below, and that the text after the colon
//                                          is the failing call's own.  `parent`: the headers from before abi.hpp, where the rows marked
//                                          `drift` carried no text (and KMeans3f named cilhip_kmeans3f): those assert type and prefix only.
// A member function is pinned through a cast of its address to the exact pointer-to-member type of the class named -- return type, parameters
// and constness; the cast also accepts a member the class inherits -- and a member template or a chained call through the type of a call.
#include <cilantro_hip/clustering.hpp>
#include <cilantro_hip/fusion.hpp>
#include <cilantro_hip/grid_downsampler.hpp>
#include <cilantro_hip/image_point_cloud_conversions.hpp>
#include <cilantro_hip/kd_tree.hpp>
#include <cilantro_hip/model_estimation.hpp>
#include <cilantro_hip/multidimensional_scaling.hpp>
#include <cilantro_hip/normal_estimation.hpp>
#include <cilantro_hip/principal_component_analysis.hpp>
#include <cilantro_hip/spatial.hpp>

#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

using namespace cilantro_hip;

#define MEMBER(C, name, ...) static_assert(std::is_same<decltype(static_cast<__VA_ARGS__>(&C::name)), __VA_ARGS__>::value, #C "::" #name)
#define RESULT(T, ...) static_assert(std::is_same<decltype(__VA_ARGS__), T>::value, #__VA_ARGS__)
#define SAME(A, ...) static_assert(std::is_same<A, __VA_ARGS__>::value, #A)

typedef std::vector<float> Floats;
typedef std::vector<size_t> Indices;
typedef std::vector<std::vector<size_t>> IndexLists;
typedef RadiusNeighborhoodSpecification<float> Radius;
template <class T> T& lv();      // an lvalue of T in an unevaluated call

// ---- the shared types are visible through every header that showed them -----------------------------------------------------------
SAME(Neighborhood, std::vector<Neighbor>);
SAME(NeighborhoodSet, std::vector<std::vector<Neighbor>>);
SAME(RadiusNeighborhoodSpecification<>, RadiusNeighborhoodSpecification<float>);
SAME(decltype(Neighbor::index), size_t);
SAME(decltype(Neighbor::value), float);
SAME(decltype(Radius::radius), float);
static_assert(ConstPointsView::rows() == 3 && std::is_convertible<Floats, ConstPointsView>::value && std::is_constructible<ConstPointsView, const float*, size_t>::value, "ConstPointsView");
static_assert(std::is_constructible<ConstDataView, const float*, size_t, size_t>::value && std::is_constructible<ConstDataView, const Floats&, size_t>::value, "ConstDataView");
static_assert(!std::is_convertible<float, Radius>::value && std::is_constructible<Radius, float>::value, "the radius specification's constructor is explicit");

// ---- connected components ---------------------------------------------------------------------------------------------------------------
template <class C, class ViewT>
struct ClusteringSurface {      // what all six clustering class templates show, for the index types of C
  typedef typename C::ClusterToPointIndicesMap Lists;
  typedef typename C::PointToClusterIndexMap Labels;
  MEMBER(C, getClusterToPointIndicesMap, const Lists& (C::*)() const);
  MEMBER(C, getPointToClusterIndexMap, const Labels& (C::*)() const);
  MEMBER(C, getNumberOfClusters, size_t (C::*)() const);
  MEMBER(C, getNumberOfPoints, size_t (C::*)() const);
};
template <class C, class ViewT, class PointIndexT>
struct ComponentsSurface : ClusteringSurface<C, ViewT> {
  typedef std::vector<PointIndexT> Seeds;
  RESULT(C&, lv<C>().segment(lv<const Radius>()));
  RESULT(C&, lv<C>().segment(lv<const Radius>(), AlwaysTrueEvaluator()));
  RESULT(C&, lv<C>().segment(lv<const Radius>(), PointsProximityEvaluator(1.0f), size_t(1), size_t(2)));
  RESULT(C&, lv<C>().segment(lv<const Radius>(), lv<const Seeds>()));
  RESULT(C&, lv<C>().segment(lv<const Radius>(), lv<const Seeds>(), PointsProximityEvaluator(1.0f), size_t(1), size_t(2)));
  RESULT(C&, lv<C>().segment(lv<const Radius>()).segment(lv<const Radius>(), lv<const Seeds>()));
  MEMBER(C, getLabeledPointIndices, Seeds (C::*)() const);
  MEMBER(C, getUnlabeledPointIndices, Seeds (C::*)() const);
};
typedef ConnectedComponentExtraction3f<> CCE3;
typedef ConnectedComponentExtractionXf<> CCEX;
typedef ConnectedComponentExtraction2f<> CCE2;
SAME(CCE3, ConnectedComponentExtraction3f<size_t, size_t>);
SAME(CCEX, ConnectedComponentExtractionXf<size_t, size_t>);
SAME(CCE2, ConnectedComponentExtraction2f<size_t, size_t>);
SAME(CCE3::ClusterToPointIndicesMap, IndexLists);
SAME(CCE3::PointToClusterIndexMap, Indices);
SAME(CCEX::ClusterToPointIndicesMap, IndexLists);
SAME(CCEX::PointToClusterIndexMap, Indices);
SAME(ConnectedComponentExtraction3f<uint32_t, int>::ClusterToPointIndicesMap, std::vector<std::vector<uint32_t>>);
SAME(ConnectedComponentExtraction3f<uint32_t, int>::PointToClusterIndexMap, std::vector<int>);
SAME(ConnectedComponentExtractionXf<uint32_t, int>::ClusterToPointIndicesMap, std::vector<std::vector<uint32_t>>);
SAME(ConnectedComponentExtractionXf<uint32_t, int>::PointToClusterIndexMap, std::vector<int>);
template struct ComponentsSurface<CCE3, ConstPointsView, size_t>;
template struct ComponentsSurface<ConnectedComponentExtraction3f<uint32_t, int>, ConstPointsView, uint32_t>;
template struct ComponentsSurface<CCEX, ConstDataView, size_t>;
template struct ComponentsSurface<ConnectedComponentExtractionXf<uint32_t, int>, ConstDataView, uint32_t>;
MEMBER(CCEX, getDimension, size_t (CCEX::*)() const);
MEMBER(CCEX, getLastStats, const cilhip_ccn_stats& (CCEX::*)() const);
static_assert(std::is_constructible<CCE3, const ConstPointsView&>::value && std::is_constructible<CCE3, const ConstPointsView&, int>::value && !std::is_convertible<ConstPointsView, CCE3>::value, "CCE3f(points, device = 0), explicit");
static_assert(std::is_constructible<CCEX, const ConstDataView&>::value && std::is_constructible<CCEX, const ConstDataView&, int, int>::value && !std::is_convertible<ConstDataView, CCEX>::value, "CCEXf(points, device = 0, form = 0), explicit");
static_assert(std::is_base_of<CCEX, CCE2>::value && std::is_constructible<CCE2, const ConstDataView&, int, int>::value && std::is_constructible<CCE2, const float*, size_t>::value &&
                  std::is_constructible<CCE2, const float*, size_t, int>::value && !std::is_convertible<ConstDataView, CCE2>::value, "CCE2f");
RESULT(CCEX&, lv<CCE2>().segment(lv<const Radius>()));      // (the 2f class inherits the Xf class's segment)

// ---- mean shift -------------------------------------------------------------------------------------------------------------------------
template <class C, class ViewT>
struct MeanShiftSurface : ClusteringSurface<C, ViewT> {
  RESULT(C&, lv<C>().cluster(1.0f, size_t(1), 1.0f));
  RESULT(C&, lv<C>().cluster(1.0f, size_t(1), 1.0f, 1e-7f, RBFKernelWeightEvaluator<float>(2.0f)));
  RESULT(C&, lv<C>().cluster(lv<const ViewT>(), 1.0f, size_t(1), 1.0f));
  RESULT(C&, lv<C>().cluster(lv<const ViewT>(), 1.0f, size_t(1), 1.0f, 1e-7f, IdentityWeightEvaluator<float>()));
  RESULT(C&, lv<C>().cluster(1.0f, size_t(1), 1.0f).cluster(lv<const ViewT>(), 1.0f, size_t(1), 1.0f));
  MEMBER(C, getShiftedSeeds, const Floats& (C::*)() const);
  MEMBER(C, getClusterModes, const Floats& (C::*)() const);
  MEMBER(C, getNumberOfPerformedIterations, size_t (C::*)() const);
};
typedef MeanShift3f<> MS3;
typedef MeanShiftXf<> MSX;
typedef MeanShift2f<> MS2;
SAME(MS3, MeanShift3f<size_t, size_t>);
SAME(MSX, MeanShiftXf<size_t, size_t>);
SAME(MS2, MeanShift2f<size_t, size_t>);
SAME(MS3::ClusterToPointIndicesMap, IndexLists);
SAME(MS3::PointToClusterIndexMap, Indices);
SAME(MeanShiftXf<uint32_t, int>::ClusterToPointIndicesMap, std::vector<std::vector<uint32_t>>);
SAME(MeanShiftXf<uint32_t, int>::PointToClusterIndexMap, std::vector<int>);
template struct MeanShiftSurface<MS3, ConstPointsView>;
template struct MeanShiftSurface<MeanShift3f<uint32_t, int>, ConstPointsView>;
template struct MeanShiftSurface<MSX, ConstDataView>;
template struct MeanShiftSurface<MeanShiftXf<uint32_t, int>, ConstDataView>;
MEMBER(MSX, getDimension, size_t (MSX::*)() const);
static_assert(std::is_constructible<MS3, const ConstPointsView&>::value && std::is_constructible<MS3, const ConstPointsView&, size_t, int>::value && !std::is_convertible<ConstPointsView, MS3>::value, "MeanShift3f(points, max_leaf_size = 10, device = 0), explicit");
static_assert(std::is_constructible<MSX, const ConstDataView&>::value && std::is_constructible<MSX, const ConstDataView&, size_t, int>::value && !std::is_convertible<ConstDataView, MSX>::value, "MeanShiftXf(points, max_leaf_size = 10, device = 0), explicit");
static_assert(std::is_base_of<MSX, MS2>::value && std::is_constructible<MS2, const ConstDataView&, size_t, int>::value && std::is_constructible<MS2, const float*, size_t>::value &&
                  std::is_constructible<MS2, const float*, size_t, int>::value && !std::is_convertible<ConstDataView, MS2>::value, "MeanShift2f");
RESULT(MSX&, lv<MS2>().cluster(1.0f, size_t(1), 1.0f));

// ---- k-means ----------------------------------------------------------------------------------------------------------------------------
typedef KMeansXf<> KMX;
SAME(KMX, KMeansXf<size_t, size_t>);
SAME(KMX::ClusterToPointIndicesMap, IndexLists);
SAME(KMX::PointToClusterIndexMap, Indices);
SAME(KMeansXf<uint32_t, int>::ClusterToPointIndicesMap, std::vector<std::vector<uint32_t>>);
SAME(KMeansXf<uint32_t, int>::PointToClusterIndexMap, std::vector<int>);
template struct ClusteringSurface<KMX, ConstDataView>;
template struct ClusteringSurface<KMeansXf<uint32_t, int>, ConstDataView>;
MEMBER(KMX, cluster, KMX& (KMX::*)(const Floats&, size_t, float, bool));
MEMBER(KMX, cluster, KMX& (KMX::*)(const Indices&, size_t, float, bool));
RESULT(KMX&, lv<KMX>().cluster(lv<const Floats>()));
RESULT(KMX&, lv<KMX>().cluster(lv<const Indices>()));
MEMBER(KMX, getClusterCentroids, const Floats& (KMX::*)() const);
MEMBER(KMX, getNumberOfPerformedIterations, size_t (KMX::*)() const);
static_assert(std::is_default_constructible<KMX>::value && std::is_constructible<KMX, const float*, size_t, size_t>::value && std::is_constructible<KMX, const float*, size_t, size_t, int>::value, "KMeansXf");
static_assert(std::is_base_of<KMX, SpectralClusteringXf<>>::value && std::is_base_of<KMeansXf<uint32_t, int>, SpectralClustering<3, uint32_t, int>>::value, "SpectralClustering is a KMeansXf");
template struct ClusteringSurface<SpectralClusteringXf<>, ConstDataView>;
MEMBER(KMeans3f, cluster, KMeans3f& (KMeans3f::*)(const ConstPointsView&, size_t, float, bool));
MEMBER(KMeans3f, cluster, KMeans3f& (KMeans3f::*)(size_t, size_t, float, bool));
RESULT(KMeans3f&, lv<KMeans3f>().cluster(lv<const ConstPointsView>()));
RESULT(KMeans3f&, lv<KMeans3f>().cluster(size_t(2)));
MEMBER(KMeans3f, getClusterCentroids, const Floats& (KMeans3f::*)() const);
MEMBER(KMeans3f, getPointToClusterIndexMap, const Indices& (KMeans3f::*)() const);
MEMBER(KMeans3f, getNumberOfClusters, size_t (KMeans3f::*)() const);
MEMBER(KMeans3f, getNumberOfPerformedIterations, size_t (KMeans3f::*)() const);
MEMBER(KMeans3f, getClusterToPointIndicesMap, IndexLists (KMeans3f::*)() const);      // by value
static_assert(std::is_constructible<KMeans3f, const ConstPointsView&, int>::value && !std::is_convertible<ConstPointsView, KMeans3f>::value, "KMeans3f(data, device = 0), explicit");

// ---- kd-trees ---------------------------------------------------------------------------------------------------------------------------
MEMBER(KDTree3f, kNNSearch, NeighborhoodSet (KDTree3f::*)(const ConstPointsView&, size_t) const);
MEMBER(KDTree3f, kNNInRadiusSearch, NeighborhoodSet (KDTree3f::*)(const ConstPointsView&, size_t, float) const);
MEMBER(KDTree3f, radiusSearch, NeighborhoodSet (KDTree3f::*)(const ConstPointsView&, float) const);
MEMBER(KDTree3f, getPointsMatrixMap, const ConstPointsView& (KDTree3f::*)() const);
static_assert(std::is_constructible<KDTree3f, const ConstPointsView&, int>::value && !std::is_convertible<ConstPointsView, KDTree3f>::value, "KDTree3f(points, device = 0), explicit");
MEMBER(KDTreeXf, kNNSearch, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&, size_t) const);
MEMBER(KDTreeXf, kNNSearch, Neighborhood (KDTreeXf::*)(const float*, size_t) const);
MEMBER(KDTreeXf, kNNInRadiusSearch, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&, size_t, float) const);
MEMBER(KDTreeXf, kNNInRadiusSearch, Neighborhood (KDTreeXf::*)(const float*, size_t, float) const);
MEMBER(KDTreeXf, nearestNeighborSearch, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&) const);
MEMBER(KDTreeXf, radiusSearch, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&, float) const);
MEMBER(KDTreeXf, search, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&, const KNNNeighborhoodSpecification&) const);
MEMBER(KDTreeXf, search, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&, const KNNInRadiusNeighborhoodSpecification<float>&) const);
MEMBER(KDTreeXf, search, NeighborhoodSet (KDTreeXf::*)(const ConstDataView&, const Radius&) const);
MEMBER(KDTreeXf, getPointsMatrixMap, const ConstDataView& (KDTreeXf::*)() const);
static_assert(std::is_constructible<KDTreeXf, const ConstDataView&, int>::value && !std::is_convertible<ConstDataView, KDTreeXf>::value, "KDTreeXf(points, device = 0), explicit");
static_assert(std::is_base_of<KDTreeXf, KDTree2f>::value && std::is_constructible<KDTree2f, const ConstDataView&, int>::value && std::is_constructible<KDTree2f, const float*, size_t>::value &&
                  std::is_constructible<KDTree2f, const float*, size_t, int>::value && !std::is_convertible<ConstDataView, KDTree2f>::value, "KDTree2f");

// ---- normal estimators ------------------------------------------------------------------------------------------------------------------
template <class N>
struct NormalsSurface {
  MEMBER(N, getViewPoint, const float* (N::*)() const);
  MEMBER(N, setViewPoint, N& (N::*)(const float*));
  MEMBER(N, setViewPoint, N& (N::*)(float, float, float));
  MEMBER(N, getNormalsAndCurvatureKNN, const N& (N::*)(Floats&, Floats&, size_t) const);
  MEMBER(N, getNormalsKNN, Floats (N::*)(size_t) const);
  MEMBER(N, getCurvatureKNN, Floats (N::*)(size_t) const);
  MEMBER(N, getNormalsAndCurvatureKNNInRadius, const N& (N::*)(Floats&, Floats&, size_t, float) const);
  MEMBER(N, getNormalsKNNInRadius, Floats (N::*)(size_t, float) const);
  MEMBER(N, getCurvatureKNNInRadius, Floats (N::*)(size_t, float) const);
  MEMBER(N, getNormalsAndCurvatureRadius, const N& (N::*)(Floats&, Floats&, float) const);
  MEMBER(N, getNormalsRadius, Floats (N::*)(float) const);
  MEMBER(N, getCurvatureRadius, Floats (N::*)(float) const);
  RESULT(N&, lv<N>().setViewPoint(0.0f, 0.0f, 0.0f).setViewPoint(lv<const float[3]>()));
  static_assert(std::is_constructible<N, const ConstPointsView&>::value && std::is_constructible<N, const ConstPointsView&, int>::value && !std::is_convertible<ConstPointsView, N>::value,
                "(points, device = 0), explicit");
};
template struct NormalsSurface<NormalEstimation3f>;
template struct NormalsSurface<RobustNormalEstimation3f>;
MEMBER(RobustNormalEstimation3f, covarianceMethod, const MinimumCovarianceDeterminant3f& (RobustNormalEstimation3f::*)() const);
MEMBER(RobustNormalEstimation3f, covarianceMethod, MinimumCovarianceDeterminant3f& (RobustNormalEstimation3f::*)());
MEMBER(RobustNormalEstimation3f, getSubsetMasksAndInliersKNN, void (RobustNormalEstimation3f::*)(std::vector<uint32_t>&, std::vector<uint8_t>&, size_t) const);
MEMBER(RobustNormalEstimation3f, getSubsetMasksAndInliersKNNInRadius, void (RobustNormalEstimation3f::*)(std::vector<uint32_t>&, std::vector<uint8_t>&, size_t, float) const);

// ---- RANSAC estimators ------------------------------------------------------------------------------------------------------------------
template <class E>
struct RansacSurface {
  typedef typename E::Model Model;
  SAME(typename E::ResidualScalar, float);
  SAME(typename E::ResidualVector, Floats);
  SAME(typename E::IndexVector, Indices);
  MEMBER(E, getSampleSize, size_t (E::*)() const);
  MEMBER(E, getTargetInlierCount, size_t (E::*)() const);
  MEMBER(E, setTargetInlierCount, E& (E::*)(size_t));
  MEMBER(E, getMaxNumberOfIterations, size_t (E::*)() const);
  MEMBER(E, setMaxNumberOfIterations, E& (E::*)(size_t));
  MEMBER(E, getMaxInlierResidual, float (E::*)() const);
  MEMBER(E, setMaxInlierResidual, E& (E::*)(float));
  MEMBER(E, getReEstimationStep, bool (E::*)() const);
  MEMBER(E, setReEstimationStep, E& (E::*)(bool));
  MEMBER(E, setSeed, E& (E::*)(uint64_t));
  MEMBER(E, setSamples, E& (E::*)(const std::vector<uint32_t>&));
  MEMBER(E, estimate, E& (E::*)());
  MEMBER(E, estimate, E& (E::*)(float, size_t, size_t));
  MEMBER(E, getModel, const Model& (E::*)());
  MEMBER(E, getModelResiduals, const Floats& (E::*)());
  MEMBER(E, getModelInliers, const Indices& (E::*)());
  MEMBER(E, targetInlierCountAchieved, bool (E::*)());
  MEMBER(E, getNumberOfPerformedIterations, size_t (E::*)());
  MEMBER(E, getNumberOfInliers, size_t (E::*)());
  MEMBER(E, estimateModel, Model (E::*)());
  MEMBER(E, getDataPointsCount, size_t (E::*)() const);
  RESULT(E&, lv<E>().setTargetInlierCount(1).setMaxNumberOfIterations(1).setMaxInlierResidual(1.0f).setReEstimationStep(true).setSeed(1).setSamples(std::vector<uint32_t>()).estimate().estimate(1.0f, 1, 1));
};
template struct RansacSurface<PlaneRANSACEstimator3f>;
template struct RansacSurface<RigidTransformRANSACEstimator3f>;
SAME(PlaneRANSACEstimator3f::Model, Hyperplane3f);
MEMBER(PlaneRANSACEstimator3f, getModel, PlaneRANSACEstimator3f& (PlaneRANSACEstimator3f::*)(Hyperplane3f&));
MEMBER(PlaneRANSACEstimator3f, getDeviceMilliseconds, double (PlaneRANSACEstimator3f::*)() const);
static_assert(std::is_constructible<PlaneRANSACEstimator3f, const ConstPointsView&, int>::value && !std::is_convertible<ConstPointsView, PlaneRANSACEstimator3f>::value, "PlaneRANSACEstimator3f(points, device = 0), explicit");
SAME(RigidTransformRANSACEstimator3f::Model, RigidTransform3f);
SAME(RigidTransformRANSACEstimator3f::Transform, RigidTransform3f);
static_assert(RigidTransformRANSACEstimator3f::Dim == 3 && RigidTransformRANSACEstimator3f::MinSampleSize == 3, "the enumerators");
static_assert(std::is_constructible<RigidTransformRANSACEstimator3f, const ConstPointsView&, const ConstPointsView&>::value &&
                  std::is_constructible<RigidTransformRANSACEstimator3f, const ConstPointsView&, const ConstPointsView&, int>::value &&
                  std::is_constructible<RigidTransformRANSACEstimator3f, const ConstPointsView&, const ConstPointsView&, const CorrespondenceSet<float>&, int>::value &&
                  std::is_constructible<RigidTransformRANSACEstimator3f, const ConstPointsView&, const ConstPointsView&, const std::vector<uint32_t>&, const std::vector<uint32_t>&, int>::value,
              "the three constructors");

// ---- run time ---------------------------------------------------------------------------------------------------------------------------
static int g_bad = 0;
static void fail(const std::string& what, const std::string& detail) {
  ++g_bad;
  std::printf("FAIL %s: %s\n", what.c_str(), detail.c_str());
}

// `call` throws std::invalid_argument whose text holds `needle`
static void refuses(const char* what, const char* needle, const std::function<void()>& call) {
  try {
    call();
    fail(what, "no exception");
  } catch (const std::invalid_argument& e) {
    if (!std::strstr(e.what(), needle)) fail(what, std::string("the text is \"") + e.what() + "\"");
  } catch (const std::exception& e) {
    fail(what, std::string("another exception type: ") + e.what());
  }
}

// ~40 points off the origin with one exact duplicate, and the same as dim-major views
static Floats cloud(size_t n, size_t dim) {
  Floats p(n * dim);
  for (size_t i = 0; i < p.size(); ++i) p[i] = 100.0f + 0.01f * (float)((i * 7919u) % 257u);
  for (size_t a = 0; a < dim && n > 1; ++a) p[(n - 1) * dim + a] = p[a];
  return p;
}

static int run_host() {
  const Floats p3 = cloud(40, 3), p2 = cloud(40, 2), p4 = cloud(40, 4), few = cloud(10, 3);
  const ConstPointsView v3(p3), v_few(few);
  const ConstDataView d2(p2, 2), d4(p4, 4), d3(p3, 3);
  const Radius nh(1.0f);
  // a seed index out of range
  refuses("CCE3f seed", "a seed index is not below the number of points", [&] { CCE3 c(v3); c.segment(nh, Indices{0, 40}); });
  refuses("CCEXf seed", "a seed index is not below the number of points", [&] { CCEX c(d4); c.segment(nh, Indices{40}); });
  // evaluator arrays of another size
  refuses("CCE3f evaluator size", "the evaluator's arrays and the points differ in size", [&] { CCE3 c(v3); c.segment(nh, NormalsProximityEvaluator(v_few, 0.1f)); });
  refuses("CCEXf evaluator size", "the evaluator's arrays and the points differ in size", [&] { CCEX c(d4); c.segment(nh, ColorsProximityEvaluator(v_few, 0.1f)); });
  // normals of another dimension than the points
  refuses("CCE3f normals", "the evaluator's normals are not 3 x n", [&] { const Floats n4 = cloud(40, 4); CCE3 c(v3); c.segment(nh, NormalsProximityEvaluator(ConstDataView(n4, 4), 0.1f)); });
  refuses("CCEXf normals", "the evaluator's normals are not dim x n", [&] { CCEX c(d4); c.segment(nh, NormalsProximityEvaluator(v3, 0.1f)); });
  // seeds of another dimension
  refuses("MeanShiftXf seeds", "the seeds have another dimension than the points", [&] { MSX m(d4); m.cluster(d2, 1.0f, 5, 0.1f); });
  // setSamples too short
  refuses("plane setSamples", "setSamples: 3 indices per iteration", [&] { PlaneRANSACEstimator3f e(v3); e.setMaxNumberOfIterations(4).setSamples(std::vector<uint32_t>(11, 0u)).estimate(); });
  refuses("plane setSamples, lazy", "setSamples: 3 indices per iteration", [&] { PlaneRANSACEstimator3f e(v3); e.setSamples(std::vector<uint32_t>(3, 0u)).getModel(); });
  refuses("rigid setSamples", "setSamples: 3 indices per iteration", [&] { RigidTransformRANSACEstimator3f e(v3, v3); e.setSamples(std::vector<uint32_t>(6, 0u)).estimate(0.1f, 5, 3); });
  refuses("rigid pairs", "dst / src pairs must have the same length", [&] { RigidTransformRANSACEstimator3f e(v3, v_few); });
  // a query of another dimension than the tree
  refuses("KDTreeXf knn", "the queries' dimension is not the tree's", [&] { KDTreeXf t(d4); t.kNNSearch(d2, 3); });
  refuses("KDTreeXf radius", "the queries' dimension is not the tree's", [&] { KDTreeXf t(d4); t.radiusSearch(d3, 1.0f); });
  refuses("KDTreeXf search", "the queries' dimension is not the tree's", [&] { KDTreeXf t(d4); t.search(d2, Radius(1.0f)); });
  // the 2f constructors
  refuses("CCE2f", "ConnectedComponentExtraction2f: the points are a 2 x n matrix", [&] { CCE2 c(d4); });
  refuses("MeanShift2f", "MeanShift2f: the points are a 2 x n matrix", [&] { MS2 m(d3); });
  refuses("KDTree2f", "KDTree2f: the points are not 2-D", [&] { KDTree2f t(d4); });
  // the three radius-only getters of the robust estimator
  const char* radius_only = "a radius-only neighbourhood keeps no neighbour list on the device, and the MCD trials rank a list; use the ...KNNInRadius getters (k <= 32)";
  refuses("robust getNormalsRadius", radius_only, [&] { RobustNormalEstimation3f r(v3); r.getNormalsRadius(0.5f); });
  refuses("robust getCurvatureRadius", radius_only, [&] { RobustNormalEstimation3f r(v3); r.getCurvatureRadius(0.5f); });
  refuses("robust getNormalsAndCurvatureRadius", radius_only, [&] { RobustNormalEstimation3f r(v3); Floats a(7, 1.0f), b(5, 1.0f); try { r.getNormalsAndCurvatureRadius(a, b, 0.5f); } catch (...) { if (a.size() != 7 || b.size() != 5) fail("robust radius", "the outputs were touched"); throw; } });
  // the settings the estimators start from, and that a setter makes the lazy getters run again (they refuse here, so no device is needed)
  {
    PlaneRANSACEstimator3f e(v3);
    RigidTransformRANSACEstimator3f r(v3, v3);
    if (e.getMaxInlierResidual() != 0.1f || r.getMaxInlierResidual() != 0.01f || e.getTargetInlierCount() != 20 || r.getTargetInlierCount() != 20 || e.getMaxNumberOfIterations() != 100 ||
        r.getMaxNumberOfIterations() != 100 || !e.getReEstimationStep() || !r.getReEstimationStep() || e.getSampleSize() != 3 || r.getSampleSize() != 3 || e.getDataPointsCount() != 40 ||
        r.getDataPointsCount() != 40 || e.getDeviceMilliseconds() != 0.0)
      fail("RANSAC defaults", "a default moved");
    NormalEstimation3f plain(v3);
    RobustNormalEstimation3f robust(v3);
    const float* vp = plain.getViewPoint();
    const float* vr = robust.setViewPoint(1.0f, 2.0f, 3.0f).getViewPoint();
    if (vp[0] == vp[0] || vp[1] == vp[1] || vp[2] == vp[2] || vr[0] != 1.0f || vr[1] != 2.0f || vr[2] != 3.0f) fail("view point", "NaN by default, then what was set");
  }
  // before any call: empty maps; an empty cloud needs no device
  {
    Floats none;
    CCE3 c{ConstPointsView(none)};
    CCEX x{ConstDataView(none, 5)};
    MS3 m{ConstPointsView(none)};
    MSX mx{ConstDataView(none, 5)};
    KMX k;
    if (c.getNumberOfClusters() || c.getNumberOfPoints() || !c.getLabeledPointIndices().empty() || x.getDimension() != 5 || mx.getDimension() != 5 || m.getNumberOfPerformedIterations() || k.getNumberOfClusters() ||
        x.getLastStats().launches != 0)
      fail("fresh objects", "not empty");
    c.segment(nh).segment(nh, Indices());
    x.segment(nh).segment(nh, Indices());
    m.cluster(1.0f, 3, 0.1f).cluster(ConstPointsView(none), 1.0f, 3, 0.1f);
    mx.cluster(1.0f, 3, 0.1f).cluster(ConstDataView(none, 5), 1.0f, 3, 0.1f);
    if (c.getNumberOfClusters() || x.getNumberOfPoints() || !x.getUnlabeledPointIndices().empty() || m.getNumberOfClusters() || !mx.getShiftedSeeds().empty() || !mx.getClusterModes().empty())
      fail("empty clouds", "not empty");
  }
  if (g_bad) { std::printf("FAIL: %d host checks\n", g_bad); return 1; }
  std::printf("host OK\n");
  return 0;
}

// ---- without a device: every wrapper that turns a return code into an exception -----------------------------------------------------------
struct Row {
  const char* wrapper;
  const char* entry;            // "<entry> failed (rc <rc>): <the library's text>"
  int rc;
  bool drift;                   // before abi.hpp: "<parent_entry> failed (rc <rc>)" and no text
  const char* parent_entry;
  std::function<void()> call;
};

static std::string last_error() { return cilhip_last_error(nullptr); }

static int run_nodevice(bool parent) {
  const Floats p3 = cloud(40, 3), p4 = cloud(40, 4), p2 = cloud(40, 2);
  const ConstPointsView v3(p3);
  const ConstDataView d4(p4, 4);
  const Radius nh(1.0f);
  const float K[9] = {500.0f, 0.0f, 0.0f, 0.0f, 500.0f, 0.0f, 4.0f, 3.0f, 1.0f};      // column-major intrinsics of an 8 x 6 image
  const std::vector<unsigned short> depth(48, 1000);
  const Floats square = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 1.0f, 0.0f, 1.0f};
  const Floats halfspaces = {1.0f, 0.0f, -1.0f, -1.0f, 0.0f, 0.0f, 0.0f, 1.0f, -1.0f, 0.0f, -1.0f, 0.0f};      // the unit square, 3 x 4
  const int nd = CILHIP_ERR_NO_DEVICE;
  const std::vector<Row> rows = {
      {"ConnectedComponentExtraction3f::segment", "cilhip_connected_components3f", nd, false, nullptr, [&] { CCE3 c(v3); c.segment(nh); }},
      {"ConnectedComponentExtraction3f::segment(seeds)", "cilhip_connected_components3f", nd, false, nullptr, [&] { CCE3 c(v3); c.segment(nh, Indices{1}); }},
      {"ConnectedComponentExtractionXf::segment", "cilhip_connected_components_nd", nd, false, nullptr, [&] { CCEX c(d4); c.segment(nh); }},
      {"ConnectedComponentExtractionXf::segment, dim 17", "cilhip_connected_components_nd", CILHIP_ERR_UNSUPPORTED, false, nullptr, [&] { const Floats w = cloud(4, 17); CCEX c(ConstDataView(w, 17)); c.segment(nh); }},
      {"ConnectedComponentExtractionXf::segment, form 3", "cilhip_connected_components_nd", CILHIP_ERR_INVALID, false, nullptr, [&] { CCEX c(d4, 0, 3); c.segment(nh); }},
      {"MeanShift3f::cluster", "cilhip_mean_shift3f", nd, false, nullptr, [&] { MS3 m(v3); m.cluster(1.0f, 5, 0.1f); }},
      {"MeanShiftXf::cluster", "cilhip_mean_shift_nd", nd, false, nullptr, [&] { MSX m(d4); m.cluster(d4, 1.0f, 5, 0.1f); }},
      {"MeanShiftXf::cluster, dim 17", "cilhip_mean_shift_nd", CILHIP_ERR_UNSUPPORTED, false, nullptr, [&] { const Floats w = cloud(4, 17); MSX m(ConstDataView(w, 17)); m.cluster(1.0f, 5, 0.1f); }},
      {"KMeansXf::cluster", "cilhip_kmeans_nd", nd, false, nullptr, [&] { KMX k(p4.data(), 40, 4); k.cluster(Indices{0, 7, 19}); }},
      {"SparseAffinities::fromCSR", "cilhip_sparse_from_csr", nd, false, nullptr, [&] { SparseAffinities::fromCSR(2, {0, 1, 2}, {1, 0}, {1.0f, 1.0f}); }},
      {"getNNGraphFunctionValueSparseMatrix", "cilhip_nn_graph_matrix", nd, false, nullptr, [&] { NeighborhoodSet nn(2); nn[0] = {Neighbor{0, 0.0f}, Neighbor{1, 1.0f}}; nn[1] = {Neighbor{1, 0.0f}, Neighbor{0, 1.0f}}; getNNGraphFunctionValueSparseMatrix(nn); }},
      {"KDTree3f::kNNSearch", "cilhip_knn3f", nd, true, "cilhip_knn3f", [&] { KDTree3f t(v3); t.kNNSearch(v3, 4); }},
      {"KDTree3f::kNNSearch, k 33", "cilhip_knn3f", CILHIP_ERR_INVALID, true, "cilhip_knn3f", [&] { KDTree3f t(v3); t.kNNInRadiusSearch(v3, 33, 1.0f); }},
      {"KDTree3f::radiusSearch", "cilhip_radius_search3f", nd, true, "cilhip_radius_search3f", [&] { KDTree3f t(v3); t.radiusSearch(v3, 1.0f); }},
      {"KDTreeXf::kNNSearch", "cilhip_knn_nd", nd, false, nullptr, [&] { KDTreeXf t(d4); t.kNNSearch(d4, 4); }},
      {"KDTreeXf::kNNSearch, k 33", "cilhip_knn_nd", CILHIP_ERR_UNSUPPORTED, false, nullptr, [&] { KDTreeXf t(d4); t.kNNSearch(p4.data(), 33); }},
      {"KDTreeXf::radiusSearch", "cilhip_radius_search_nd", nd, false, nullptr, [&] { KDTreeXf t(d4); t.search(d4, Radius(1.0f)); }},
      {"NormalEstimation3f, k-NN", "cilhip_normals_knn3f", nd, true, "cilhip_normals_knn3f", [&] { NormalEstimation3f e(v3); e.getNormalsKNN(5); }},
      {"NormalEstimation3f, radius", "cilhip_normals_radius3f", nd, true, "cilhip_normals_radius3f", [&] { NormalEstimation3f e(v3); e.getCurvatureRadius(0.5f); }},
      {"RobustNormalEstimation3f, k-NN", "cilhip_robust_normals_knn3f", nd, false, nullptr, [&] { RobustNormalEstimation3f e(v3); e.getNormalsKNNInRadius(8, 0.5f); }},
      {"RobustNormalEstimation3f, k 33", "cilhip_robust_normals_knn3f", CILHIP_ERR_INVALID, false, nullptr, [&] { RobustNormalEstimation3f e(v3); e.getNormalsKNN(33); }},
      {"PlaneRANSACEstimator3f::estimate", "cilhip_plane_ransac3f", nd, true, "cilhip_plane_ransac3f", [&] { PlaneRANSACEstimator3f e(v3); e.setSeed(3).getModelInliers(); }},
      {"PlaneRANSACEstimator3f::estimateModel", "cilhip_plane_fit3f", nd, true, "cilhip_plane_fit3f", [&] { PlaneRANSACEstimator3f e(v3); e.estimateModel(); }},
      {"RigidTransformRANSACEstimator3f::estimate", "cilhip_transform_ransac3f", nd, true, "cilhip_transform_ransac3f", [&] { RigidTransformRANSACEstimator3f e(v3, v3); e.estimate(0.1f, 30, 10); }},
      {"RigidTransformRANSACEstimator3f::estimateModel", "cilhip_transform_fit3f", nd, true, "cilhip_transform_fit3f", [&] { RigidTransformRANSACEstimator3f e(v3, v3); e.estimateModel(); }},
      {"KMeans3f::cluster", "cilhip_kmeans3f_ex", nd, true, "cilhip_kmeans3f", [&] { KMeans3f k(v3); k.cluster(ConstPointsView(p3.data(), 3)); }},
      {"SurfelMap3f::removeUnstable", "cilhip_fusion_remove_unstable3f", nd, false, nullptr, [&] { SurfelMap3f m; m.model.points = m.model.normals = m.model.colors = Floats(p3.begin(), p3.begin() + 12); m.confidence = Floats(4, 1.0f); m.removeUnstable(0.5f); }},
      {"SurfelMap3f::fuse", "cilhip_fuse_frame3f", nd, false, nullptr, [&] { PointCloud3f f; f.points = f.normals = f.colors = Floats(p3.begin(), p3.begin() + 12); SurfelMap3f m; m.fuse(f, RigidTransform3f(), K, 8, 6); }},
      {"PointsGridDownsampler3f", "cilhip_grid_downsample3f", nd, false, nullptr, [&] { PointsGridDownsampler3f g(v3, 0.5f); }},
      {"PrincipalComponentAnalysis", "cilhip_pca_fit", nd, false, nullptr, [&] { PrincipalComponentAnalysis3f a(p3.data(), 40); }},
      {"MultidimensionalScaling", "cilhip_mds_embedding", nd, false, nullptr, [&] { const Floats D(16, 1.0f); MultidimensionalScaling2f m(D.data(), 4); }},
      {"ConvexPolytope", "cilhip_convex_hull_create", nd, false, nullptr, [&] { ConvexHull2f h(square); }},
      {"ConvexPolytope::getPointSignedDistancesFromFacets", "cilhip_polytope_signed_distances", nd, false, nullptr, [&] { ConvexPolytope2f::fromHalfspaces(halfspaces).getPointSignedDistancesFromFacets(p2.data(), 40); }},
      {"ConvexPolytope::getInteriorPointsIndexMask", "cilhip_polytopes_interior_mask", nd, false, nullptr, [&] { ConvexPolytope2f::fromHalfspaces(halfspaces).getInteriorPointsIndexMask(p2.data(), 40); }},
      {"ConvexPolytope::getInteriorPointIndices", "cilhip_polytopes_interior_indices", nd, false, nullptr, [&] { ConvexPolytope2f::fromHalfspaces(halfspaces).getInteriorPointIndices(p2.data(), 40); }},
      {"SpaceRegion::getInteriorPointsIndexMask", "cilhip_polytopes_interior_mask", nd, false, nullptr, [&] { SpaceRegion2f(ConvexPolytope2f::fromHalfspaces(halfspaces)).getInteriorPointsIndexMask(p2.data(), 40); }},
      {"SpaceRegion::getInteriorPointIndices", "cilhip_polytopes_interior_indices", nd, false, nullptr, [&] { SpaceRegion2f(ConvexPolytope2f::fromHalfspaces(halfspaces)).getInteriorPointIndices(p2.data(), 40); }},
      {"depthImageToPoints", "cilhip_depth_image_to_points3f", nd, false, nullptr, [&] { Floats out; depthImageToPoints(depth.data(), DepthValueConverter<unsigned short>(0.001f), 8, 6, K, out); }},
      {"pointsToDepthImage", "cilhip_points_to_depth_image3f", nd, false, nullptr, [&] { std::vector<unsigned short> img(48); pointsToDepthImage(v3, K, DepthValueConverter<unsigned short>(0.001f), img.data(), 8, 6); }},
      {"pointsToIndexMap", "cilhip_points_to_index_map3f", nd, false, nullptr, [&] { std::vector<size_t> map(48); pointsToIndexMap(v3, K, map.data(), 8, 6); }},
  };
  for (const Row& r : rows) {
    // another entry fails first, and leaves its text behind
    float one = 1.0f, out[4];
    int valid = 0;
    const bool by_pca = std::strcmp(r.entry, "cilhip_pca_fit") != 0;
    const int first = by_pca ? cilhip_pca_fit(0, &one, 1, 0, nullptr, 0, CILHIP_MEM_HOST, out, out, out, out, &valid)
                             : cilhip_mds_embedding(0, nullptr, 0, CILHIP_MEM_HOST, nullptr, nullptr, nullptr, nullptr);
    const std::string earlier = last_error();
    if (first == CILHIP_OK || earlier.empty() || earlier == "null context") fail(r.wrapper, "the earlier call did not fail with a text: \"" + earlier + "\"");
    try {
      r.call();
      fail(r.wrapper, "no exception");
    } catch (const std::invalid_argument& e) {
      fail(r.wrapper, std::string("std::invalid_argument: ") + e.what());
    } catch (const std::runtime_error& e) {
      const std::string text = e.what(), own = last_error();
      const bool short_form = parent && r.drift;
      const std::string prefix = std::string(short_form ? r.parent_entry : r.entry) + " failed (rc " + std::to_string(r.rc) + ")";
      if (text.compare(0, prefix.size(), prefix) != 0) { fail(r.wrapper, "\"" + text + "\" does not start with \"" + prefix + "\""); continue; }
      if (short_form) {
        if (text != prefix) fail(r.wrapper, "\"" + text + "\": more than the short form");
        continue;
      }
      const std::string tail = text.substr(prefix.size());
      if (tail.compare(0, 2, ": ") != 0 || tail.size() <= 2) { fail(r.wrapper, "\"" + text + "\": no text after the return code"); continue; }
      if (tail.substr(2) == earlier) fail(r.wrapper, "\"" + text + "\": the text is the earlier call's");
      if (tail.substr(2) != own) fail(r.wrapper, "\"" + text + "\": the text is not what the call left: \"" + own + "\"");
    } catch (const std::exception& e) {
      fail(r.wrapper, std::string("another exception type: ") + e.what());
    }
  }
  if (g_bad) { std::printf("FAIL: %d of %zu rows\n", g_bad, rows.size()); return 1; }
  std::printf("nodevice OK: %zu rows\n", rows.size());
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "host")) return run_host();
  if (argc >= 2 && !std::strcmp(argv[1], "nodevice")) return run_nodevice(argc >= 3 && !std::strcmp(argv[2], "parent"));
  std::printf("usage: test_header_surface host | nodevice [parent]\n");
  return 2;
}

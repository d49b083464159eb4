// tests/cpp/test_warp_field_affine.cpp -- the C++ mirror of the affine warp-field classes, the dense rigid class and
// resampleAffineTransforms (cilantro_hip/icp.hpp).
//   test_warp_field_affine host   the host half: the four instances' types, setters and getters; needs no device
//   test_warp_field_affine run    small non-rigid registrations end to end (a device is needed): prints "run OK <iterations>"
#include <cilantro_hip/icp.hpp>
#include <cilantro_hip/normal_estimation.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <type_traits>

using namespace cilantro_hip;

#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static void surface(size_t n, float phase, std::vector<float>& xyz, std::vector<float>& nrm) {
  xyz.resize(3 * n); nrm.resize(3 * n);
  const size_t side = (size_t)std::ceil(std::sqrt((double)n));
  for (size_t i = 0; i < n; ++i) {
    const float x = (float)(i % side) / (float)side + 0.37f * phase / (float)side, y = (float)(i / side) / (float)side + 0.21f * phase / (float)side;
    const float z = 0.1f * std::sin(5.0f * x) * std::cos(4.0f * y) + 0.003f * phase * std::sin(3.0f * y);
    const float zx = 0.5f * std::cos(5.0f * x) * std::cos(4.0f * y), zy = -0.4f * std::sin(5.0f * x) * std::sin(4.0f * y);
    const float inv = 1.0f / std::sqrt(zx * zx + zy * zy + 1.0f);
    xyz[3 * i] = x; xyz[3 * i + 1] = y; xyz[3 * i + 2] = z;
    nrm[3 * i] = -zx * inv; nrm[3 * i + 1] = -zy * inv; nrm[3 * i + 2] = inv;
  }
}

// mean |n . (d - q)| of q against its nearest target point
static double plane_residual(const std::vector<float>& dst, const std::vector<float>& dst_n, const std::vector<float>& q) {
  double sum = 0.0;
  for (size_t i = 0; i < q.size() / 3; ++i) {
    size_t best = 0;
    float bd = INFINITY;
    for (size_t j = 0; j < dst.size() / 3; ++j) {
      const float dx = dst[3 * j] - q[3 * i], dy = dst[3 * j + 1] - q[3 * i + 1], dz = dst[3 * j + 2] - q[3 * i + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 < bd) { bd = d2; best = j; }
    }
    sum += std::fabs((double)dst_n[3 * best] * (dst[3 * best] - q[3 * i]) + (double)dst_n[3 * best + 1] * (dst[3 * best + 1] - q[3 * i + 1]) +
                     (double)dst_n[3 * best + 2] * (dst[3 * best + 2] - q[3 * i + 2]));
  }
  return sum / (double)(q.size() / 3);
}

template <class ICP>
static int settings_round_trip(ICP& icp) {
  static_assert(std::is_same<decltype(icp.setHuberLossBoundary(1.0f)), ICP&>::value, "the setters return the instance");
  icp.setMaxNumberOfIterations(4).setConvergenceTolerance(2.5e-3f).setMaxNumberOfGaussNewtonIterations(1).setStiffnessRegularizationWeight(1.0f).setHuberLossBoundary(1e-2f);
  REQUIRE(icp.getMaxNumberOfIterations() == 4 && icp.getConvergenceTolerance() == 2.5e-3f && icp.getMaxNumberOfGaussNewtonIterations() == 1);
  REQUIRE(icp.getStiffnessRegularizationWeight() == 1.0f && icp.getHuberLossBoundary() == 1e-2f && icp.getPointToPlaneMetricWeight() == 1.0f && icp.getPointToPointMetricWeight() == 0.0f);
  REQUIRE(icp.getMaxNumberOfConjugateGradientIterations() == 1000 && icp.getNumberOfPerformedIterations() == 0 && !icp.hasConverged());
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_warp_field_affine host|run\n"); return 2; }
  const bool host = !std::strcmp(argv[1], "host");
  if (host) {
    // the entries and the resample's name exist with the rigid siblings' signatures; no device is touched
    static_assert(std::is_same<decltype(&cilhip_warp_field_estimate_affine3f), decltype(&cilhip_warp_field_estimate3f)>::value, "estimate");
    static_assert(std::is_same<decltype(&cilhip_warp_field_resample_affine3f), decltype(&cilhip_warp_field_resample3f)>::value, "resample");
    static_assert(std::is_same<decltype(&cilhip_warp_field_icp_run_affine), decltype(&cilhip_warp_field_icp_run)>::value, "loop");
    static_assert(std::is_same<AffineTransformSet3f, RigidTransformSet3f>::value, "one holder type");
    static_assert(std::is_constructible<SimpleCombinedMetricSparseAffineWarpFieldICP3f, ConstPointsView, ConstPointsView, ConstPointsView, NeighborhoodSet, size_t, NeighborhoodSet>::value, "sparse affine");
    static_assert(std::is_constructible<SimpleCombinedMetricDenseAffineWarpFieldICP3f, ConstPointsView, ConstPointsView, ConstPointsView, NeighborhoodSet>::value, "dense affine");
    static_assert(std::is_constructible<SimpleCombinedMetricDenseRigidWarpFieldICP3f, ConstPointsView, ConstPointsView, ConstPointsView, NeighborhoodSet>::value, "dense rigid");
    REQUIRE(resampleAffineTransforms(AffineTransformSet3f(), NeighborhoodSet(3)).size() == 3);      // (nothing to blend: identities, no device)
    REQUIRE(resampleAffineTransforms(AffineTransformSet3f(2), NeighborhoodSet()).empty());
    REQUIRE(cilhip_warp_field_resample_affine3f(nullptr, nullptr, nullptr, CILHIP_MEM_HOST) == CILHIP_ERR_INVALID);
    std::printf("host OK\n");
    return 0;
  }
  std::vector<float> dst, dst_n, src, src_n;
  surface(2500, 1.0f, dst, dst_n);
  surface(1600, 0.0f, src, src_n);
  const double before = plane_residual(dst, dst_n, src);
  std::vector<float> ctrl;
  PointsGridDownsampler3f(ConstPointsView(src), 0.15f).getDownsampledPoints(ctrl);
  KDTree3f tree{ConstPointsView(ctrl)};
  const NeighborhoodSet s2c = tree.kNNSearch(ConstPointsView(src), 4), reg = tree.kNNSearch(ConstPointsView(ctrl), 8);
  // sparse affine
  SimpleCombinedMetricSparseAffineWarpFieldICP3f icp(ConstPointsView(dst), ConstPointsView(dst_n), ConstPointsView(src), s2c, ctrl.size() / 3, reg);
  if (settings_round_trip(icp)) return 1;
  icp.correspondenceSearchEngine().setMaxDistance(0.05f * 0.05f);
  icp.controlWeightEvaluator().setSigma(0.075f);
  icp.regularizationWeightEvaluator().setSigma(0.45f);
  const AffineTransformSet3f dense = icp.estimate().getDenseWarpField();
  REQUIRE(dense.size() == 1600 && icp.getTransform().size() == ctrl.size() / 3 && icp.getNumberOfPerformedIterations() >= 1);
  const std::vector<float> warped = transformPoints(dense, ConstPointsView(src));
  for (float v : warped) REQUIRE(std::isfinite(v));
  REQUIRE(plane_residual(dst, dst_n, warped) < before);
  REQUIRE(icp.getResiduals().size() == 1600);
  const AffineTransformSet3f again = resampleAffineTransforms(icp.getTransform(), s2c, WarpWeightEvaluator(WarpWeightEvaluator::RBFKernel, 0.075f));
  REQUIRE(again.size() == dense.size());
  for (size_t i = 0; i < dense.size(); ++i)
    for (int q = 0; q < 16; ++q) REQUIRE(again[i].m[q] == dense[i].m[q]);
  // dense affine and dense rigid: every source point its own node
  KDTree3f src_tree{ConstPointsView(src)};
  const NeighborhoodSet src_reg = src_tree.kNNSearch(ConstPointsView(src), 6);
  SimpleCombinedMetricDenseAffineWarpFieldICP3f da(ConstPointsView(dst), ConstPointsView(dst_n), ConstPointsView(src), src_reg);
  if (settings_round_trip(da)) return 1;
  da.correspondenceSearchEngine().setMaxDistance(0.05f * 0.05f);
  da.regularizationWeightEvaluator().setSigma(0.1f);
  REQUIRE(da.estimate().getDenseWarpField().size() == 1600 && &da.getDenseWarpField() == &da.getTransform());
  REQUIRE(plane_residual(dst, dst_n, transformPoints(da.getDenseWarpField(), ConstPointsView(src))) < before);
  SimpleCombinedMetricDenseRigidWarpFieldICP3f dr(ConstPointsView(dst), ConstPointsView(dst_n), ConstPointsView(src), src_reg);
  if (settings_round_trip(dr)) return 1;
  dr.correspondenceSearchEngine().setMaxDistance(0.05f * 0.05f);
  dr.regularizationWeightEvaluator().setSigma(0.1f);
  dr.setStiffnessRegularizationWeight(200.0f);
  REQUIRE(dr.estimate().getDenseWarpField().size() == 1600);
  REQUIRE(plane_residual(dst, dst_n, transformPoints(dr.getDenseWarpField(), ConstPointsView(src))) < before);
  std::printf("run OK %zu\n", icp.getNumberOfPerformedIterations());
  return 0;
}

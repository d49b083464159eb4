// tests/cpp/test_warp_field.cpp -- the C++ mirror of the warp-field classes (cilantro_hip/icp.hpp, point_cloud.hpp).
//   test_warp_field host   the host half: types, setters and getters with the reference's defaults; needs no device
//   test_warp_field run    a small non-rigid registration end to end (a device is needed): prints "run OK <iterations>"
#include <cilantro_hip/icp.hpp>
#include <cilantro_hip/normal_estimation.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>

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

int main(int argc, char** argv) {
  if (argc < 2) { std::fprintf(stderr, "usage: test_warp_field host|run\n"); return 2; }
  if (!std::strcmp(argv[1], "host")) {
    cilhip_warp_params p;
    cilhip_warp_default_params(&p);
    REQUIRE(p.w_p2p == 0.0f && p.w_p2pl == 1.0f && p.w_reg == 1.0f && p.huber_boundary == 1e-4f && p.max_gn_iter == 10 && p.max_cg_iter == 1000);
    WarpWeightEvaluator ev;
    REQUIRE(ev.kind() == WarpWeightEvaluator::RBFKernel && ev.setSigma(0.5f).sigma() == 0.5f);
    NeighborhoodSet nh(2);
    nh[0] = {Neighbor{1, 0.25f}, Neighbor{0, 0.5f}};
    nh[1] = {Neighbor{0, 0.0f}};
    std::vector<uint32_t> idx; std::vector<float> d2;
    REQUIRE(internal::to_lists(nh, idx, d2) == 2 && idx[0] == 1 && idx[1] == 0 && idx[2] == 0 && idx[3] == 0xFFFFFFFFu && d2[1] == 0.5f);
    RigidTransformSet3f ts(3);
    REQUIRE(ts[2](0, 0) == 1.0f && ts[2](3, 3) == 1.0f && ts[1].translation(2) == 0.0f);
    bool threw = false;
    try { transformPoints(ts, ConstPointsView(d2.data(), 1)); } catch (const std::invalid_argument&) { threw = true; }
    REQUIRE(threw);
    std::printf("host OK\n");
    return 0;
  }
  std::vector<float> dst, dst_n, src, src_n;
  surface(2500, 1.0f, dst, dst_n);
  surface(1600, 0.0f, src, src_n);
  std::vector<float> ctrl;
  PointsGridDownsampler3f(ConstPointsView(src), 0.15f).getDownsampledPoints(ctrl);
  KDTree3f tree{ConstPointsView(ctrl)};
  const NeighborhoodSet s2c = tree.kNNSearch(ConstPointsView(src), 4), reg = tree.kNNSearch(ConstPointsView(ctrl), 8);
  SimpleCombinedMetricSparseRigidWarpFieldICP3f icp(ConstPointsView(dst), ConstPointsView(dst_n), ConstPointsView(src), s2c, ctrl.size() / 3, reg);
  icp.correspondenceSearchEngine().setMaxDistance(0.05f * 0.05f);
  icp.controlWeightEvaluator().setSigma(0.075f);
  icp.regularizationWeightEvaluator().setSigma(0.45f);
  icp.setMaxNumberOfIterations(5).setConvergenceTolerance(2.5e-3f).setMaxNumberOfGaussNewtonIterations(1).setStiffnessRegularizationWeight(200.0f).setHuberLossBoundary(1e-2f);
  const RigidTransformSet3f dense = icp.estimate().getDenseWarpField();
  REQUIRE(dense.size() == 1600 && icp.getTransform().size() == ctrl.size() / 3 && icp.getNumberOfPerformedIterations() >= 1);
  const std::vector<float> res = icp.getResiduals();
  REQUIRE(res.size() == 1600);
  PointCloud3f cloud; cloud.points = src; cloud.normals = src_n;
  const PointCloud3f warped = cloud.transformed(dense);
  REQUIRE(warped.size() == 1600 && warped.hasNormals());
  for (float v : warped.points) REQUIRE(std::isfinite(v));
  const RigidTransformSet3f again = resampleTransforms(icp.getTransform(), s2c, WarpWeightEvaluator(WarpWeightEvaluator::RBFKernel, 0.075f));
  REQUIRE(again.size() == dense.size());
  for (size_t i = 0; i < dense.size(); ++i)
    for (int q = 0; q < 16; ++q) REQUIRE(again[i].m[q] == dense[i].m[q]);
  std::printf("run OK %zu\n", icp.getNumberOfPerformedIterations());
  return 0;
}

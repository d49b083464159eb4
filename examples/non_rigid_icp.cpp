// examples/non_rigid_icp.cpp -- the flow of cilantro's examples/non_rigid_icp.cpp (example 1: a sparsely supported warp field) on the GPU
// engine: control nodes from gridDownsample, the source-to-control lists (k = 4) and the regularisation lists (k = 8) from the k-NN
// mirror, SimpleCombinedMetricSparseRigidWarpFieldICP3f with the example's parameters (:41-82), the source warped by the dense field.
//
//   g++ -O2 -std=c++17 -Iinclude examples/non_rigid_icp.cpp -o non_rigid_icp -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./non_rigid_icp dst.ply src.ply [control_res]
//
// Differs from the reference example only where the missing pieces force it: no visualizer -- the iteration count, convergence, the
// registration time and the minimum / mean / maximum residual are printed.
#include <cilantro_hip/icp.hpp>
#include <cilantro_hip/normal_estimation.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <chrono>
#include <cstdio>
#include <cstdlib>

using namespace cilantro_hip;

int main(int argc, char** argv) {
  if (argc < 3) {
    std::printf("Please provide paths to two PLY files.\n");
    return 0;
  }
  PointCloud3f dst(argv[1]), src(argv[2]);
  if (!dst.hasNormals()) {
    std::printf("Target point cloud is empty or does not have normals!\n");
    return 0;
  }

  // Neighborhood parameters
  const float control_res = argc > 3 ? std::strtof(argv[3], nullptr) : 0.025f;
  const float src_to_control_sigma = 0.5f * control_res;
  const float regularization_sigma = 3.0f * control_res;
  const float max_correspondence_dist_sq = 0.02f * 0.02f;

  // Get a sparse set of control nodes by downsampling
  std::vector<float> control_points;
  PointsGridDownsampler3f(ConstPointsView(src.points), control_res).getDownsampledPoints(control_points);
  const ConstPointsView control_view(control_points);
  KDTree3f control_tree(control_view);
  // Find which control nodes affect each point in src; regularization neighborhoods for control nodes
  const NeighborhoodSet src_to_control_nn = control_tree.kNNSearch(ConstPointsView(src.points), 4);
  const NeighborhoodSet regularization_nn = control_tree.kNNSearch(control_view, 8);
  std::printf("Source points: %zu, target points: %zu, control nodes: %zu\n", src.size(), dst.size(), control_view.cols());

  const auto t0 = std::chrono::steady_clock::now();
  SimpleCombinedMetricSparseRigidWarpFieldICP3f icp(ConstPointsView(dst.points), ConstPointsView(dst.normals), ConstPointsView(src.points), src_to_control_nn,
                                                    control_view.cols(), regularization_nn);
  icp.correspondenceSearchEngine().setMaxDistance(max_correspondence_dist_sq);
  icp.controlWeightEvaluator().setSigma(src_to_control_sigma);
  icp.regularizationWeightEvaluator().setSigma(regularization_sigma);
  icp.setMaxNumberOfIterations(15).setConvergenceTolerance(2.5e-3f);
  icp.setMaxNumberOfGaussNewtonIterations(1).setGaussNewtonConvergenceTolerance(5e-4f);
  icp.setMaxNumberOfConjugateGradientIterations(500).setConjugateGradientConvergenceTolerance(1e-5f);
  icp.setPointToPointMetricWeight(0.0f).setPointToPlaneMetricWeight(1.0f).setStiffnessRegularizationWeight(200.0f);
  icp.setHuberLossBoundary(1e-2f);
  const RigidTransformSet3f tf_est = icp.estimate().getDenseWarpField();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Registration time: %.2fms\n", ms);
  std::printf("Iterations performed: %zu\n", icp.getNumberOfPerformedIterations());
  std::printf("Has converged: %d\n", (int)icp.hasConverged());

  const auto t1 = std::chrono::steady_clock::now();
  const std::vector<float> residuals = icp.getResiduals();
  std::printf("Residual computation time: %.2fms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count());
  double lo = 1e300, hi = 0.0, sum = 0.0;
  size_t finite = 0;
  for (float r : residuals)
    if (std::isfinite(r)) { lo = r < lo ? r : lo; hi = r > hi ? r : hi; sum += r; ++finite; }
  if (finite) std::printf("Residuals (min / mean / max): %.6g / %.6g / %.6g\n", lo, sum / (double)finite, hi);

  // Warp src
  const PointCloud3f warped = src.transformed(tf_est);
  std::printf("Warped points: %zu\n", warped.size());
  return 0;
}

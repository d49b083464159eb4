// examples/robust_normal_estimation.cpp -- the flow of cilantro's examples/robust_normal_estimation.cpp on the GPU engine: a PLY cloud, its
// normals cleared, downsampled to a 5 mm grid, then normals from the minimum-covariance-determinant covariance of every point's 12 nearest
// neighbours -- 2 trials, 1 refinement, chi-square threshold 6.25 (the 90 % confidence ellipsoid), oriented towards the origin.  A point
// the ellipsoid of its own neighbourhood leaves out is an outlier: its normal is NaN, and removeInvalidNormals() drops it.
//
//   g++ -O2 -std=c++17 -Iinclude examples/robust_normal_estimation.cpp -o robust_normal_estimation -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./robust_normal_estimation cloud.ply
//
// Differs from the reference example only where the missing pieces force it: no kd-tree object to time (the search is part of the call)
// and no visualizer -- the counts of valid and invalid normals and the times are printed.
#include <cilantro_hip/normal_estimation.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>

using namespace cilantro_hip;

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("Please provide path to PLY file.\n");
    return 0;
  }
  PointCloud3f cloud(argv[1]);
  if (cloud.isEmpty()) {
    std::printf("Input cloud is empty!\n");
    return 0;
  }
  cloud.normals.clear();      // Clear input normals

  const auto t0 = std::chrono::steady_clock::now();
  cloud.gridDownsample(0.005f);
  const auto t1 = std::chrono::steady_clock::now();

  RobustNormalEstimation3f ne{ConstPointsView(cloud.points)};
  ne.setViewPoint(0.0f, 0.0f, 0.0f);
  ne.covarianceMethod().setChiSquareThreshold(6.25f).setNumberOfTrials(2).setNumberOfRefinements(1);      // 90% confidence ellipsoid
  cloud.normals = ne.getNormalsKNN(12);

  const size_t total = cloud.size();
  cloud.removeInvalidNormals();
  const auto t2 = std::chrono::steady_clock::now();

  std::printf("Downsampled points: %zu\n", total);
  std::printf("Valid normals: %zu\n", cloud.size());
  std::printf("Invalid normals: %zu\n", total - cloud.size());
  std::printf("Downsampling time: %.2fms\n", std::chrono::duration<double, std::milli>(t1 - t0).count());
  std::printf("Estimation time: %.2fms\n", std::chrono::duration<double, std::milli>(t2 - t1).count());
  return 0;
}

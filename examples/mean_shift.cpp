// examples/mean_shift.cpp -- the flow of cilantro's examples/mean_shift.cpp on the GPU engine: three Gaussian blobs of 500 points each
// (unit variance, lifted by 10 along z, pushed 2.5 apart along random directions), clustered by mean shift with a flat kernel of radius
// 2, every point a seed.
//
//   g++ -O2 -std=c++17 -Iinclude examples/mean_shift.cpp -o mean_shift -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./mean_shift
//
// Differs from the reference example only where the missing pieces force it: no visualizer -- the cluster count, the iteration count, the
// size range and the modes are printed.
#include <cilantro_hip/clustering.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

using namespace cilantro_hip;

static std::vector<float> three_blobs() {
  std::default_random_engine rng;
  std::normal_distribution<float> normal(0.0f, 1.0f);
  const size_t per_blob = 500, blobs = 3;
  std::vector<float> xyz(3 * blobs * per_blob);
  for (float& v : xyz) v = normal(rng);
  for (size_t j = 0; j < blobs * per_blob; ++j) xyz[3 * j + 2] += 10.0f;
  for (size_t b = 0; b < blobs; ++b) {      // every blob pushed 2.5 along a random direction
    float dir[3];
    for (float& v : dir) v = normal(rng);
    const float scale = 2.5f / std::sqrt(dir[0] * dir[0] + dir[1] * dir[1] + dir[2] * dir[2]);
    for (size_t j = 0; j < per_blob; ++j)
      for (int k = 0; k < 3; ++k) xyz[3 * (b * per_blob + j) + k] += scale * dir[k];
  }
  return xyz;
}

int main() {
  const std::vector<float> points = three_blobs();
  std::printf("Number of points: %zu\n", points.size() / 3);

  MeanShift3f<> ms{ConstPointsView(points)};
  const auto t0 = std::chrono::steady_clock::now();
  ms.cluster(2.0f, 5000, 0.2f, 1e-7f, UnityWeightEvaluator<float>());      // flat kernel
  const double elapsed = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Clustering time: %.2fms\n", elapsed);
  std::printf("Number of clusters: %zu\n", ms.getNumberOfClusters());
  std::printf("Performed mean shift iterations: %zu\n", ms.getNumberOfPerformedIterations());
  const auto& cpi = ms.getClusterToPointIndicesMap();
  size_t mins = points.size() / 3, maxs = 0;
  for (const auto& c : cpi) { mins = c.size() < mins ? c.size() : mins; maxs = c.size() > maxs ? c.size() : maxs; }
  std::printf("Cluster size range is: [%zu,%zu]\n", mins, maxs);
  const auto& modes = ms.getClusterModes();
  for (size_t c = 0; c < cpi.size() && c < 10; ++c) std::printf("  mode %zu: (%.4f, %.4f, %.4f), %zu seeds\n", c, modes[3 * c], modes[3 * c + 1], modes[3 * c + 2], cpi[c].size());
  return 0;
}

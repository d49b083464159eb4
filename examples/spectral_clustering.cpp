// examples/spectral_clustering.cpp -- the flow of cilantro's examples/spectral_clustering.cpp on the GPU engine: two concentric shells
// (1500 points of radius 1, 200 of radius 0.3, lifted by 4 along z), a 30-nearest-neighbour graph weighted by an RBF kernel and made
// symmetric, and spectral clustering with at most 4 clusters, the number estimated from the eigenvalues, on the random-walk Laplacian.
//
//   g++ -O2 -std=c++17 -Iinclude examples/spectral_clustering.cpp -o spectral_clustering -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./spectral_clustering
//
// Differs from the reference example only where the missing pieces force it: no visualizer -- the counts the reference prints, the
// eigenvalues and the solver's figures are printed; `--describe` prints the set-up and needs no device.
#include <cilantro_hip/clustering.hpp>
#include <cilantro_hip/normal_estimation.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace cilantro_hip;

static std::vector<float> two_shells() {
  std::default_random_engine rng;
  std::uniform_real_distribution<float> uniform(-1.0f, 1.0f);      // setRandom().normalize()
  std::vector<float> xyz(3 * 1700);
  for (size_t i = 0; i < 1700; ++i) {
    float v[3], norm = 0.0f;
    do {
      for (float& c : v) c = uniform(rng);
      norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    } while (norm == 0.0f);
    const float scale = (i < 1500 ? 1.0f : 0.3f) / norm;
    for (int k = 0; k < 3; ++k) xyz[3 * i + k] = scale * v[k];
    xyz[3 * i + 2] += 4.0f;
  }
  return xyz;
}

int main(int argc, char** argv) {
  const std::vector<float> points = two_shells();
  const size_t max_num_clusters = 4;
  std::printf("Number of points: %zu\n", points.size() / 3);
  if (argc >= 2 && !std::strcmp(argv[1], "--describe")) {
    std::printf("30 neighbours, RBF kernel (sigma 1), forced symmetry, at most %zu clusters, estimated, NORMALIZED_RANDOM_WALK\n", max_num_clusters);
    return 0;
  }

  // Build neighborhood graph: 30 neighbors
  const NeighborhoodSet nn = KDTree3f(ConstPointsView(points)).kNNSearch(ConstPointsView(points), 30);
  const SparseAffinities affinities = getNNGraphFunctionValueSparseMatrix(nn, RBFKernelWeightEvaluator<float>(), true);

  const auto t0 = std::chrono::steady_clock::now();
  SpectralClusteringXf<> sc(affinities, max_num_clusters, true, GraphLaplacianType::NORMALIZED_RANDOM_WALK);
  const double elapsed = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Clustering time: %.2fms\n", elapsed);
  std::printf("Number of clusters: %zu\n", sc.getNumberOfClusters());
  std::printf("Performed k-means iterations: %zu\n", sc.getNumberOfPerformedIterations());
  const auto& cpi = sc.getClusterToPointIndicesMap();
  size_t mins = points.size() / 3, maxs = 0;
  for (const auto& c : cpi) { mins = c.size() < mins ? c.size() : mins; maxs = c.size() > maxs ? c.size() : maxs; }
  std::printf("Cluster size range is: [%zu,%zu]\n", mins, maxs);
  std::printf("Eigenvalues:");
  for (float v : sc.getComputedEigenValues()) std::printf(" %.6g", v);
  const cilhip_spectral_result& r = sc.getSolverResult();
  std::printf("\nSolver: %zu outer iterations, %zu block products, largest residual %.3g\n", r.outer_iterations, r.block_products, r.max_residual);
  return 0;
}

// tests/cpp/test_spectral.cpp -- the C++ mirror of spectral clustering (include/cilantro_hip/clustering.hpp: SpectralClusteringXf, KMeansXf,
// getNNGraphFunctionValueSparseMatrix, estimateNumberOfClustersEigengap), driven by tests/test_spectral_refs_cpu.py (build; the host half)
// and tests/test_gpu_spectral.py (`run`):
//   test_spectral host
//   test_spectral run      three blobs of 60 points, 8 neighbours -> 3 clusters of 60
#include <cilantro_hip/clustering.hpp>
#include <cilantro_hip/normal_estimation.hpp>

#include <cstdio>
#include <cstring>
#include <random>

using namespace cilantro_hip;

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // what needs no device: the eigengap rule, the defaults, the enum's codes, the refusals of the entries
      if (estimateNumberOfClustersEigengap(std::vector<float>{0.0f, 0.0f, 0.0f, 0.5f, 0.6f}, 4) != 3) return 1;
      if (estimateNumberOfClustersEigengap(std::vector<float>{0.25f, 0.25f, 0.25f}, 2) != 2) return 1;      // all equal: max_num_clusters
      if (estimateNumberOfClustersEigengap(std::vector<float>{0.5f, 0.6f, 0.65f}, 2) != 1) return 1;        // no gap above ev[0]: max_ind stays 0
      if ((int)GraphLaplacianType::UNNORMALIZED != 0 || (int)GraphLaplacianType::NORMALIZED_SYMMETRIC != 1 || (int)GraphLaplacianType::NORMALIZED_RANDOM_WALK != 2) return 1;
      cilhip_spectral_params prm;
      cilhip_spectral_default_params(&prm);
      if (prm.max_num_clusters != 2 || prm.estimate_num_clusters != 0 || prm.laplacian_type != 2 || prm.max_outer != 1000 || prm.degree != 24 || prm.guard != 3) return 1;
      bool threw = false;
      try { SparseAffinities::fromCSR(2, {0, 2, 3}, {1, 0, 1}, {1.0f, 1.0f, 1.0f}); } catch (const std::runtime_error&) { threw = true; }      // (row 0: columns descend)
      if (!threw) return 1;
      threw = false;
      try { SpectralClusteringXf<> sc(SparseAffinities(), 2); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;
      std::printf("host OK\n");
      return 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "run")) {
      std::default_random_engine rng(3);
      std::normal_distribution<float> normal(0.0f, 0.05f);
      std::vector<float> xyz(3 * 180);
      for (size_t i = 0; i < 180; ++i)
        for (int k = 0; k < 3; ++k) xyz[3 * i + k] = normal(rng) + (k == (int)(i / 60) ? 2.0f : 0.0f);
      const NeighborhoodSet nn = KDTree3f(ConstPointsView(xyz)).kNNSearch(ConstPointsView(xyz), 8);
      const SparseAffinities W = getNNGraphFunctionValueSparseMatrix(nn, RBFKernelWeightEvaluator<float>(1.0f), true);
      if (W.rows() != 180 || W.nonZeros() < 180 * 8) return 1;
      SpectralClusteringXf<> sc(W, 4, true, GraphLaplacianType::NORMALIZED_RANDOM_WALK, 100, std::numeric_limits<float>::epsilon(), false, {0, 60, 120});
      if (sc.getNumberOfClusters() != 3 || sc.getEmbeddingDimension() != 3 || sc.getComputedEigenValues().size() != 5) return 1;
      for (size_t i = 0; i < 180; ++i)
        if (sc.getPointToClusterIndexMap()[i] != i / 60) return 1;
      SpectralClustering3f<> sc3(W, GraphLaplacianType::NORMALIZED_SYMMETRIC, 100, std::numeric_limits<float>::epsilon(), false, {0, 60, 120});
      for (const auto& c : sc3.getClusterToPointIndicesMap())
        if (c.size() != 60) return 1;
      std::printf("run OK: %zu clusters\n", sc.getNumberOfClusters());
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
  std::fprintf(stderr, "usage: test_spectral host | run\n");
  return 2;
}

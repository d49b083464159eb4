// examples/mean_shift_nd.cpp -- the three blobs of examples/mean_shift.cpp carried into 6-D: every point is followed by a unit normal, the
// joint feature mean shift is most often run on.  The blobs keep their positions (unit variance, lifted by 10 along z, pushed 2.5 apart
// along random directions); each blob's normals scatter (sigma 0.1) around a direction of its own.  Flat kernel of radius 2, every
// point a seed, through MeanShiftXf (cilhip_mean_shift_nd: exhaustive, exact, 1 to 16 dimensions).
//
//   g++ -O2 -std=c++17 -Iinclude examples/mean_shift_nd.cpp -o mean_shift_nd -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./mean_shift_nd
//
// No visualizer: the cluster count, the iteration count, the size range and the modes are printed.
#include <cilantro_hip/clustering.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

using namespace cilantro_hip;

static std::vector<float> three_blobs_with_normals() {
  std::default_random_engine rng;
  std::normal_distribution<float> normal(0.0f, 1.0f);
  const size_t per_blob = 500, blobs = 3, dim = 6;
  std::vector<float> f(dim * blobs * per_blob);
  for (size_t b = 0; b < blobs; ++b) {
    float push[3], axis[3];
    for (float& v : push) v = normal(rng);
    for (float& v : axis) v = normal(rng);
    const float scale = 2.5f / std::sqrt(push[0] * push[0] + push[1] * push[1] + push[2] * push[2]);
    for (size_t j = 0; j < per_blob; ++j) {
      float* row = f.data() + dim * (b * per_blob + j);
      for (int k = 0; k < 3; ++k) row[k] = normal(rng) + scale * push[k];      // the point: pushed 2.5 along a random direction
      row[2] += 10.0f;
      float nrm[3], len = 0.0f;
      for (int k = 0; k < 3; ++k) { nrm[k] = axis[k] + 0.1f * normal(rng); len += nrm[k] * nrm[k]; }
      for (int k = 0; k < 3; ++k) row[3 + k] = nrm[k] / std::sqrt(len);      // its unit normal
    }
  }
  return f;
}

int main() {
  const size_t dim = 6;
  const std::vector<float> features = three_blobs_with_normals();
  std::printf("Number of points: %zu (dimension %zu)\n", features.size() / dim, dim);

  MeanShiftXf<> ms{ConstDataView(features, dim)};
  const auto t0 = std::chrono::steady_clock::now();
  ms.cluster(2.0f, 5000, 0.2f, 1e-7f, UnityWeightEvaluator<float>());      // flat kernel
  const double elapsed = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Clustering time: %.2fms\n", elapsed);
  std::printf("Number of clusters: %zu\n", ms.getNumberOfClusters());
  std::printf("Performed mean shift iterations: %zu\n", ms.getNumberOfPerformedIterations());
  const auto& cpi = ms.getClusterToPointIndicesMap();
  size_t mins = features.size() / dim, maxs = 0;
  for (const auto& c : cpi) { mins = c.size() < mins ? c.size() : mins; maxs = c.size() > maxs ? c.size() : maxs; }
  std::printf("Cluster size range is: [%zu,%zu]\n", mins, maxs);
  const auto& modes = ms.getClusterModes();
  for (size_t c = 0; c < cpi.size() && c < 10; ++c) {
    std::printf("  mode %zu: (", c);
    for (size_t k = 0; k < dim; ++k) std::printf("%s%.4f", k ? ", " : "", modes[dim * c + k]);
    std::printf("), %zu seeds\n", cpi[c].size());
  }
  return 0;
}

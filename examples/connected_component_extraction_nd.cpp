// examples/connected_component_extraction_nd.cpp -- the three blobs of examples/mean_shift_nd.cpp carried into 6-D: every point is followed
// by a unit normal, and the 6-D rows are the points that are segmented.  Each blob's normals scatter (sigma 0.1) around a direction of its
// own.  Two rows are joined when they are within a radius of 1.5 (squared: 2.25) in the joint space, closer than 1.2 there (the distance
// clause) and their normals are within 30 degrees (the normals clause; an N-D evaluator's normals have dim components: the row's normal,
// zero-padded in front): a distance + normals evaluator over N-D views, through ConnectedComponentExtractionXf
// (cilhip_connected_components_nd: exact, 1 to 16 dimensions, no neighbour list is written).
//
//   g++ -O2 -std=c++17 -Iinclude examples/connected_component_extraction_nd.cpp -o connected_component_extraction_nd -Lcilantro_amd/lib
//       -lcilantro_hip -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./connected_component_extraction_nd
//
// No visualizer: the segment count, the sizes, the form that ran and the tile pairs tested / total are printed.
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
  const size_t n = features.size() / dim;
  std::printf("Number of points: %zu (dimension %zu)\n", n, dim);

  // the 6-component vectors the normals clause compares: (0, 0, 0, nx, ny, nz) -- their dot product is the normals'
  std::vector<float> directions(features.size(), 0.0f);
  for (size_t i = 0; i < n; ++i)
    for (size_t k = 3; k < dim; ++k) directions[dim * i + k] = features[dim * i + k];

  ConnectedComponentExtractionXf<> cce{ConstDataView(features, dim)};
  const RadiusNeighborhoodSpecification<float> nh(1.5f * 1.5f);
  const PointsNormalsProximityEvaluator evaluator(ConstDataView(directions, dim), 1.2f * 1.2f, 30.0f * (float)M_PI / 180.0f);
  const auto t0 = std::chrono::steady_clock::now();
  cce.segment(nh, evaluator, 5, n);
  const double elapsed = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Segmentation time: %.2fms\n", elapsed);
  std::printf("Number of segments: %zu\n", cce.getNumberOfClusters());
  const auto& cpi = cce.getClusterToPointIndicesMap();
  std::printf("Segment sizes:");
  for (size_t c = 0; c < cpi.size() && c < 12; ++c) std::printf(" %zu", cpi[c].size());
  std::printf("%s\n", cpi.size() > 12 ? " ..." : "");
  std::printf("Unlabeled points (segments below 5 points): %zu\n", cce.getUnlabeledPointIndices().size());
  const cilhip_ccn_stats& st = cce.getLastStats();
  std::printf("Form %d, sweep axis %zu, tile pairs tested / total: %zu / %zu, %zu launch(es)\n", st.form_used, st.axis, st.tiles_tested, st.tiles_total, st.launches);
  return 0;
}

// The C++ mirrors of DESIGN.md section 19: MultidimensionalScaling and PrincipalComponentAnalysis.
//   test_mds_pca host   what needs no device: the dimension estimate, argument refusals
//   test_mds_pca run    a 3-D cloud: MDS of its squared distances against PCA's projection (the same coordinates up to a sign per axis)
#include <cilantro_hip/multidimensional_scaling.hpp>
#include <cilantro_hip/principal_component_analysis.hpp>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace cilantro_hip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static int host() {
  CHECK(estimateEmbeddingDimensionEigengap({500.0f, 500.0f, 5.0f, 0.0f}, 3) == 2);
  CHECK(estimateEmbeddingDimensionEigengap({2.0f, 2.0f, 2.0f}, 2) == 2);
  std::vector<float> d(9, 1.0f), emb(6), ev(3);
  cilhip_mds_params prm;
  cilhip_mds_default_params(&prm);
  CHECK(prm.max_dim == 2 && prm.estimate_dim == 0 && prm.distances_are_squared == 1 && prm.max_outer == 1000);
  cilhip_mds_result res;
  CHECK(cilhip_mds_embedding(0, d.data(), 2, CILHIP_MEM_HOST, &prm, emb.data(), ev.data(), &res) == CILHIP_ERR_INVALID);
  CHECK(std::strstr(cilhip_last_error(nullptr), "M1") != nullptr);
  bool threw = false;
  try { PrincipalComponentAnalysisXf bad(d.data(), 3, 17); } catch (const std::invalid_argument&) { threw = true; }
  CHECK(threw);
  if (!failures) std::printf("host OK\n");
  return failures;
}

static int run() {
  const size_t n = 200;
  std::mt19937 rng(5);
  std::normal_distribution<float> g(0.0f, 1.0f);
  std::vector<float> p(3 * n), d(n * n);
  const float scale[3] = {3.0f, 1.5f, 0.6f};
  for (size_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) p[3 * i + k] = scale[k] * g(rng) + 10.0f;
  for (size_t i = 0; i < n; ++i)
    for (size_t j = 0; j < n; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) { const double df = (double)p[3 * i + k] - (double)p[3 * j + k]; s += df * df; }
      d[i * n + j] = (float)s;
    }
  MultidimensionalScaling3f mds(d.data(), n);
  PrincipalComponentAnalysis3f pca(p.data(), n);
  CHECK(mds.getEmbeddingDimension() == 3 && pca.isValid());
  const std::vector<float> proj = pca.project(p.data(), n, 3);
  const std::vector<float>& y = mds.getEmbeddedPoints();
  double worst = 0.0;
  for (int k = 0; k < 3; ++k) {
    double dot = 0.0;
    for (size_t i = 0; i < n; ++i) dot += (double)y[3 * i + k] * (double)proj[3 * i + k];
    const double sign = dot < 0.0 ? -1.0 : 1.0;
    for (size_t i = 0; i < n; ++i) worst = std::fmax(worst, std::fabs((double)y[3 * i + k] - sign * (double)proj[3 * i + k]));
    // lambda_mds = (n - 1) lambda_pca
    CHECK(std::fabs((double)mds.getComputedEigenValues()[k] - (double)(n - 1) * (double)pca.getEigenValues()[k]) <= 1e-4 * (double)mds.getComputedEigenValues()[k]);
  }
  std::printf("MDS against PCA: largest coordinate difference %.3g\n", worst);
  CHECK(worst <= 1e-3);      // (coordinates of size 10; the f32 distances carry 1e-7 * 400 of rounding each)
  const std::vector<float> back = pca.reconstruct(proj.data(), n, 3);
  double rt = 0.0;
  for (size_t i = 0; i < 3 * n; ++i) rt = std::fmax(rt, std::fabs((double)back[i] - (double)p[i]));
  std::printf("project / reconstruct round trip: %.3g\n", rt);
  CHECK(rt <= 1e-4);
  MultidimensionalScalingXf est(d.data(), n, 2, true);
  CHECK(est.getComputedEigenValues().size() == 3 && est.getEmbeddingDimension() == estimateEmbeddingDimensionEigengap(est.getComputedEigenValues(), 2));
  if (!failures) std::printf("run OK\n");
  return failures;
}

int main(int argc, char** argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "host")) return host();
  if (argc >= 2 && !std::strcmp(argv[1], "run")) return run();
  std::printf("usage: test_mds_pca host | run\n");
  return 0;
}

// tests/cpp/test_robust_normals.cpp -- the C++ mirror of the robust normal estimation (include/cilantro_hip/normal_estimation.hpp:
// RobustNormalEstimation3f), driven by tests/test_robust_normal_refs_cpu.py (build; the host half) and tests/test_gpu_robust_normals.py (the
// results, against the Python mirror's):
//   test_robust_normals host
//   test_robust_normals run <points.f32> <out prefix> <k> <radius or 0> <trials> <refinements> <ratio> <chi> <seed> <view point: 0 | 1 (the origin)>
//       writes <prefix>.normals.f32, <prefix>.curvature.f32, <prefix>.masks.u32 and <prefix>.inliers.u8
#include <cilantro_hip/normal_estimation.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace cilantro_hip;

template <typename T>
static void dump(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fclose(f); throw std::runtime_error("short write " + path); }
  std::fclose(f);
}
static std::vector<float> slurp(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot read " + path);
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<float> v((size_t)bytes / sizeof(float));
  if (!v.empty() && std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) { std::fclose(f); throw std::runtime_error("short read " + path); }
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // what needs no device: the defaults, the setters' chaining, the refusals
      cilhip_mcd_params prm;
      cilhip_mcd_params_default(&prm);
      if (prm.num_trials != 6 || prm.num_refinements != 3 || prm.inlier_ratio != 0.75f || prm.chi_square_threshold != -1.0f || prm.k != 0 || prm.seed != 0 ||
          !(prm.max_sq_dist > 3e38f))
        return 1;
      const std::vector<float> pts(30, 0.25f);
      RobustNormalEstimation3f ne{ConstPointsView(pts)};
      if (ne.covarianceMethod().getNumberOfTrials() != 6 || ne.covarianceMethod().getNumberOfRefinements() != 3 || ne.covarianceMethod().getInlierRatio() != 0.75f ||
          ne.covarianceMethod().getChiSquareThreshold() != -1.0f)
        return 1;
      ne.covarianceMethod().setChiSquareThreshold(6.25f).setNumberOfTrials(2).setNumberOfRefinements(1).setInlierRatio(0.5f).setSeed(7);
      if (ne.covarianceMethod().getNumberOfTrials() != 2 || ne.covarianceMethod().getNumberOfRefinements() != 1 || ne.covarianceMethod().getInlierRatio() != 0.5f ||
          ne.covarianceMethod().getChiSquareThreshold() != 6.25f || ne.covarianceMethod().getSeed() != 7)
        return 1;
      if (ne.getViewPoint()[0] == ne.getViewPoint()[0]) return 1;      // NaN: no view point by default
      ne.setViewPoint(0.0f, 0.0f, 0.0f);
      int refused = 0;
      std::vector<float> n, c;
      try { ne.getNormalsRadius(0.1f); } catch (const std::invalid_argument& e) { refused += std::strstr(e.what(), "KNNInRadius") != nullptr; }
      try { ne.getCurvatureRadius(0.1f); } catch (const std::invalid_argument& e) { refused += std::strstr(e.what(), "KNNInRadius") != nullptr; }
      try { ne.getNormalsAndCurvatureRadius(n, c, 0.1f); } catch (const std::invalid_argument& e) { refused += std::strstr(e.what(), "KNNInRadius") != nullptr; }
      if (refused != 3) return 1;
      // an argument the C entry refuses (k = 33) throws with the entry's own words, without a device
      try { ne.getNormalsKNN(33); return 1; } catch (const std::runtime_error& e) { if (!std::strstr(e.what(), "k must be in 1..32")) return 1; }
      std::printf("host OK\n");
      return 0;
    }
    if (argc == 12 && !std::strcmp(argv[1], "run")) {
      const std::vector<float> pts = slurp(argv[2]);
      const std::string pre = argv[3];
      const size_t k = (size_t)std::atoll(argv[4]);
      const float radius = (float)std::atof(argv[5]);
      RobustNormalEstimation3f ne{ConstPointsView(pts)};
      ne.covarianceMethod().setNumberOfTrials(std::atoi(argv[6])).setNumberOfRefinements(std::atoi(argv[7])).setInlierRatio((float)std::atof(argv[8]))
          .setChiSquareThreshold((float)std::atof(argv[9])).setSeed(std::strtoull(argv[10], nullptr, 10));
      if (std::atoi(argv[11])) ne.setViewPoint(0.0f, 0.0f, 0.0f);
      std::vector<float> normals, curvature;
      std::vector<uint32_t> masks;
      std::vector<uint8_t> inliers;
      if (radius > 0.0f) {
        ne.getNormalsAndCurvatureKNNInRadius(normals, curvature, k, radius);
        ne.getSubsetMasksAndInliersKNNInRadius(masks, inliers, k, radius);
        if (std::memcmp(ne.getNormalsKNNInRadius(k, radius).data(), normals.data(), 4 * normals.size()) ||
            std::memcmp(ne.getCurvatureKNNInRadius(k, radius).data(), curvature.data(), 4 * curvature.size()))
          return 1;
      } else {
        ne.getNormalsAndCurvatureKNN(normals, curvature, k);
        ne.getSubsetMasksAndInliersKNN(masks, inliers, k);
        if (std::memcmp(ne.getNormalsKNN(k).data(), normals.data(), 4 * normals.size()) || std::memcmp(ne.getCurvatureKNN(k).data(), curvature.data(), 4 * curvature.size())) return 1;
      }
      dump(pre + ".normals.f32", normals);
      dump(pre + ".curvature.f32", curvature);
      dump(pre + ".masks.u32", masks);
      dump(pre + ".inliers.u8", inliers);
      std::printf("run OK\n");
      return 0;
    }
    std::fprintf(stderr, "usage: test_robust_normals host | run <points.f32> <prefix> <k> <radius or 0> <trials> <refinements> <ratio> <chi> <seed> <0|1>\n");
    return 2;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 3;
  }
}

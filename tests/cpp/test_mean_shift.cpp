// tests/cpp/test_mean_shift.cpp -- the C++ mirror of mean-shift clustering (include/cilantro_hip/clustering.hpp: MeanShift3f), driven by
// tests/test_meanshift_refs_cpu.py (build; the host half) and tests/test_gpu_mean_shift.py (the results, against the Python mirror's):
//   test_mean_shift host
//   test_mean_shift run <points.f32> <seeds.f32 or -> <out prefix> <radius> <max_iter> <cluster_tol> <convergence_tol> <kind> <sigma>
//       writes <prefix>.shifted.f32, <prefix>.modes.f32, <prefix>.labels.u64, <prefix>.members.u64 (the clusters' lists one after the
//       other), <prefix>.sizes.u64 and <prefix>.iters.u64
#include <cilantro_hip/clustering.hpp>

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

template <class Ev>
static void go(MeanShift3f<>& ms, const std::vector<float>* seeds, float r, size_t it, float ct, float cv, const Ev& ev) {
  if (seeds) ms.cluster(ConstPointsView(*seeds), r, it, ct, cv, ev);
  else ms.cluster(r, it, ct, cv, ev);
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // what needs no device: the evaluators' descriptions, the defaults, a run without a single seed
      if (UnityWeightEvaluator<float>().kind() != 0 || IdentityWeightEvaluator<float>().kind() != 1 || RBFKernelWeightEvaluator<float>(0.5f).kind() != 2) return 1;
      if (RBFKernelWeightEvaluator<float>(0.5f).sigma() != 0.5f) return 1;
      cilhip_ms_params prm;
      cilhip_ms_default_params(&prm);
      if (prm.convergence_tol != std::numeric_limits<float>::epsilon() || prm.kernel_kind != 0 || prm.form != 0) return 1;
      const std::vector<float> none;
      MeanShift3f<> ms{ConstPointsView(none)};
      ms.cluster(1.0f, 10, 0.1f);
      if (ms.getNumberOfClusters() != 0 || ms.getNumberOfPerformedIterations() != 0 || !ms.getShiftedSeeds().empty()) return 1;
      const std::vector<float> pts(30, 0.25f);
      MeanShift3f<> ms2{ConstPointsView(pts)};
      ms2.cluster(ConstPointsView(none), 1.0f, 10, 0.1f);
      if (ms2.getNumberOfClusters() != 0 || ms2.getNumberOfPoints() != 0) return 1;
      std::printf("host OK\n");
      return 0;
    }
    if (argc >= 11 && !std::strcmp(argv[1], "run")) {
      const std::vector<float> points = slurp(argv[2]);
      const bool own = std::strcmp(argv[3], "-") != 0;
      const std::vector<float> seeds = own ? slurp(argv[3]) : std::vector<float>();
      const std::string pre = argv[4];
      const float r = (float)std::atof(argv[5]), ct = (float)std::atof(argv[7]), cv = (float)std::atof(argv[8]), sigma = (float)std::atof(argv[10]);
      const size_t it = (size_t)std::atoll(argv[6]);
      const int kind = std::atoi(argv[9]);
      MeanShift3f<> ms{ConstPointsView(points)};
      if (kind == 0) go(ms, own ? &seeds : nullptr, r, it, ct, cv, UnityWeightEvaluator<float>());
      else if (kind == 1) go(ms, own ? &seeds : nullptr, r, it, ct, cv, IdentityWeightEvaluator<float>());
      else go(ms, own ? &seeds : nullptr, r, it, ct, cv, RBFKernelWeightEvaluator<float>(sigma));
      dump(pre + ".shifted.f32", ms.getShiftedSeeds());
      dump(pre + ".modes.f32", ms.getClusterModes());
      std::vector<uint64_t> labels(ms.getPointToClusterIndexMap().begin(), ms.getPointToClusterIndexMap().end()), members, sizes;
      for (const auto& c : ms.getClusterToPointIndicesMap()) { sizes.push_back(c.size()); members.insert(members.end(), c.begin(), c.end()); }
      dump(pre + ".labels.u64", labels);
      dump(pre + ".members.u64", members);
      dump(pre + ".sizes.u64", sizes);
      dump(pre + ".iters.u64", std::vector<uint64_t>{(uint64_t)ms.getNumberOfPerformedIterations()});
      std::printf("run OK: %zu clusters, %zu iterations\n", ms.getNumberOfClusters(), ms.getNumberOfPerformedIterations());
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  std::fprintf(stderr, "usage: test_mean_shift host | run <points.f32> <seeds.f32 or -> <prefix> <radius> <max_iter> <cluster_tol> <convergence_tol> <kind> <sigma>\n");
  return 64;
}

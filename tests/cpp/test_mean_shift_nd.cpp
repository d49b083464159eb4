// tests/cpp/test_mean_shift_nd.cpp -- the C++ mirrors of mean-shift clustering in dim dimensions (include/cilantro_hip/clustering.hpp:
// MeanShiftXf, MeanShift2f), driven by tests/test_meanshift_nd_refs_cpu.py (build; the host half) and tests/test_gpu_mean_shift_nd.py
// (the results, against the Python mirror's):
//   test_mean_shift_nd host
//   test_mean_shift_nd run <dim> <points.f32> <seeds.f32 or -> <out prefix> <radius> <max_iter> <cluster_tol> <convergence_tol> <kind> <sigma>
//       (dim 2 goes through MeanShift2f)
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
static void go(MeanShiftXf<>& ms, const std::vector<float>* seeds, float r, size_t it, float ct, float cv, const Ev& ev) {
  if (seeds) ms.cluster(ConstDataView(*seeds, ms.getDimension()), r, it, ct, cv, ev);
  else ms.cluster(r, it, ct, cv, ev);
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // what needs no device: a run without a single seed, the dimension checks
      const std::vector<float> none;
      MeanShiftXf<> ms{ConstDataView(none, 6)};
      ms.cluster(1.0f, 10, 0.1f);
      if (ms.getNumberOfClusters() != 0 || ms.getNumberOfPerformedIterations() != 0 || !ms.getShiftedSeeds().empty() || ms.getDimension() != 6) return 1;
      const std::vector<float> pts(36, 0.25f);
      MeanShiftXf<> ms2{ConstDataView(pts, 9)};
      ms2.cluster(ConstDataView(none, 9), 1.0f, 10, 0.1f, 1e-4f, RBFKernelWeightEvaluator<float>(0.5f));
      if (ms2.getNumberOfClusters() != 0 || ms2.getNumberOfPoints() != 0) return 1;
      bool threw = false;
      try { ms2.cluster(ConstDataView(pts, 6), 1.0f, 10, 0.1f); } catch (const std::invalid_argument&) { threw = true; }      // seeds of another dimension
      if (!threw) return 1;
      threw = false;
      try { MeanShift2f<> bad{ConstDataView(pts, 3)}; } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;
      MeanShift2f<> two(pts.data(), 0);
      two.cluster(1.0f, 10, 0.1f);
      if (two.getNumberOfClusters() != 0 || two.getDimension() != 2) return 1;
      threw = false;
      try { MeanShiftXf<> wide{ConstDataView(pts.data(), 18, 2)}; wide.cluster(1.0f, 10, 0.1f); } catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "dim > 16") != nullptr; }
      if (!threw) return 1;      // refused by the entry, before any device
      std::printf("host OK\n");
      return 0;
    }
    if (argc >= 12 && !std::strcmp(argv[1], "run")) {
      const size_t dim = (size_t)std::atoll(argv[2]);
      const std::vector<float> points = slurp(argv[3]);
      const bool own = std::strcmp(argv[4], "-") != 0;
      const std::vector<float> seeds = own ? slurp(argv[4]) : std::vector<float>();
      const std::string pre = argv[5];
      const float r = (float)std::atof(argv[6]), ct = (float)std::atof(argv[8]), cv = (float)std::atof(argv[9]), sigma = (float)std::atof(argv[11]);
      const size_t it = (size_t)std::atoll(argv[7]);
      const int kind = std::atoi(argv[10]);
      MeanShiftXf<> any{ConstDataView(points, dim)};
      MeanShift2f<> two(points.data(), dim == 2 ? points.size() / 2 : 0);
      MeanShiftXf<>& ms = dim == 2 ? two : any;
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
  std::fprintf(stderr, "usage: test_mean_shift_nd host | run <dim> <points.f32> <seeds.f32 or -> <prefix> <radius> <max_iter> <cluster_tol> <convergence_tol> <kind> <sigma>\n");
  return 64;
}

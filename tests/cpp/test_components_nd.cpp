// tests/cpp/test_components_nd.cpp -- the C++ mirrors of connected-component segmentation in dim dimensions
// (include/cilantro_hip/clustering.hpp: ConnectedComponentExtractionXf, ConnectedComponentExtraction2f and the evaluators' N-D normals
// views), driven by tests/test_ccn_refs_cpu.py (build; the host half):
//   test_components_nd host
//   test_components_nd run <dim> <points.f32> <normals.f32 or -> <out prefix> <radius_sq> <max_distance> <max_angle> <form>
//       (dim 2 goes through ConnectedComponentExtraction2f; with normals: PointsNormalsProximityEvaluator, without: PointsProximityEvaluator)
//       writes <prefix>.labels.u64, <prefix>.members.u64 (the segments' lists one after the other) and <prefix>.sizes.u64
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

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // what needs no device: a run over no point, the dimension checks, the refusals of the entry
      const std::vector<float> none;
      ConnectedComponentExtractionXf<> cce{ConstDataView(none, 6)};
      cce.segment(RadiusNeighborhoodSpecification<float>(1.0f));
      if (cce.getNumberOfClusters() != 0 || cce.getNumberOfPoints() != 0 || cce.getDimension() != 6 || cce.getLastStats().tiles_total != 0 || !cce.getLabeledPointIndices().empty()) return 1;
      cce.segment(RadiusNeighborhoodSpecification<float>(1.0f), std::vector<size_t>(), PointsProximityEvaluator(0.5f), 2, 100);
      if (cce.getNumberOfClusters() != 0) return 1;
      const std::vector<float> pts(36, 0.25f);
      bool threw = false;
      try { ConnectedComponentExtraction2f<> bad{ConstDataView(pts, 3)}; } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;
      ConnectedComponentExtraction2f<> two(pts.data(), 0);
      two.segment(RadiusNeighborhoodSpecification<float>(1.0f));
      if (two.getNumberOfClusters() != 0 || two.getDimension() != 2) return 1;
      ConnectedComponentExtractionXf<> six{ConstDataView(pts, 6)};      // 6 points
      threw = false;
      try { six.segment(RadiusNeighborhoodSpecification<float>(1.0f), NormalsProximityEvaluator(ConstDataView(pts, 9), 0.1f)); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;      // 4 normals for 6 points
      threw = false;
      try { six.segment(RadiusNeighborhoodSpecification<float>(1.0f), PointsNormalsProximityEvaluator(ConstPointsView(pts.data(), 6), 1.0f, 0.1f)); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;      // 3-component normals over 6-component points
      threw = false;
      try { six.segment(RadiusNeighborhoodSpecification<float>(1.0f), std::vector<size_t>{6}); } catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;      // a seed past the points
      threw = false;
      try { ConnectedComponentExtraction3f<> three{ConstPointsView(pts.data(), 12)}; three.segment(RadiusNeighborhoodSpecification<float>(1.0f), NormalsProximityEvaluator(ConstDataView(pts.data(), 2, 12), 0.1f)); }
      catch (const std::invalid_argument&) { threw = true; }
      if (!threw) return 1;      // the 3-D class takes 3-component normals only
      threw = false;
      try { ConnectedComponentExtractionXf<> wide{ConstDataView(pts.data(), 18, 2)}; wide.segment(RadiusNeighborhoodSpecification<float>(1.0f)); }
      catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "dim > 16") != nullptr; }
      if (!threw) return 1;      // refused by the entry, before any device
      threw = false;
      try { ConnectedComponentExtractionXf<> odd{ConstDataView(pts, 6), 0, 3}; odd.segment(RadiusNeighborhoodSpecification<float>(1.0f)); }
      catch (const std::runtime_error& e) { threw = std::strstr(e.what(), "form") != nullptr; }
      if (!threw) return 1;
      std::printf("host OK\n");
      return 0;
    }
    if (argc >= 10 && !std::strcmp(argv[1], "run")) {
      const size_t dim = (size_t)std::atoll(argv[2]);
      const std::vector<float> points = slurp(argv[3]);
      const bool with_normals = std::strcmp(argv[4], "-") != 0;
      const std::vector<float> normals = with_normals ? slurp(argv[4]) : std::vector<float>();
      const std::string pre = argv[5];
      const float r2 = (float)std::atof(argv[6]), dist = (float)std::atof(argv[7]), angle = (float)std::atof(argv[8]);
      const int form = std::atoi(argv[9]);
      ConnectedComponentExtractionXf<> any{ConstDataView(points, dim), 0, form};
      ConnectedComponentExtraction2f<> two{ConstDataView(points.data(), 2, dim == 2 ? points.size() / 2 : 0), 0, form};
      ConnectedComponentExtractionXf<>& cce = dim == 2 ? two : any;
      if (with_normals) cce.segment(RadiusNeighborhoodSpecification<float>(r2), PointsNormalsProximityEvaluator(ConstDataView(normals, dim), dist, angle));
      else cce.segment(RadiusNeighborhoodSpecification<float>(r2), PointsProximityEvaluator(dist));
      std::vector<uint64_t> labels(cce.getPointToClusterIndexMap().begin(), cce.getPointToClusterIndexMap().end()), members, sizes;
      for (const auto& c : cce.getClusterToPointIndicesMap()) { sizes.push_back(c.size()); members.insert(members.end(), c.begin(), c.end()); }
      dump(pre + ".labels.u64", labels);
      dump(pre + ".members.u64", members);
      dump(pre + ".sizes.u64", sizes);
      std::printf("run OK: %zu segments, form %d, %zu of %zu tile pairs\n", cce.getNumberOfClusters(), cce.getLastStats().form_used, cce.getLastStats().tiles_tested, cce.getLastStats().tiles_total);
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  std::fprintf(stderr, "usage: test_components_nd host | run <dim> <points.f32> <normals.f32 or -> <prefix> <radius_sq> <max_distance> <max_angle> <form>\n");
  return 64;
}

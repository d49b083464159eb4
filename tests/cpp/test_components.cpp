// tests/cpp/test_components.cpp -- the C++ mirror of connected-component segmentation (include/cilantro_hip/clustering.hpp) and
// PointCloud3f::removeInvalid* (point_cloud.hpp), driven by tests/test_components_refs_cpu.py (build; the host half) and
// tests/test_gpu_components.py (the labels, against the Python mirror's):
//   test_components host
//   test_components run <in.ply> <out prefix> <radius> <angle in degrees> <min segment size>
//       removeInvalidData(), then writes <prefix>.{p,n,c}.f32 (the cloud that was segmented) and the label arrays <prefix>.<variant>.u64 for
//       variant = normals (NormalsProximityEvaluator, all seeds), seeded (every 7th point a seed), pnc (PointsNormalsColorsProximityEvaluator,
//       negative angle) and plain (AlwaysTrueEvaluator)
#include <cilantro_hip/clustering.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>

using namespace cilantro_hip;

template <typename T>
static void dump(const std::string& path, const std::vector<T>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fclose(f); throw std::runtime_error("short write " + path); }
  std::fclose(f);
}

static PointCloud3f six() {      // point i has x = i; point 1 has a NaN coordinate, normal 3 an infinite entry, colour 4 a NaN
  PointCloud3f c;
  for (int i = 0; i < 6; ++i)
    for (int k = 0; k < 3; ++k) { c.points.push_back(k == 0 ? (float)i : 0.5f); c.normals.push_back(k == 2 ? 1.0f : 0.0f); c.colors.push_back(0.25f); }
  c.points[3 * 1 + 2] = std::numeric_limits<float>::quiet_NaN();
  c.normals[3 * 3 + 1] = std::numeric_limits<float>::infinity();
  c.colors[3 * 4] = std::numeric_limits<float>::quiet_NaN();
  return c;
}
static bool rows_are(const PointCloud3f& c, std::initializer_list<int> want) {
  if (c.size() != want.size() || c.normals.size() != c.points.size() || c.colors.size() != c.points.size()) return false;
  size_t i = 0;
  for (int w : want) {
    if (c.points[3 * i] != (float)w) return false;
    ++i;
  }
  return true;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // utilities/point_cloud.hpp:154-245: every hole, in ascending order, takes the last row that stays
      int bad = 0;
      { PointCloud3f c = six(); bad += !rows_are(c.removeInvalidPoints(), {0, 5, 2, 3, 4}); }
      { PointCloud3f c = six(); bad += !rows_are(c.removeInvalidNormals(), {0, 1, 2, 5, 4}); }
      { PointCloud3f c = six(); bad += !rows_are(c.removeInvalidColors(), {0, 1, 2, 3, 5}); }
      { PointCloud3f c = six(); bad += !rows_are(c.removeInvalidData(), {0, 5, 2}); }
      { PointCloud3f c = six(); c.normals.clear(); c.colors.clear(); c.removeInvalidNormals().removeInvalidColors(); bad += c.size() != 6; c.removeInvalidData(); bad += c.size() != 5 || c.points[3] != 5.0f; }
      { PointCloud3f c; c.removeInvalidData(); bad += c.size() != 0; }
      { PointCloud3f c = six(); for (float& v : c.points) v = std::numeric_limits<float>::quiet_NaN(); c.removeInvalidData(); bad += !c.isEmpty() || !c.normals.empty() || !c.colors.empty(); }
      // an empty cloud needs no device
      std::vector<float> none;
      ConnectedComponentExtraction3f<> cce{ConstPointsView(none)};
      cce.segment(RadiusNeighborhoodSpecification<float>(1.0f));
      bad += cce.getNumberOfClusters() != 0 || cce.getNumberOfPoints() != 0;
      if (bad) { std::printf("FAIL: %d host checks\n", bad); return 1; }
      std::printf("host OK\n");
      return 0;
    }
    if (argc >= 7 && !std::strcmp(argv[1], "run")) {
      PointCloud3f c(argv[2]);
      const std::string pre = argv[3];
      const float radius = (float)std::atof(argv[4]), angle = (float)(std::atof(argv[5]) * M_PI / 180.0);
      const size_t min_size = (size_t)std::atoll(argv[6]);
      if (!c.hasNormals() || !c.hasColors()) throw std::runtime_error("the input needs normals and colours");
      const size_t before = c.size();
      c.removeInvalidData();
      dump(pre + ".p.f32", c.points); dump(pre + ".n.f32", c.normals); dump(pre + ".c.f32", c.colors);
      const ConstPointsView p(c.points), n(c.normals), col(c.colors);
      const RadiusNeighborhoodSpecification<float> nh(radius * radius);
      ConnectedComponentExtraction3f<> cce(p);
      cce.segment(nh, NormalsProximityEvaluator(n, angle), min_size, c.size());
      dump(pre + ".normals.u64", cce.getPointToClusterIndexMap());
      std::printf("%zu components:", cce.getNumberOfClusters());
      for (const auto& s : cce.getClusterToPointIndicesMap()) std::printf(" %zu", s.size());
      std::printf("\n");
      // the accessors agree with each other
      size_t labelled = 0;
      for (size_t k = 0; k < cce.getNumberOfClusters(); ++k) {
        const auto& s = cce.getClusterToPointIndicesMap()[k];
        labelled += s.size();
        for (size_t j = 0; j < s.size(); ++j)
          if (cce.getPointToClusterIndexMap()[s[j]] != k || (j && s[j] <= s[j - 1])) throw std::runtime_error("cluster map and labels disagree");
      }
      if (cce.getLabeledPointIndices().size() != labelled || cce.getUnlabeledPointIndices().size() != c.size() - labelled || cce.getNumberOfPoints() != c.size())
        throw std::runtime_error("labelled / unlabelled counts disagree");
      std::vector<size_t> seeds;
      for (size_t i = 0; i < c.size(); i += 7) seeds.push_back(i);
      cce.segment(nh, seeds, NormalsProximityEvaluator(n, angle), 2);
      dump(pre + ".seeded.u64", cce.getPointToClusterIndexMap());
      cce.segment(nh, PointsNormalsColorsProximityEvaluator(n, col, 0.6f * radius * radius, -angle, 0.7f), 3, 500);
      dump(pre + ".pnc.u64", cce.getPointToClusterIndexMap());
      cce.segment(nh);
      dump(pre + ".plain.u64", cce.getPointToClusterIndexMap());
      std::printf("run OK: %zu -> %zu points\n", before, c.size());
      return 0;
    }
  } catch (const std::exception& e) {
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
  std::printf("usage: test_components host | run <in.ply> <prefix> <radius> <angle in degrees> <min segment size>\n");
  return 2;
}

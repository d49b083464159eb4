// tests/cpp/test_grid_downsample.cpp -- the C++ mirrors of the voxel-grid downsamplers (include/cilantro_hip/grid_downsampler.hpp)
// and PointCloud3f::gridDownsample / gridDownsampled (point_cloud.hpp), driven by tests/test_grid_downsample_cpu.py (build; without a
// device every mirror must throw) and tests/test_gpu_grid_downsample.py (the arrays, against the Python mirror's):
//   test_grid_downsample --expect-no-device
//   test_grid_downsample run <in.ply> <out prefix> <bin size> <min points in bin> <parallel 0|1>
//       writes <prefix>.<variant>.<p|n|c>.f32 (raw packed floats) for variant = p, pn, pc, pnc (the four classes), cloud (gridDownsample
//       on the cloud as read) and cloud_copy (gridDownsampled)
#include <cilantro_hip/grid_downsampler.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace cilantro_hip;

static void dump(const std::string& path, const std::vector<float>& v) {
  FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) throw std::runtime_error("cannot write " + path);
  if (!v.empty() && std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) { std::fclose(f); throw std::runtime_error("short write " + path); }
  std::fclose(f);
}

template <typename F>
static int must_throw(const char* what, F&& f) {
  try {
    f();
  } catch (const std::exception& e) {
    std::printf("%s: threw \"%s\"\n", what, e.what());
    return 0;
  }
  std::printf("FAIL: %s did not throw\n", what);
  return 1;
}

int main(int argc, char** argv) {
  try {
    if (argc >= 2 && !std::strcmp(argv[1], "--expect-no-device")) {
      PointCloud3f c;
      for (int i = 0; i < 300; ++i) { c.points.push_back(0.01f * (float)(i % 17)); c.normals.push_back(i % 3 == 2 ? 1.0f : 0.0f); c.colors.push_back(0.5f); }
      const ConstPointsView p(c.points), n(c.normals), col(c.colors);
      int bad = 0;
      bad += must_throw("PointsGridDownsampler3f", [&] { PointsGridDownsampler3f d(p, 0.05f); });
      bad += must_throw("PointsNormalsGridDownsampler3f", [&] { PointsNormalsGridDownsampler3f d(p, n, 0.05f); });
      bad += must_throw("PointsColorsGridDownsampler3f", [&] { PointsColorsGridDownsampler3f d(p, col, 0.05f, false); });
      bad += must_throw("PointsNormalsColorsGridDownsampler3f", [&] { PointsNormalsColorsGridDownsampler3f d(p, n, col, 0.05f); });
      bad += must_throw("PointCloud3f::gridDownsample", [&] { PointCloud3f q = c; q.gridDownsample(0.05f); });
      bad += must_throw("PointCloud3f::gridDownsampled", [&] { (void)c.gridDownsampled(0.05f, 2, false); });
      bad += must_throw("bin_size 0", [&] { PointsGridDownsampler3f d(p, 0.0f); });
      // an empty cloud needs no device
      PointCloud3f e;
      e.gridDownsample(0.05f);
      if (e.size() != 0) { std::printf("FAIL: empty cloud\n"); ++bad; }
      if (bad) return 1;
      std::printf("no-device OK\n");
      return 0;
    }
    if (argc >= 7 && !std::strcmp(argv[1], "run")) {
      PointCloud3f c(argv[2]);
      const std::string pre = argv[3];
      const float bin = (float)std::atof(argv[4]);
      const size_t min_pts = (size_t)std::atoll(argv[5]);
      const bool parallel = std::atoi(argv[6]) != 0;
      if (!c.hasNormals() || !c.hasColors()) throw std::runtime_error("the input needs normals and colours");
      const ConstPointsView p(c.points), n(c.normals), col(c.colors);
      std::vector<float> a, b, d;
      PointsGridDownsampler3f(p, bin, parallel).getDownsampledPoints(a, min_pts);
      dump(pre + ".p.p.f32", a);
      {
        const PointsNormalsGridDownsampler3f ds(p, n, bin, parallel);
        ds.getDownsampledPointsNormals(a, b, min_pts);
        dump(pre + ".pn.p.f32", a); dump(pre + ".pn.n.f32", b);
        if (ds.getDownsampledPoints(min_pts) != a || ds.getDownsampledNormals(min_pts) != b) throw std::runtime_error("getters disagree (pn)");
      }
      {
        const PointsColorsGridDownsampler3f ds(p, col, bin, parallel);
        ds.getDownsampledPointsColors(a, d, min_pts);
        dump(pre + ".pc.p.f32", a); dump(pre + ".pc.c.f32", d);
        if (ds.getDownsampledPoints(min_pts) != a || ds.getDownsampledColors(min_pts) != d) throw std::runtime_error("getters disagree (pc)");
      }
      {
        const PointsNormalsColorsGridDownsampler3f ds(p, n, col, bin, parallel);
        ds.getDownsampledPointsNormalsColors(a, b, d, min_pts);
        dump(pre + ".pnc.p.f32", a); dump(pre + ".pnc.n.f32", b); dump(pre + ".pnc.c.f32", d);
      }
      const PointCloud3f copy = c.gridDownsampled(bin, min_pts, parallel);
      dump(pre + ".cloud_copy.p.f32", copy.points); dump(pre + ".cloud_copy.n.f32", copy.normals); dump(pre + ".cloud_copy.c.f32", copy.colors);
      const size_t before = c.size();
      c.gridDownsample(bin, min_pts, parallel);
      dump(pre + ".cloud.p.f32", c.points); dump(pre + ".cloud.n.f32", c.normals); dump(pre + ".cloud.c.f32", c.colors);
      std::printf("run OK: %zu -> %zu points\n", before, c.size());
      return 0;
    }
  } catch (const std::exception& e) {
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
  std::printf("usage: test_grid_downsample --expect-no-device | run <in.ply> <prefix> <bin> <min points> <parallel>\n");
  return 2;
}

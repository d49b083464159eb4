// tests/cpp/test_fusion.cpp -- the C++ mirror of the map fusion (cilantro_hip/fusion.hpp) on files tests/test_gpu_fusion.py writes:
//   test_fusion run <prefix> <w> <h> <frames> <conf_thresh>
// reads <prefix>.K.f32 and, per frame i, <prefix>.f<i>.{xyz,nrm,rgb,pose}.f32; fuses the frames in order, prints one line of counts per
// frame, writes the model as <prefix>.fused.{points,normals,colors,confidence}.f32, runs removeUnstable and writes <prefix>.clean.*.
#include <cilantro_hip/fusion.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

using namespace cilantro_hip;

static std::vector<float> read_f32(const std::string& path) {
  std::ifstream f(path, std::ios::binary | std::ios::ate);
  if (!f) throw std::runtime_error("cannot open " + path);
  const std::streamoff bytes = f.tellg();
  std::vector<float> v((size_t)bytes / sizeof(float));
  f.seekg(0);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
  return v;
}
static void write_f32(const std::string& path, const std::vector<float>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(float)));
  if (!f) throw std::runtime_error("cannot write " + path);
}
static void write_model(const std::string& pre, const SurfelMap3f& s) {
  write_f32(pre + ".points.f32", s.model.points);
  write_f32(pre + ".normals.f32", s.model.normals);
  write_f32(pre + ".colors.f32", s.model.colors);
  write_f32(pre + ".confidence.f32", s.confidence);
}

int main(int argc, char** argv) {
  if (argc < 7 || std::strcmp(argv[1], "run") != 0) {
    std::fprintf(stderr, "usage: test_fusion run <prefix> <w> <h> <frames> <conf_thresh>\n");
    return 2;
  }
  try {
    const std::string pre = argv[2];
    const size_t w = (size_t)std::atol(argv[3]), h = (size_t)std::atol(argv[4]);
    const int frames = std::atoi(argv[5]);
    const float thresh = std::strtof(argv[6], nullptr);
    const std::vector<float> K = read_f32(pre + ".K.f32");
    if (K.size() != 9) throw std::runtime_error("K must hold 9 floats");
    SurfelMap3f surfels;
    if (surfels.size() != 0 || !surfels.model.isEmpty()) throw std::runtime_error("a new map is not empty");
    for (int i = 0; i < frames; ++i) {
      const std::string fp = pre + ".f" + std::to_string(i);
      PointCloud3f frame;
      frame.points = read_f32(fp + ".xyz.f32");
      frame.normals = read_f32(fp + ".nrm.f32");
      frame.colors = read_f32(fp + ".rgb.f32");
      const std::vector<float> pose = read_f32(fp + ".pose.f32");
      if (pose.size() != 16) throw std::runtime_error("a pose must hold 16 floats");
      RigidTransform3f cam_pose;
      std::memcpy(cam_pose.data(), pose.data(), sizeof(float) * 16);
      const size_t before = surfels.size();
      surfels.fuse(frame, cam_pose, K.data(), w, h);
      const cilhip_fusion_counts& c = surfels.lastCounts();
      std::printf("frame %d: visited %zu fused %zu appended %zu removed %zu untouched %zu\n", i, c.visited, c.fused, c.appended, c.removed, c.untouched);
      if (surfels.size() != before - c.removed + c.appended || c.visited != c.fused + c.appended + c.removed + c.untouched) throw std::runtime_error("the counts do not add up");
      if (surfels.model.points.size() != 3 * surfels.size() || surfels.model.colors.size() != 3 * surfels.size()) throw std::runtime_error("the model's arrays differ in size");
    }
    write_model(pre + ".fused", surfels);
    surfels.removeUnstable(thresh);
    write_model(pre + ".clean", surfels);
    SurfelMap3f copy = surfels;
    if (copy.clear().size() != 0 || !copy.model.isEmpty()) throw std::runtime_error("clear() left rows");
    std::printf("run OK\n");
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}

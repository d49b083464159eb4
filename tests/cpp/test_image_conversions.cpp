// tests/cpp/test_image_conversions.cpp -- the C++ mirror of the image conversions (include/cilantro_hip/image_point_cloud_conversions.hpp
// and PointCloud3f::fromDepthImage / fromRGBDImages), driven by tests/test_image_conversions_cpp_cpu.py (build; the host half) and
// tests/test_gpu_image_conversions.py (the results, against the Python mirror's):
//   test_image_conversions host
//   test_image_conversions run <depth.u16> <rgb.u8> <w> <h> <K.f32: 9 floats, column-major> <E.f32: 16 floats, column-major> <scale> <out prefix>
//       writes <prefix>.points.f32 / .normals.f32 / .colors.f32 (PointCloud3f::fromRGBDImages with normals), <prefix>.world.f32 /
//       .world_normals.f32 (depthImageToPointsNormals with the extrinsics, keep_invalid), <prefix>.depth.u16 / .rgb.u8 (the cloud rendered
//       back) and <prefix>.index.u64 (pointsToIndexMap of the world cloud under the extrinsics)
#include <cilantro_hip/point_cloud.hpp>

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
template <typename T>
static std::vector<T> slurp(const std::string& path) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) throw std::runtime_error("cannot read " + path);
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  std::vector<T> v((size_t)bytes / sizeof(T));
  if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fclose(f); throw std::runtime_error("short read " + path); }
  std::fclose(f);
  return v;
}

int main(int argc, char** argv) {
  try {
    const float K[9] = {525.0f, 0.0f, 0.0f, 0.0f, 525.0f, 0.0f, 319.5f, 239.5f, 1.0f};
    if (argc >= 2 && !std::strcmp(argv[1], "host")) {
      // what needs no device: the converters' descriptions, an image without pixels, a refused call
      const cilhip_depth_converter a = DepthValueConverter<unsigned short, float>(1000.0f).abi(), b = TruncatedDepthValueConverter<float, float>(2.0f, 3.5f).abi();
      if (a.raw_type != CILHIP_DEPTH_U16 || a.scale != 1000.0f || a.truncated != 0 || b.raw_type != CILHIP_DEPTH_F32 || b.truncated != 1 || b.max_depth != 3.5f) return 1;
      if (DepthValueConverter<unsigned short, float>(4.0f).inverseScale != 0.25f) return 1;
      const unsigned short none = 0;
      PointCloud3f cloud;
      cloud.points.assign(6, 1.0f);
      cloud.fromDepthImage(&none, DepthValueConverter<unsigned short, float>(1000.0f), 0, 7, K, false, true);
      if (!cloud.isEmpty() || cloud.hasNormals()) return 1;
      std::vector<size_t> map(1, 7);
      pointsToIndexMap<size_t>(ConstPointsView(cloud.points), K, map.data(), 0, 0);
      if (map[0] != 7) return 1;
      bool threw = false;
      try {
        cloud.fromDepthImage(&none, DepthValueConverter<unsigned short, float>(0.0f), 1, 1, K);      // scale 0
      } catch (const std::runtime_error& e) {
        threw = std::strstr(e.what(), "scale") != nullptr;
      }
      if (!threw) return 1;
      std::printf("host OK\n");
      return 0;
    }
    if (argc >= 10 && !std::strcmp(argv[1], "run")) {
      const std::vector<unsigned short> depth = slurp<unsigned short>(argv[2]);
      const std::vector<unsigned char> rgb = slurp<unsigned char>(argv[3]);
      const size_t w = (size_t)std::atoll(argv[4]), h = (size_t)std::atoll(argv[5]);
      const std::vector<float> Kf = slurp<float>(argv[6]), Ef = slurp<float>(argv[7]);
      const DepthValueConverter<unsigned short, float> conv((float)std::atof(argv[8]));
      const std::string pre = argv[9];
      if (depth.size() != w * h || rgb.size() != 3 * w * h || Kf.size() != 9 || Ef.size() != 16) throw std::runtime_error("bad input sizes");
      RigidTransform3f E;
      std::memcpy(E.data(), Ef.data(), sizeof(float) * 16);
      PointCloud3f cloud;
      cloud.fromRGBDImages(rgb.data(), depth.data(), conv, w, h, Kf.data(), false, true);
      dump(pre + ".points.f32", cloud.points);
      dump(pre + ".normals.f32", cloud.normals);
      dump(pre + ".colors.f32", cloud.colors);
      std::vector<float> world, world_normals;
      depthImageToPointsNormals(depth.data(), conv, w, h, Kf.data(), E, world, world_normals, true);
      dump(pre + ".world.f32", world);
      dump(pre + ".world_normals.f32", world_normals);
      std::vector<unsigned short> back(w * h);
      std::vector<unsigned char> back_rgb(3 * w * h);
      pointsColorsToRGBDImages(ConstPointsView(cloud.points), ConstPointsView(cloud.colors), Kf.data(), conv, back_rgb.data(), back.data(), w, h);
      dump(pre + ".depth.u16", back);
      dump(pre + ".rgb.u8", back_rgb);
      std::vector<size_t> index(w * h);
      pointsToIndexMap<size_t>(ConstPointsView(world), E, Kf.data(), index.data(), w, h);
      dump(pre + ".index.u64", std::vector<uint64_t>(index.begin(), index.end()));
      std::printf("run OK: %zu rows\n", cloud.size());
      return 0;
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 2;
  }
  std::fprintf(stderr, "usage: test_image_conversions host | run <depth.u16> <rgb.u8> <w> <h> <K.f32> <E.f32> <scale> <prefix>\n");
  return 64;
}

// examples/depth_image_conversions.cpp -- the sensor-facing half of cilantro's examples/fusion.cpp without a camera: a PLY cloud is
// rendered to a 640 x 480 millimetre depth image (pointsToDepthImage), read back as an organised cloud with normals
// (PointCloud3f::fromDepthImage(..., compute_normals)) and indexed per pixel (pointsToIndexMap), all on the device.
//
//   g++ -O2 -std=c++17 -Iinclude examples/depth_image_conversions.cpp -o depth_image_conversions -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./depth_image_conversions cloud.ply [out.ply]
//
// The cloud is taken to be in the camera frame (z forward), as a frame unprojected from a depth sensor is; K is the one of fusion.cpp.
#include <cilantro_hip/point_cloud.hpp>

#include <cstdio>
#include <limits>
#include <vector>

using namespace cilantro_hip;

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("Please provide path to PLY file.\n");
    return 0;
  }
  try {
    const PointCloud3f cloud(argv[1]);
    const size_t w = 640, h = 480;
    const float K[9] = {525.0f, 0.0f, 0.0f, 0.0f, 525.0f, 0.0f, 319.5f, 239.5f, 1.0f};      // column-major
    const TruncatedDepthValueConverter<unsigned short, float> dc(1000.0f, 4.0f);           // millimetres, cut at 4 m

    std::vector<unsigned short> depth(w * h);
    pointsToDepthImage(ConstPointsView(cloud.points), K, dc, depth.data(), w, h);
    size_t lit = 0;
    for (unsigned short d : depth) lit += d > 0;
    std::printf("Points: %zu, depth pixels set: %zu of %zu\n", cloud.size(), lit, w * h);

    PointCloud3f frame;
    frame.fromDepthImage(depth.data(), dc, w, h, K, false, true);
    std::printf("Points with normals read back from the image: %zu\n", frame.size());

    std::vector<size_t> index(w * h);
    pointsToIndexMap<size_t>(ConstPointsView(frame.points), K, index.data(), w, h);
    size_t named = 0;
    for (size_t i : index) named += i != std::numeric_limits<size_t>::max();
    std::printf("Pixels of the index map that name a point: %zu\n", named);
    if (argc >= 3) frame.toPLYFile(argv[2]);
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}

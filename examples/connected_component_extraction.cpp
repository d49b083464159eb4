// examples/connected_component_extraction.cpp -- the flow of cilantro's examples/connected_component_extraction.cpp on the GPU
// engine: read a PLY with normals, downsample it, drop invalid rows, segment it into smooth patches (points within 2 cm whose
// normals differ by at most 2 degrees are joined), print the segments.
//
//   g++ -O2 -std=c++17 -Iinclude examples/connected_component_extraction.cpp -o connected_component_extraction -Lcilantro_amd/lib \
//       -lcilantro_hip -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib
//   ./connected_component_extraction cloud.ply [segmented.ply]
//
// Differs from the reference example only where the missing pieces force it: no visualizer -- the segment count and sizes are
// printed, and the cloud coloured by segment is written to the second argument when there is one.
#include <cilantro_hip/clustering.hpp>
#include <cilantro_hip/point_cloud.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>

using namespace cilantro_hip;

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("Please provide path to PLY file.\n"); return 0; }
  PointCloud3f cloud(argv[1]);
  cloud.gridDownsample(0.005f).removeInvalidData();
  if (!cloud.hasNormals()) { std::printf("Input cloud does not have normals!\n"); return 0; }

  const auto t0 = std::chrono::steady_clock::now();
  const RadiusNeighborhoodSpecification<float> nh(0.02f * 0.02f);
  const NormalsProximityEvaluator ev(ConstPointsView(cloud.normals), (float)(2.0 * M_PI / 180.0));
  ConnectedComponentExtraction3f<> cce{ConstPointsView(cloud.points)};
  cce.segment(nh, ev, 100, cloud.size());
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Segmentation time: %.2fms (upload + index + segmentation)\n", ms);
  std::printf("%zu components found\n", cce.getNumberOfClusters());
  for (size_t k = 0; k < cce.getNumberOfClusters(); ++k) std::printf("  segment %zu: %zu points\n", k, cce.getClusterToPointIndicesMap()[k].size());
  std::printf("%zu of %zu points are in no segment\n", cce.getUnlabeledPointIndices().size(), cce.getNumberOfPoints());

  if (argc >= 3) {      // one colour per segment, black for the points without one
    PointCloud3f seg = cloud;
    seg.colors.assign(seg.points.size(), 0.0f);
    const auto& labels = cce.getPointToClusterIndexMap();
    for (size_t i = 0; i < labels.size(); ++i) {
      if (labels[i] >= cce.getNumberOfClusters()) continue;
      unsigned h = (unsigned)(labels[i] + 1) * 2654435761u;
      for (int k = 0; k < 3; ++k) { seg.colors[3 * i + k] = 0.25f + 0.75f * (float)((h >> (8 * k)) & 255u) / 255.0f; }
    }
    seg.toPLYFile(argv[2]);
  }
  return 0;
}

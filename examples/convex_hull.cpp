// examples/convex_hull.cpp -- cilantro's examples/convex_hull.cpp on the GPU engine.  Without an argument: the hull of the unit cube's
// corners and its centre, vertices, faces and both neighbour tables printed (the cube's faces come out as 6 quads).  With a PLY file:
// ConvexHull3f(cloud.points, true, true), the hull cloud taken from getVertexPointIndices(), and the counts, area, volume and device
// rounds printed where the reference opens its viewer.
//
//   g++ -O2 -std=c++17 -Iinclude examples/convex_hull.cpp -o convex_hull -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./convex_hull [cloud.ply]
#include <cilantro_hip/point_cloud.hpp>
#include <cilantro_hip/spatial.hpp>

#include <cstdio>
#include <vector>

static void print_lists(const char* title, const std::vector<std::vector<size_t>>& lists, const char* row) {
  std::printf("%s\n", title);
  for (size_t i = 0; i < lists.size(); ++i) {
    std::printf("%s %zu:", row, i);
    for (const size_t v : lists[i]) std::printf(" %zu", v);
    std::printf("\n");
  }
}

static void run_demo() {
  const std::vector<float> points = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0.5f, 0.5f, 0.5f};

  cilantro_hip::ConvexHull3f ch(points, true);

  const std::vector<float>& v = ch.getVertices();
  std::printf("Vertices: %zu\n", v.size() / 3);
  for (size_t i = 0; i < v.size() / 3; ++i) std::printf("%g %g %g\n", v[3 * i], v[3 * i + 1], v[3 * i + 2]);
  print_lists("Faces:", ch.getFacetVertexIndices(), "Face");
  print_lists("Vertex neighbor faces:", ch.getVertexNeighborFacets(), "Vertex");
  print_lists("Face neighbor faces:", ch.getFacetNeighborFacets(), "Neighbors of face");
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("No input PLY file path provided, running simple demo.\n");
    run_demo();
    return 0;
  }

  cilantro_hip::PointCloud3f cloud(argv[1]);
  if (cloud.points.empty()) {
    std::printf("Input cloud is empty!\n");
    return 0;
  }

  cilantro_hip::ConvexHull3f ch(cloud.points, true, true);

  cilantro_hip::PointCloud3f hull_cloud;
  for (const size_t i : ch.getVertexPointIndices()) {
    hull_cloud.points.insert(hull_cloud.points.end(), cloud.points.begin() + 3 * i, cloud.points.begin() + 3 * i + 3);
    if (!cloud.normals.empty()) hull_cloud.normals.insert(hull_cloud.normals.end(), cloud.normals.begin() + 3 * i, cloud.normals.begin() + 3 * i + 3);
    if (!cloud.colors.empty()) hull_cloud.colors.insert(hull_cloud.colors.end(), cloud.colors.begin() + 3 * i, cloud.colors.begin() + 3 * i + 3);
  }

  const cilhip_hull_info& info = ch.getInfo();
  std::printf("Points: %zu (%zu not finite)\n", cloud.points.size() / 3, info.n_nonfinite);
  std::printf("Hull vertices: %zu, faces: %zu\n", hull_cloud.points.size() / 3, ch.getFacetVertexIndices().size());
  std::printf("Area: %.9g, volume: %.9g\n", ch.getArea(), ch.getVolume());
  std::printf("Device rounds: %zu, survivors of the first cull: %zu, plane tests: %llu\n", info.rounds, info.survivors_first_round, info.plane_tests);
  return 0;
}

// examples/projective_icp.cpp -- the localisation step of cilantro's examples/fusion.cpp:127-158 without a camera: a PLY cloud is
// rendered to a 640 x 480 u16 millimetre depth image, read back as the model frame with normals (PointCloud3f::fromDepthImage(...,
// compute_normals)), and a displaced copy of it is registered to the model by projective point-to-plane ICP with the example's settings
// (max_distance 0.1^2, 6 iterations, tolerance 5e-4).
//
//   g++ -O2 -std=c++17 -Iinclude examples/projective_icp.cpp -o projective_icp -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./projective_icp cloud.ply
//
// The cloud is taken to be in the camera frame (z forward); K is the one of fusion.cpp:64.
#include <cilantro_hip/point_cloud.hpp>

#include <cmath>
#include <cstdio>
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
    const DepthValueConverter<unsigned short, float> dc(1000.0f);

    std::vector<unsigned short> depth(w * h);
    pointsToDepthImage(ConstPointsView(cloud.points), K, dc, depth.data(), w, h);
    PointCloud3f model;
    model.fromDepthImage(depth.data(), dc, w, h, K, false, true);
    std::printf("Points: %zu, model points with normals: %zu\n", cloud.size(), model.size());

    // the frame to localise: the model seen from a camera moved by a few millimetres and a fraction of a degree
    const float a = 0.006f, ca = std::cos(a), sa = std::sin(a);
    std::vector<float> frame(model.points.size());
    for (size_t i = 0; i < model.size(); ++i) {
      const float x = model.points[3 * i], y = model.points[3 * i + 1], z = model.points[3 * i + 2];
      frame[3 * i] = ca * x + sa * z + 0.004f;
      frame[3 * i + 1] = y - 0.003f;
      frame[3 * i + 2] = -sa * x + ca * z + 0.002f;
    }

    SimpleCombinedMetricRigidProjectiveICP3f icp(ConstPointsView(model.points), ConstPointsView(model.normals), ConstPointsView(frame));
    icp.correspondenceSearchEngine().setProjectionIntrinsicMatrix(K).setProjectionImageWidth(w).setProjectionImageHeight(h).setMaxDistance(0.1f * 0.1f);
    icp.setMaxNumberOfIterations(6);
    icp.setConvergenceTolerance(5e-4f);
    const RigidTransform3f T = icp.estimate().getTransform();
    std::printf("Iterations performed: %zu, has converged: %d\n", icp.getNumberOfPerformedIterations(), (int)icp.hasConverged());
    std::printf("Correspondences of the last iteration: %zu\n", icp.correspondenceSearchEngine().getCorrespondences().size());
    std::printf("Estimated transform:\n");
    for (int r = 0; r < 4; ++r) std::printf("  % .6f % .6f % .6f % .6f\n", T(r, 0), T(r, 1), T(r, 2), T(r, 3));
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}

// examples/fusion.cpp -- the flow of cilantro's examples/fusion.cpp without a camera or a viewer: a PLY cloud is rendered to 640 x 480 RGB-D
// images from a few camera poses (pointsColorsToRGBDImages); every image pair is read back as a frame with normals and colours
// (PointCloud3f::fromRGBDImages(..., compute_normals), fusion.cpp:127), localised against the model by projective point-to-plane ICP with
// the example's settings (:131-141: 0.1^2, 6 iterations, 5e-4, one optimisation step) and fused into the model (SurfelMap3f::fuse,
// :147-236); at the end unstable points leave (removeUnstable(3.0f), :51-59, :259-260) and the model is written as a PLY.
//
//   g++ -O2 -std=c++17 -Iinclude examples/fusion.cpp -o fusion -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./fusion cloud.ply [model.ply]
//
// The cloud is taken to be in the first camera's frame (z forward); K is the one of fusion.cpp:64.
#include <cilantro_hip/fusion.hpp>

#include <cmath>
#include <cstdio>
#include <vector>

using namespace cilantro_hip;

// a camera that has turned by `a` radians about y and moved by (tx, 0, tz): camera to world
static RigidTransform3f camera_pose(float a, float tx, float tz) {
  RigidTransform3f E;
  E.linear(0, 0) = std::cos(a); E.linear(0, 2) = std::sin(a);
  E.linear(2, 0) = -std::sin(a); E.linear(2, 2) = std::cos(a);
  E.translation(0) = tx; E.translation(2) = tz;
  return E;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("Please provide path to PLY file.\n");
    return 0;
  }
  try {
    PointCloud3f cloud(argv[1]);
    if (!cloud.hasColors()) cloud.colors.assign(cloud.points.size(), 0.8f);
    const size_t w = 640, h = 480;
    const float K[9] = {525.0f, 0.0f, 0.0f, 0.0f, 525.0f, 0.0f, 319.5f, 239.5f, 1.0f};      // column-major
    const TruncatedDepthValueConverter<unsigned short, float> dc(1000.0f, 4.0f);           // millimetres, cut at 4 m (the example: 1.8 m)
    const float confidence_thresh = 3.0f;                                                  // fusion.cpp:101

    SurfelMap3f surfels;
    RigidTransform3f cam_pose;
    std::vector<unsigned short> depth(w * h);
    std::vector<unsigned char> rgb(3 * w * h);
    const int views = 12;
    for (int v = 0; v < views; ++v) {
      // the sensor: the cloud seen from a camera that drifts sideways and turns a little with every view
      const RigidTransform3f seen_from = camera_pose(0.004f * v, 0.003f * v, -0.002f * v);
      pointsColorsToRGBDImages(ConstPointsView(cloud.points), ConstPointsView(cloud.colors), seen_from, K, dc, rgb.data(), depth.data(), w, h);
      PointCloud3f frame;
      frame.fromRGBDImages(rgb.data(), depth.data(), dc, w, h, K, false, true);

      // Localize
      size_t iterations = 0;
      if (!surfels.model.isEmpty()) {
        SimpleCombinedMetricRigidProjectiveICP3f icp(ConstPointsView(surfels.model.points), ConstPointsView(surfels.model.normals), ConstPointsView(frame.points));
        icp.correspondenceSearchEngine().setProjectionExtrinsicMatrix(cam_pose).setProjectionImageWidth(w).setProjectionImageHeight(h).setProjectionIntrinsicMatrix(K);
        icp.correspondenceSearchEngine().setMaxDistance(0.1f * 0.1f);
        icp.setInitialTransform(cam_pose);
        icp.setConvergenceTolerance(5e-4f);
        icp.setMaxNumberOfIterations(6);
        icp.setMaxNumberOfOptimizationStepIterations(1);
        cam_pose = icp.estimate().getTransform();
        iterations = icp.getNumberOfPerformedIterations();
      } else {
        cam_pose.setIdentity();
      }

      // Map
      surfels.fuse(frame, cam_pose, K, w, h);
      const cilhip_fusion_counts& c = surfels.lastCounts();
      std::printf("view %d: frame points %zu, ICP iterations %zu, pose t = (% .4f % .4f % .4f) | visited %zu fused %zu appended %zu removed %zu untouched %zu | model %zu\n", v,
                  frame.size(), iterations, cam_pose.translation(0), cam_pose.translation(1), cam_pose.translation(2), c.visited, c.fused, c.appended, c.removed, c.untouched,
                  surfels.size());
    }
    std::printf("Fused %d frames\n", views);
    std::printf("Removing unstable points\n");
    surfels.removeUnstable(confidence_thresh);
    std::printf("Model points: %zu\n", surfels.size());
    if (argc >= 3) {
      std::printf("Saving model to '%s'\n", argv[2]);
      surfels.model.toPLYFile(argv[2], true);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 1;
  }
  return 0;
}

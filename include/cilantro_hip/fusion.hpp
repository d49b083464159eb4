// cilantro_hip/fusion.hpp -- the model of cilantro's examples/fusion.cpp and its "Map" step (:147-236), header-only on top of the C ABI
// (c_api.h: cilhip_fuse_frame3f, cilhip_fusion_remove_unstable3f, which state the arithmetic; DESIGN.md section 16 has the rules F1-F9):
//
//   SurfelMap3f::model, ::confidence      the example's `PointCloud3f model` and `std::vector<float> confidence`   :89-90
//   SurfelMap3f::fuse                     one registered frame into the model                                       :147-236
//   SurfelMap3f::removeUnstable           cleanup_callback                                                          :51-59
//   SurfelMap3f::clear                    clear_callback                                                            :46-49
//
// The frame is a PointCloud3f with normals and colours in the camera frame (fromRGBDImages(..., compute_normals)), cam_pose the camera's
// pose (camera to world), intrinsics 9 floats column-major.  Capacity is handled inside.  No CPU fallback: a failing C-ABI call throws.
#pragma once

#include <algorithm>
#include <stdexcept>
#include <string>
#include <vector>

#include "abi.hpp"
#include "c_api.h"
#include "icp.hpp"
#include "point_cloud.hpp"

namespace cilantro_hip {

class SurfelMap3f {
public:
  PointCloud3f model;
  std::vector<float> confidence;
  cilhip_fusion_params params;

  explicit SurfelMap3f(int device = 0) : device_(device), last_{0, 0, 0, 0, 0} { cilhip_fusion_default_params(&params); }

  size_t size() const { return confidence.size(); }

  SurfelMap3f& fuse(const PointCloud3f& frame, const RigidTransform3f& cam_pose, const float* intrinsics, size_t image_w, size_t image_h) {
    const size_t nf = frame.size();
    if (nf && (!frame.hasNormals() || !frame.hasColors())) throw std::invalid_argument("SurfelMap3f::fuse: the frame needs normals and colors");
    const size_t n = size();
    if (model.points.size() != 3 * n || model.normals.size() != 3 * n || model.colors.size() != 3 * n)
      throw std::invalid_argument("SurfelMap3f::fuse: model.points, normals, colors and confidence differ in size");
    const size_t capacity = n + std::min(nf, image_w * image_h);
    resize(capacity);
    size_t n_out = n;
    const int rc = cilhip_fuse_frame3f(device_, model.points.data(), model.normals.data(), model.colors.data(), confidence.data(), n, capacity, frame.points.data(),
                                       frame.normals.data(), frame.colors.data(), nf, CILHIP_MEM_HOST, cam_pose.data(), intrinsics, image_w, image_h, &params, &n_out, &last_);
    resize(rc == CILHIP_OK ? n_out : n);
    detail::check(rc, "cilhip_fuse_frame3f");
    return *this;
  }

  SurfelMap3f& removeUnstable(float conf_thresh) {
    size_t n_out = size();
    detail::check(cilhip_fusion_remove_unstable3f(device_, model.points.data(), model.normals.data(), model.colors.data(), confidence.data(), size(), CILHIP_MEM_HOST, conf_thresh, &n_out),
                  "cilhip_fusion_remove_unstable3f");
    resize(n_out);
    return *this;
  }

  SurfelMap3f& clear() {
    resize(0);
    return *this;
  }

  // the populations of the last fuse(): visited = fused + appended + removed + untouched
  const cilhip_fusion_counts& lastCounts() const { return last_; }

private:
  void resize(size_t rows) {
    model.points.resize(3 * rows);
    model.normals.resize(3 * rows);
    model.colors.resize(3 * rows);
    confidence.resize(rows);
  }
  int device_;
  cilhip_fusion_counts last_;
};

}  // namespace cilantro_hip

// cilantro_hip/image_point_cloud_conversions.hpp -- C++ host-side mirrors of cilantro's core/image_point_cloud_conversions.hpp,
// header-only on top of the C ABI (c_api.h: cilhip_depth_image_to_points3f, cilhip_points_to_depth_image3f,
// cilhip_points_to_index_map3f, which state the arithmetic; DESIGN.md section 14 has the rules):
//
//   DepthValueConverter<RawT, float>, TruncatedDepthValueConverter<RawT, float>     :7-51   (RawT: unsigned short or float)
//   depthImageToPoints, depthImageToPointsNormals                                   :53-349
//   RGBDImagesToPointsColors, RGBDImagesToPointsNormalsColors                       :351-695
//   pointsToDepthImage, pointsColorsToRGBDImages                                    :697-863
//   pointsToIndexMap                                                                :865-934
//
// Same names, argument order and defaults as the reference.  Intrinsics are 9 floats, column-major (Eigen::Matrix3f::data()),
// extrinsics a RigidTransform3f; clouds go in as non-owning (pointer, count) views and come out as packed xyz / rgb
// std::vector<float>.  The index map is size_t with std::numeric_limits<size_t>::max() for an empty pixel, as the reference's default.
// No CPU fallback: a failing C-ABI call throws.
#pragma once

#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "abi.hpp"
#include "c_api.h"
#include "icp.hpp"

namespace cilantro_hip {

template <typename RawDepthT, typename MetricDepthT = float>
struct DepthValueConverter {
  static_assert(std::is_same<MetricDepthT, float>::value && (std::is_same<RawDepthT, unsigned short>::value || std::is_same<RawDepthT, float>::value),
                "built for float metric depth over unsigned short or float raw depth");
  using RawDepth = RawDepthT;
  using MetricDepth = MetricDepthT;
  DepthValueConverter() : scale(1.0f), inverseScale(1.0f) {}
  DepthValueConverter(MetricDepthT mult) : scale(mult), inverseScale(1.0f / mult) {}
  cilhip_depth_converter abi() const { return cilhip_depth_converter{std::is_same<RawDepthT, float>::value ? CILHIP_DEPTH_F32 : CILHIP_DEPTH_U16, scale, 0, std::numeric_limits<float>::max()}; }
  const MetricDepthT scale;
  const MetricDepthT inverseScale;
};

template <typename RawDepthT, typename MetricDepthT = float>
struct TruncatedDepthValueConverter {
  static_assert(std::is_same<MetricDepthT, float>::value && (std::is_same<RawDepthT, unsigned short>::value || std::is_same<RawDepthT, float>::value),
                "built for float metric depth over unsigned short or float raw depth");
  using RawDepth = RawDepthT;
  using MetricDepth = MetricDepthT;
  TruncatedDepthValueConverter() : scale(1.0f), inverseScale(1.0f), maxDepth(std::numeric_limits<float>::max()) {}
  TruncatedDepthValueConverter(MetricDepthT mult, MetricDepthT thresh) : scale(mult), inverseScale(1.0f / mult), maxDepth(thresh) {}
  cilhip_depth_converter abi() const { return cilhip_depth_converter{std::is_same<RawDepthT, float>::value ? CILHIP_DEPTH_F32 : CILHIP_DEPTH_U16, scale, 1, maxDepth}; }
  const MetricDepthT scale;
  const MetricDepthT inverseScale;
  const MetricDepthT maxDepth;
};

namespace detail {

// the one call behind the eight image -> cloud overloads
inline void image_to_cloud(const void* depth, const unsigned char* rgb, const cilhip_depth_converter& conv, size_t w, size_t h, const float* intrinsics,
                           const RigidTransform3f* extrinsics, std::vector<float>& points, std::vector<float>* normals, std::vector<float>* colors, bool keep_invalid,
                           int device) {
  const size_t n = w * h;
  size_t rows = 0;
  points.resize(room(3 * n));
  if (normals) normals->resize(room(3 * n));
  if (colors) colors->resize(room(3 * n));
  check(cilhip_depth_image_to_points3f(device, depth, rgb, w, h, CILHIP_MEM_HOST, &conv, intrinsics, extrinsics ? extrinsics->data() : nullptr, keep_invalid ? 1 : 0,
                                                   normals ? 1 : 0, points.data(), normals ? normals->data() : nullptr, colors ? colors->data() : nullptr, n, &rows),
                    "cilhip_depth_image_to_points3f");
  points.resize(3 * rows);
  if (normals) normals->resize(3 * rows);
  if (colors) colors->resize(3 * rows);
}

}  // namespace detail

template <class DepthConverterT>
void depthImageToPoints(const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w, size_t image_h, const float* intrinsics,
                        std::vector<float>& points, bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, nullptr, depth_converter.abi(), image_w, image_h, intrinsics, nullptr, points, nullptr, nullptr, keep_invalid, device);
}
template <class DepthConverterT>
void depthImageToPoints(const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w, size_t image_h, const float* intrinsics,
                        const RigidTransform3f& extrinsics, std::vector<float>& points, bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, nullptr, depth_converter.abi(), image_w, image_h, intrinsics, &extrinsics, points, nullptr, nullptr, keep_invalid, device);
}
template <class DepthConverterT>
void depthImageToPointsNormals(const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w, size_t image_h,
                               const float* intrinsics, std::vector<float>& points, std::vector<float>& normals, bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, nullptr, depth_converter.abi(), image_w, image_h, intrinsics, nullptr, points, &normals, nullptr, keep_invalid, device);
}
template <class DepthConverterT>
void depthImageToPointsNormals(const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w, size_t image_h,
                               const float* intrinsics, const RigidTransform3f& extrinsics, std::vector<float>& points, std::vector<float>& normals, bool keep_invalid = false,
                               int device = 0) {
  detail::image_to_cloud(depth_data, nullptr, depth_converter.abi(), image_w, image_h, intrinsics, &extrinsics, points, &normals, nullptr, keep_invalid, device);
}
template <class DepthConverterT>
void RGBDImagesToPointsColors(const unsigned char* rgb_data, const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w,
                              size_t image_h, const float* intrinsics, std::vector<float>& points, std::vector<float>& colors, bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, rgb_data, depth_converter.abi(), image_w, image_h, intrinsics, nullptr, points, nullptr, &colors, keep_invalid, device);
}
template <class DepthConverterT>
void RGBDImagesToPointsColors(const unsigned char* rgb_data, const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w,
                              size_t image_h, const float* intrinsics, const RigidTransform3f& extrinsics, std::vector<float>& points, std::vector<float>& colors,
                              bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, rgb_data, depth_converter.abi(), image_w, image_h, intrinsics, &extrinsics, points, nullptr, &colors, keep_invalid, device);
}
template <class DepthConverterT>
void RGBDImagesToPointsNormalsColors(const unsigned char* rgb_data, const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w,
                                     size_t image_h, const float* intrinsics, std::vector<float>& points, std::vector<float>& normals, std::vector<float>& colors,
                                     bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, rgb_data, depth_converter.abi(), image_w, image_h, intrinsics, nullptr, points, &normals, &colors, keep_invalid, device);
}
template <class DepthConverterT>
void RGBDImagesToPointsNormalsColors(const unsigned char* rgb_data, const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w,
                                     size_t image_h, const float* intrinsics, const RigidTransform3f& extrinsics, std::vector<float>& points, std::vector<float>& normals,
                                     std::vector<float>& colors, bool keep_invalid = false, int device = 0) {
  detail::image_to_cloud(depth_data, rgb_data, depth_converter.abi(), image_w, image_h, intrinsics, &extrinsics, points, &normals, &colors, keep_invalid, device);
}

template <class DepthConverterT>
void pointsToDepthImage(const ConstPointsView& points, const float* intrinsics, const DepthConverterT& depth_converter, typename DepthConverterT::RawDepth* depth_data,
                        size_t image_w, size_t image_h, int device = 0) {
  const cilhip_depth_converter c = depth_converter.abi();
  detail::check(cilhip_points_to_depth_image3f(device, points.data(), nullptr, points.cols(), CILHIP_MEM_HOST, nullptr, intrinsics, &c, image_w, image_h, depth_data, nullptr),
                            "cilhip_points_to_depth_image3f");
}
template <class DepthConverterT>
void pointsToDepthImage(const ConstPointsView& points, const RigidTransform3f& extrinsics, const float* intrinsics, const DepthConverterT& depth_converter,
                        typename DepthConverterT::RawDepth* depth_data, size_t image_w, size_t image_h, int device = 0) {
  const cilhip_depth_converter c = depth_converter.abi();
  detail::check(cilhip_points_to_depth_image3f(device, points.data(), nullptr, points.cols(), CILHIP_MEM_HOST, extrinsics.data(), intrinsics, &c, image_w, image_h,
                                                           depth_data, nullptr),
                            "cilhip_points_to_depth_image3f");
}
template <class DepthConverterT>
void pointsColorsToRGBDImages(const ConstPointsView& points, const ConstPointsView& colors, const float* intrinsics, const DepthConverterT& depth_converter,
                              unsigned char* rgb_data, typename DepthConverterT::RawDepth* depth_data, size_t image_w, size_t image_h, int device = 0) {
  if (colors.cols() != points.cols()) throw std::invalid_argument("pointsColorsToRGBDImages: colors and points differ in size");
  const cilhip_depth_converter c = depth_converter.abi();
  detail::check(cilhip_points_to_depth_image3f(device, points.data(), colors.data(), points.cols(), CILHIP_MEM_HOST, nullptr, intrinsics, &c, image_w, image_h,
                                                           depth_data, rgb_data),
                            "cilhip_points_to_depth_image3f");
}
template <class DepthConverterT>
void pointsColorsToRGBDImages(const ConstPointsView& points, const ConstPointsView& colors, const RigidTransform3f& extrinsics, const float* intrinsics,
                              const DepthConverterT& depth_converter, unsigned char* rgb_data, typename DepthConverterT::RawDepth* depth_data, size_t image_w, size_t image_h,
                              int device = 0) {
  if (colors.cols() != points.cols()) throw std::invalid_argument("pointsColorsToRGBDImages: colors and points differ in size");
  const cilhip_depth_converter c = depth_converter.abi();
  detail::check(cilhip_points_to_depth_image3f(device, points.data(), colors.data(), points.cols(), CILHIP_MEM_HOST, extrinsics.data(), intrinsics, &c, image_w,
                                                           image_h, depth_data, rgb_data),
                            "cilhip_points_to_depth_image3f");
}

namespace detail {
template <typename IndexT>
void index_map(const ConstPointsView& points, const RigidTransform3f* extrinsics, const float* intrinsics, IndexT* index_map_data, size_t image_w, size_t image_h, int device) {
  std::vector<uint32_t> raw(room(image_w * image_h));
  check(cilhip_points_to_index_map3f(device, points.data(), points.cols(), CILHIP_MEM_HOST, extrinsics ? extrinsics->data() : nullptr, intrinsics, image_w, image_h,
                                                 raw.data()),
                    "cilhip_points_to_index_map3f");
  for (size_t k = 0; k < image_w * image_h; ++k) index_map_data[k] = raw[k] == 0xFFFFFFFFu ? std::numeric_limits<IndexT>::max() : (IndexT)raw[k];
}
}  // namespace detail

template <typename IndexT = size_t>
void pointsToIndexMap(const ConstPointsView& points, const float* intrinsics, IndexT* index_map_data, size_t image_w, size_t image_h, int device = 0) {
  detail::index_map(points, nullptr, intrinsics, index_map_data, image_w, image_h, device);
}
template <typename IndexT = size_t>
void pointsToIndexMap(const ConstPointsView& points, const RigidTransform3f& extrinsics, const float* intrinsics, IndexT* index_map_data, size_t image_w, size_t image_h,
                      int device = 0) {
  detail::index_map(points, &extrinsics, intrinsics, index_map_data, image_w, image_h, device);
}

}  // namespace cilantro_hip

// cilantro_hip/grid_downsampler.hpp -- C++ host-side mirrors of cilantro's voxel-grid downsamplers, header-only on top of the
// C ABI (c_api.h: cilhip_grid_downsample3f, which states the arithmetic):
//
//   PointsGridDownsampler3f               core/grid_downsampler.hpp:8-44
//   PointsNormalsGridDownsampler3f        :46-132
//   PointsColorsGridDownsampler3f         :134-220
//   PointsNormalsColorsGridDownsampler3f  :222-340
//
// Same constructor arguments, getter names and defaults as the reference.  Clouds go in as non-owning (pointer, count) views and
// come out as packed xyz / rgb std::vector<float>.  `parallel` keeps the one meaning that is reproducible: true = bins in
// lexicographic cell order, false = bins in order of first appearance; the sums are the same either way.  The device pass runs
// once, in the constructor (as the reference builds its bins there); every getter is served from it, min_points_in_bin included.
// No CPU fallback: a failing C-ABI call throws.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "abi.hpp"
#include "c_api.h"
#include "icp.hpp"

namespace cilantro_hip {

namespace detail {

// the one implementation behind the four names
class GridDownsamplerBase {
public:
  size_t getNumberOfOccupiedBins() const { return counts_.size(); }
  const std::vector<uint32_t>& getBinPointCounts() const { return counts_; }

protected:
  GridDownsamplerBase(const ConstPointsView& points, const float* normals, const float* colors, float bin_size, bool parallel, int device) {
    const size_t n = points.cols();
    size_t rows = 0;
    points_.resize(room(3 * n));
    if (normals) normals_.resize(room(3 * n));
    if (colors) colors_.resize(room(3 * n));
    counts_.resize(room(n));
    check(cilhip_grid_downsample3f(device, points.data(), normals, colors, n, CILHIP_MEM_HOST, bin_size, 1, parallel ? 1 : 0, points_.data(), normals ? normals_.data() : nullptr,
                                   colors ? colors_.data() : nullptr, counts_.data(), n, &rows),
          "cilhip_grid_downsample3f");
    points_.resize(3 * rows);
    if (normals) normals_.resize(3 * rows);
    if (colors) colors_.resize(3 * rows);
    counts_.resize(rows);
  }

  // grid_downsampler.hpp:26-33: bins with fewer members are left out, the others keep their order
  void select(const std::vector<float>& rows, std::vector<float>& out, size_t min_points_in_bin) const {
    out.clear();
    out.reserve(rows.size());
    for (size_t k = 0; k < counts_.size(); ++k)
      if (counts_[k] >= min_points_in_bin) out.insert(out.end(), rows.begin() + 3 * k, rows.begin() + 3 * k + 3);
  }

  std::vector<float> points_, normals_, colors_;
  std::vector<uint32_t> counts_;
};

}  // namespace detail

class PointsGridDownsampler3f : public detail::GridDownsamplerBase {
public:
  PointsGridDownsampler3f(const ConstPointsView& points, float bin_size, bool parallel = true, int device = 0)
      : GridDownsamplerBase(points, nullptr, nullptr, bin_size, parallel, device) {}
  const PointsGridDownsampler3f& getDownsampledPoints(std::vector<float>& ds_points, size_t min_points_in_bin = 1) const { select(points_, ds_points, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledPoints(size_t min_points_in_bin = 1) const { std::vector<float> r; select(points_, r, min_points_in_bin); return r; }
};

class PointsNormalsGridDownsampler3f : public detail::GridDownsamplerBase {
public:
  PointsNormalsGridDownsampler3f(const ConstPointsView& points, const ConstPointsView& normals, float bin_size, bool parallel = true, int device = 0)
      : GridDownsamplerBase(points, checked(points, normals, "normals"), nullptr, bin_size, parallel, device) {}
  const PointsNormalsGridDownsampler3f& getDownsampledPoints(std::vector<float>& ds_points, size_t min_points_in_bin = 1) const { select(points_, ds_points, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledPoints(size_t min_points_in_bin = 1) const { std::vector<float> r; select(points_, r, min_points_in_bin); return r; }
  const PointsNormalsGridDownsampler3f& getDownsampledNormals(std::vector<float>& ds_normals, size_t min_points_in_bin = 1) const { select(normals_, ds_normals, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledNormals(size_t min_points_in_bin = 1) const { std::vector<float> r; select(normals_, r, min_points_in_bin); return r; }
  const PointsNormalsGridDownsampler3f& getDownsampledPointsNormals(std::vector<float>& ds_points, std::vector<float>& ds_normals, size_t min_points_in_bin = 1) const {
    select(points_, ds_points, min_points_in_bin); select(normals_, ds_normals, min_points_in_bin);
    return *this;
  }
  static const float* checked(const ConstPointsView& points, const ConstPointsView& att, const char* what) {
    if (att.cols() != points.cols()) throw std::invalid_argument(std::string("grid downsampler: ") + what + " and points differ in size");
    return att.data();
  }
};

class PointsColorsGridDownsampler3f : public detail::GridDownsamplerBase {
public:
  PointsColorsGridDownsampler3f(const ConstPointsView& points, const ConstPointsView& colors, float bin_size, bool parallel = true, int device = 0)
      : GridDownsamplerBase(points, nullptr, PointsNormalsGridDownsampler3f::checked(points, colors, "colors"), bin_size, parallel, device) {}
  const PointsColorsGridDownsampler3f& getDownsampledPoints(std::vector<float>& ds_points, size_t min_points_in_bin = 1) const { select(points_, ds_points, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledPoints(size_t min_points_in_bin = 1) const { std::vector<float> r; select(points_, r, min_points_in_bin); return r; }
  const PointsColorsGridDownsampler3f& getDownsampledColors(std::vector<float>& ds_colors, size_t min_points_in_bin = 1) const { select(colors_, ds_colors, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledColors(size_t min_points_in_bin = 1) const { std::vector<float> r; select(colors_, r, min_points_in_bin); return r; }
  const PointsColorsGridDownsampler3f& getDownsampledPointsColors(std::vector<float>& ds_points, std::vector<float>& ds_colors, size_t min_points_in_bin = 1) const {
    select(points_, ds_points, min_points_in_bin); select(colors_, ds_colors, min_points_in_bin);
    return *this;
  }
};

class PointsNormalsColorsGridDownsampler3f : public detail::GridDownsamplerBase {
public:
  PointsNormalsColorsGridDownsampler3f(const ConstPointsView& points, const ConstPointsView& normals, const ConstPointsView& colors, float bin_size, bool parallel = true,
                                       int device = 0)
      : GridDownsamplerBase(points, PointsNormalsGridDownsampler3f::checked(points, normals, "normals"), PointsNormalsGridDownsampler3f::checked(points, colors, "colors"),
                            bin_size, parallel, device) {}
  const PointsNormalsColorsGridDownsampler3f& getDownsampledPoints(std::vector<float>& ds_points, size_t min_points_in_bin = 1) const { select(points_, ds_points, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledPoints(size_t min_points_in_bin = 1) const { std::vector<float> r; select(points_, r, min_points_in_bin); return r; }
  const PointsNormalsColorsGridDownsampler3f& getDownsampledNormals(std::vector<float>& ds_normals, size_t min_points_in_bin = 1) const { select(normals_, ds_normals, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledNormals(size_t min_points_in_bin = 1) const { std::vector<float> r; select(normals_, r, min_points_in_bin); return r; }
  const PointsNormalsColorsGridDownsampler3f& getDownsampledColors(std::vector<float>& ds_colors, size_t min_points_in_bin = 1) const { select(colors_, ds_colors, min_points_in_bin); return *this; }
  std::vector<float> getDownsampledColors(size_t min_points_in_bin = 1) const { std::vector<float> r; select(colors_, r, min_points_in_bin); return r; }
  const PointsNormalsColorsGridDownsampler3f& getDownsampledPointsNormalsColors(std::vector<float>& ds_points, std::vector<float>& ds_normals, std::vector<float>& ds_colors,
                                                                                size_t min_points_in_bin = 1) const {
    select(points_, ds_points, min_points_in_bin); select(normals_, ds_normals, min_points_in_bin); select(colors_, ds_colors, min_points_in_bin);
    return *this;
  }
};

}  // namespace cilantro_hip

// cilantro_hip/point_cloud.hpp -- the wire format either side of the ICP path: a
// minimal PointCloud3f with PLY ingest / output, header-only, no third-party code.  Mirrors what the reference's
// examples do before and after registration:
//   utilities/point_cloud.hpp:20-22, :501-541     PointCloud3f {points, normals, colors}, fromPLYFile / toPLYFile
//   utilities/ply_io.hpp:43-143                   PLYReader / PLYWriter (tinyply underneath in the reference)
// Same property names as the reference reads and writes: vertex x y z [nx ny nz] [red green blue]; colours are
// uchar in the file and floats in [0,1] in memory (point_cloud.hpp:513, :535).  Reads ascii and
// binary_little_endian files with any scalar property types; other elements (faces ...) are skipped.
// The clouds feed the engine as non-owning views:  ConstPointsView(cloud.points), ConstPointsView(cloud.normals).
//   utilities/point_cloud.hpp:201-245             removeInvalidPoints / Normals / Colors / Data: host compaction, in the order the reference's remove() (:154-198) leaves
//   utilities/point_cloud.hpp:247-290             gridDownsample / gridDownsampled (on the device: grid_downsampler.hpp); member
//                                                 templates as in the reference, so a program that never calls them links without the library
//   utilities/point_cloud.hpp:445-457             transformed(TransformSet): one rigid transform per point (on the device: icp.hpp transformPoints)
//   utilities/point_cloud.hpp:87-116, :463-499    the depth-image constructor, fromDepthImage / fromRGBDImages (on the device:
//                                                 image_point_cloud_conversions.hpp); intrinsics: 9 floats, column-major
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "grid_downsampler.hpp"
#include "image_point_cloud_conversions.hpp"

namespace cilantro_hip {

class PointCloud3f {
public:
  std::vector<float> points;   // packed xyz (3 x N column-major, as cilantro's VectorSet3f)
  std::vector<float> normals;  // packed xyz or empty
  std::vector<float> colors;   // packed rgb in [0,1] or empty

  PointCloud3f() = default;
  explicit PointCloud3f(const std::string& file_name) { fromPLYFile(file_name); }   // point_cloud.hpp:118-121

  template <class DepthConverterT>                                                 // point_cloud.hpp:87-98
  PointCloud3f(const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w, size_t image_h, const float* intrinsics,
               bool keep_invalid = false, bool compute_normals = false) {
    fromDepthImage(depth_data, depth_converter, image_w, image_h, intrinsics, keep_invalid, compute_normals);
  }

  // point_cloud.hpp:463-478
  template <class DepthConverterT>
  PointCloud3f& fromDepthImage(const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w, size_t image_h,
                               const float* intrinsics, bool keep_invalid = false, bool compute_normals = false) {
    colors.clear();
    normals.clear();
    if (compute_normals) depthImageToPointsNormals<DepthConverterT>(depth_data, depth_converter, image_w, image_h, intrinsics, points, normals, keep_invalid);
    else depthImageToPoints<DepthConverterT>(depth_data, depth_converter, image_w, image_h, intrinsics, points, keep_invalid);
    return *this;
  }

  // point_cloud.hpp:484-499
  template <class DepthConverterT>
  PointCloud3f& fromRGBDImages(const unsigned char* rgb_data, const typename DepthConverterT::RawDepth* depth_data, const DepthConverterT& depth_converter, size_t image_w,
                               size_t image_h, const float* intrinsics, bool keep_invalid = false, bool compute_normals = false) {
    normals.clear();
    if (compute_normals) RGBDImagesToPointsNormalsColors<DepthConverterT>(rgb_data, depth_data, depth_converter, image_w, image_h, intrinsics, points, normals, colors, keep_invalid);
    else RGBDImagesToPointsColors<DepthConverterT>(rgb_data, depth_data, depth_converter, image_w, image_h, intrinsics, points, colors, keep_invalid);
    return *this;
  }

  size_t size() const { return points.size() / 3; }
  bool isEmpty() const { return points.empty(); }
  bool hasNormals() const { return size() > 0 && normals.size() == points.size(); }   // point_cloud.hpp:139-141
  bool hasColors() const { return size() > 0 && colors.size() == points.size(); }

  // point_cloud.hpp:201-245: rows with a non-finite entry in the named attribute(s) leave the cloud, from every attribute it has
  PointCloud3f& removeInvalidPoints() { return removeRows(true, false, false); }
  PointCloud3f& removeInvalidNormals() { return hasNormals() ? removeRows(false, true, false) : *this; }
  PointCloud3f& removeInvalidColors() { return hasColors() ? removeRows(false, false, true) : *this; }
  PointCloud3f& removeInvalidData() { return removeRows(true, hasNormals(), hasColors()); }

  // point_cloud.hpp:247-266: the variant follows from the attributes the cloud has
  template <typename GridPointScalarT = std::ptrdiff_t>
  PointCloud3f& gridDownsample(float bin_size, size_t min_points_in_bin = 1, bool parallel = true) {
    PointCloud3f res = gridDownsampled<GridPointScalarT>(bin_size, min_points_in_bin, parallel);
    points.swap(res.points); normals.swap(res.normals); colors.swap(res.colors);
    return *this;
  }

  // point_cloud.hpp:445-457 with a TransformSet: one rigid transform per point, on the device (examples/non_rigid_icp.cpp:154); normals
  // turn with the linear part.  A member template like the ones above: a program that never calls it links without the library
  template <class TransformSetT = RigidTransformSet3f>
  PointCloud3f transformed(const TransformSetT& tforms, int device = 0) const {
    PointCloud3f cloud;
    cloud.points = transformPoints(tforms, ConstPointsView(points), device);
    if (hasNormals()) {
      TransformSetT linear(tforms);
      for (auto& t : linear) t.translation(0) = t.translation(1) = t.translation(2) = 0.0f;
      cloud.normals = transformPoints(linear, ConstPointsView(normals), device);
    }
    if (hasColors()) cloud.colors = colors;
    return cloud;
  }

  // point_cloud.hpp:268-290
  template <typename GridPointScalarT = std::ptrdiff_t>
  PointCloud3f gridDownsampled(float bin_size, size_t min_points_in_bin = 1, bool parallel = true) const {
    PointCloud3f res;
    const ConstPointsView p(points), n(normals), c(colors);
    if (hasNormals() && hasColors())
      PointsNormalsColorsGridDownsampler3f(p, n, c, bin_size, parallel).getDownsampledPointsNormalsColors(res.points, res.normals, res.colors, min_points_in_bin);
    else if (hasNormals())
      PointsNormalsGridDownsampler3f(p, n, bin_size, parallel).getDownsampledPointsNormals(res.points, res.normals, min_points_in_bin);
    else if (hasColors())
      PointsColorsGridDownsampler3f(p, c, bin_size, parallel).getDownsampledPointsColors(res.points, res.colors, min_points_in_bin);
    else
      PointsGridDownsampler3f(p, bin_size, parallel).getDownsampledPoints(res.points, min_points_in_bin);
    return res;
  }

  PointCloud3f& fromPLYFile(const std::string& file_name) {
    std::ifstream f(file_name, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + file_name);
    std::string line;
    if (!std::getline(f, line) || strip(line) != "ply") throw std::runtime_error(file_name + ": not a PLY file");
    enum Fmt { ASCII, BLE } fmt = ASCII;
    struct Prop { std::string name, type; bool is_list; std::string count_type; };
    struct Elem { std::string name; size_t count; std::vector<Prop> props; };
    std::vector<Elem> elems;
    for (;;) {
      if (!std::getline(f, line)) throw std::runtime_error(file_name + ": truncated PLY header");
      std::istringstream ss(strip(line));
      std::string key;
      ss >> key;
      if (key == "end_header") break;
      if (key == "format") {
        std::string v;
        ss >> v;
        if (v == "ascii") fmt = ASCII;
        else if (v == "binary_little_endian") fmt = BLE;
        else throw std::runtime_error(file_name + ": unsupported PLY format " + v);
      } else if (key == "element") {
        Elem e;
        ss >> e.name >> e.count;
        elems.push_back(e);
      } else if (key == "property") {
        if (elems.empty()) throw std::runtime_error(file_name + ": property before element");
        Prop p;
        std::string t;
        ss >> t;
        if (t == "list") { p.is_list = true; ss >> p.count_type >> p.type >> p.name; }
        else { p.is_list = false; p.type = t; ss >> p.name; }
        elems.back().props.push_back(p);
      }
    }
    points.clear(); normals.clear(); colors.clear();
    // The element counts are untrusted input: a count larger than the rest of the file can hold (every row takes at
    // least one byte per property) is a malformed file, not an allocation request.
    const std::streamoff data_begin = (std::streamoff)f.tellg();
    f.seekg(0, std::ios::end);
    const std::streamoff data_bytes = (std::streamoff)f.tellg() - data_begin;
    f.seekg(data_begin, std::ios::beg);
    if (!f || data_bytes < 0) throw std::runtime_error(file_name + ": cannot size the PLY data section");
    for (const Elem& e : elems) {
      size_t min_row = 0;
      for (const Prop& pr : e.props) min_row += fmt == ASCII ? 1 : scalar_size(pr.is_list ? pr.count_type : pr.type, file_name);
      if (min_row == 0) min_row = 1;
      if (e.count > (size_t)data_bytes / min_row) throw std::runtime_error(file_name + ": element count exceeds the file size");
    }
    for (const Elem& e : elems) {
      const bool vertex = e.name == "vertex";
      int ix[9];
      for (int& v : ix) v = -1;
      static const char* names[9] = {"x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"};
      for (size_t p = 0; p < e.props.size(); ++p)
        for (int k = 0; k < 9; ++k)
          if (!e.props[p].is_list && e.props[p].name == names[k]) ix[k] = (int)p;
      const bool has_p = vertex && ix[0] >= 0 && ix[1] >= 0 && ix[2] >= 0;
      const bool has_n = vertex && ix[3] >= 0 && ix[4] >= 0 && ix[5] >= 0;
      const bool has_c = vertex && ix[6] >= 0 && ix[7] >= 0 && ix[8] >= 0;
      if (has_p) points.resize(3 * e.count);
      if (has_n) normals.resize(3 * e.count);
      if (has_c) colors.resize(3 * e.count);
      std::vector<double> row(e.props.size());
      for (size_t i = 0; i < e.count; ++i) {
        for (size_t p = 0; p < e.props.size(); ++p) {
          const Prop& pr = e.props[p];
          if (pr.is_list) {
            const size_t cnt = (size_t)read_scalar(f, pr.count_type, fmt == ASCII, file_name);
            for (size_t k = 0; k < cnt; ++k) (void)read_scalar(f, pr.type, fmt == ASCII, file_name);
            row[p] = 0.0;
          } else {
            row[p] = read_scalar(f, pr.type, fmt == ASCII, file_name);
          }
        }
        if (has_p) for (int k = 0; k < 3; ++k) points[3 * i + k] = (float)row[ix[k]];
        if (has_n) for (int k = 0; k < 3; ++k) normals[3 * i + k] = (float)row[ix[3 + k]];
        if (has_c) for (int k = 0; k < 3; ++k) colors[3 * i + k] = (float)row[ix[6 + k]] * (1.0f / 255.0f);
      }
      if (vertex) break;   // everything the path needs has been read
    }
    return *this;
  }

  const PointCloud3f& toPLYFile(const std::string& file_name, bool binary = true) const {
    std::ofstream f(file_name, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + file_name + " for writing");
    const size_t n = size();
    f << "ply\nformat " << (binary ? "binary_little_endian" : "ascii") << " 1.0\nelement vertex " << n
      << "\nproperty float x\nproperty float y\nproperty float z\n";
    if (hasNormals()) f << "property float nx\nproperty float ny\nproperty float nz\n";
    if (hasColors()) f << "property uchar red\nproperty uchar green\nproperty uchar blue\n";
    f << "end_header\n";
    for (size_t i = 0; i < n; ++i) {
      unsigned char rgb[3] = {0, 0, 0};
      if (hasColors())
        for (int k = 0; k < 3; ++k) {
          const float v = 255.0f * colors[3 * i + k];            // point_cloud.hpp:535: cast, not rounded
          rgb[k] = (unsigned char)(v < 0.0f ? 0.0f : v > 255.0f ? 255.0f : v);
        }
      if (binary) {
        f.write(reinterpret_cast<const char*>(&points[3 * i]), 12);
        if (hasNormals()) f.write(reinterpret_cast<const char*>(&normals[3 * i]), 12);
        if (hasColors()) f.write(reinterpret_cast<const char*>(rgb), 3);
      } else {
        std::ostringstream ss;
        ss.precision(9);
        ss << points[3 * i] << ' ' << points[3 * i + 1] << ' ' << points[3 * i + 2];
        if (hasNormals()) ss << ' ' << normals[3 * i] << ' ' << normals[3 * i + 1] << ' ' << normals[3 * i + 2];
        if (hasColors()) ss << ' ' << (int)rgb[0] << ' ' << (int)rgb[1] << ' ' << (int)rgb[2];
        f << ss.str() << '\n';
      }
    }
    if (!f) throw std::runtime_error("write failed: " + file_name);
    return *this;
  }

private:
  static bool finite3(const std::vector<float>& v, size_t i) { return std::isfinite(v[3 * i]) && std::isfinite(v[3 * i + 1]) && std::isfinite(v[3 * i + 2]); }
  PointCloud3f& removeRows(bool by_points, bool by_normals, bool by_colors) {
    const bool has_n = hasNormals(), has_c = hasColors();
    const size_t n = size();
    std::vector<char> bad(n, 0);
    size_t n_bad = 0;
    for (size_t i = 0; i < n; ++i) {
      bad[i] = (by_points && !finite3(points, i)) || (by_normals && !finite3(normals, i)) || (by_colors && !finite3(colors, i));
      n_bad += bad[i];
    }
    if (n_bad == 0) return *this;
    if (n_bad == n) { points.clear(); normals.clear(); colors.clear(); return *this; }
    // as remove() does (:164-186): every hole, in ascending order, takes the last row that stays; the rest keeps its place
    size_t last = n - 1;
    while (bad[last]) --last;
    for (size_t i = 0; i < last; ++i) {
      if (!bad[i]) continue;
      for (int k = 0; k < 3; ++k) {
        points[3 * i + k] = points[3 * last + k];
        if (has_n) normals[3 * i + k] = normals[3 * last + k];
        if (has_c) colors[3 * i + k] = colors[3 * last + k];
      }
      --last;
      while (i < last && bad[last]) --last;
    }
    points.resize(3 * (last + 1));
    if (has_n) normals.resize(3 * (last + 1));
    if (has_c) colors.resize(3 * (last + 1));
    return *this;
  }
  static std::string strip(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && (s[a] == ' ' || s[a] == '\t' || s[a] == '\r')) ++a;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t' || s[b - 1] == '\r' || s[b - 1] == '\n')) --b;
    return s.substr(a, b - a);
  }
  template <typename T>
  static double read_bin(std::istream& f, const std::string& file) {
    T v;
    f.read(reinterpret_cast<char*>(&v), sizeof(T));   // the host is little endian (x86-64 / the GPU boxes)
    if (!f) throw std::runtime_error(file + ": truncated PLY data");
    return (double)v;
  }
  static size_t scalar_size(const std::string& type, const std::string& file) {
    if (type == "double" || type == "float64") return 8;
    if (type == "float" || type == "float32" || type == "uint" || type == "uint32" || type == "int" || type == "int32") return 4;
    if (type == "ushort" || type == "uint16" || type == "short" || type == "int16") return 2;
    if (type == "uchar" || type == "uint8" || type == "char" || type == "int8") return 1;
    throw std::runtime_error(file + ": unknown PLY property type " + type);
  }
  static double read_scalar(std::istream& f, const std::string& type, bool ascii, const std::string& file) {
    if (ascii) {
      double v;
      if (!(f >> v)) throw std::runtime_error(file + ": truncated PLY data");
      return v;
    }
    if (type == "float" || type == "float32") return read_bin<float>(f, file);
    if (type == "double" || type == "float64") return read_bin<double>(f, file);
    if (type == "uchar" || type == "uint8") return read_bin<uint8_t>(f, file);
    if (type == "char" || type == "int8") return read_bin<int8_t>(f, file);
    if (type == "ushort" || type == "uint16") return read_bin<uint16_t>(f, file);
    if (type == "short" || type == "int16") return read_bin<int16_t>(f, file);
    if (type == "uint" || type == "uint32") return read_bin<uint32_t>(f, file);
    if (type == "int" || type == "int32") return read_bin<int32_t>(f, file);
    throw std::runtime_error(file + ": unknown PLY property type " + type);
  }
};

}  // namespace cilantro_hip

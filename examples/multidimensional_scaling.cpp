// examples/multidimensional_scaling.cpp -- the flow of cilantro's examples/multidimensional_scaling.cpp on the GPU engine: 1000 points on a
// wobbling circle, their squared distances, and the classical 2-D embedding computed from the distances alone.
//
//   g++ -O2 -std=c++17 -Iinclude examples/multidimensional_scaling.cpp -o multidimensional_scaling -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./multidimensional_scaling
//
// Differs from the reference example only where the missing pieces force it: no visualizer -- the time, the dimension, the eigenvalues, the
// solver's figures and the largest error of the reproduced pairwise distances are printed.
#include <cilantro_hip/multidimensional_scaling.hpp>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <vector>

#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

using namespace cilantro_hip;

static void generate_input_data(std::vector<float>& original_points, std::vector<float>& dist_sq) {
  const size_t num_points = 1000;
  original_points.resize(3 * num_points);
  for (size_t i = 0; i < num_points; i++) {
    original_points[3 * i + 0] = std::cos((2.0f * M_PI * i) / num_points);
    original_points[3 * i + 1] = std::sin((2.0f * M_PI * i) / num_points);
    original_points[3 * i + 2] = 0.1f * std::sin(10.0f * (2.0f * M_PI * i) / num_points);
  }
  dist_sq.resize(num_points * num_points);
  for (size_t i = 0; i < num_points; i++) {
    for (size_t j = 0; j < num_points; j++) {
      float s = 0.0f;
      for (int k = 0; k < 3; ++k) { const float d = original_points[3 * i + k] - original_points[3 * j + k]; s += d * d; }
      dist_sq[i * num_points + j] = s;
    }
  }
}

int main() {
  std::vector<float> points, distances_sq;
  generate_input_data(points, distances_sq);
  const size_t n = points.size() / 3;
  std::printf("Number of points: %zu\n", n);

  const auto t0 = std::chrono::steady_clock::now();
  MultidimensionalScaling<float, 2> mds(distances_sq.data(), n);
  // MultidimensionalScaling<float> mds(distances_sq.data(), n, 3, true);
  const double elapsed = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  std::printf("Elapsed time: %.2fms\n", elapsed);
  const size_t dim = mds.getEmbeddingDimension();
  std::printf("Embedding dimension: %zu\n", dim);
  std::printf("Eigenvalues:");
  for (float v : mds.getComputedEigenValues()) std::printf(" %.6g", v);
  const cilhip_mds_result& r = mds.getSolverResult();
  std::printf("\nSolver: %zu outer iterations, %zu block products, largest residual %.3g\n", r.outer_iterations, r.block_products, r.max_residual);

  // how well the embedded points reproduce the distances they were computed from (the wobble along z, amplitude 0.1, is what 2-D loses)
  const std::vector<float>& y = mds.getEmbeddedPoints();
  double worst = 0.0;
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < n; j++) {
      double s = 0.0;
      for (size_t k = 0; k < dim; ++k) { const double d = (double)y[i * dim + k] - (double)y[j * dim + k]; s += d * d; }
      worst = std::fmax(worst, std::fabs(s - (double)distances_sq[i * n + j]));
    }
  std::printf("Largest error of a reproduced squared distance: %.4g\n", worst);
  return 0;
}

// examples/principal_component_analysis.cpp -- cilantro's examples/principal_component_analysis.cpp on the GPU engine: the 8 corners of a
// 1 x 100 x 1000 box; mean, eigenvalues and eigenvectors printed.
//
//   g++ -O2 -std=c++17 -Iinclude examples/principal_component_analysis.cpp -o principal_component_analysis -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./principal_component_analysis
#include <cilantro_hip/principal_component_analysis.hpp>

#include <cstdio>
#include <vector>

int main() {
  const std::vector<float> points = {0, 0, 0, 1, 0, 0, 0, 100, 0, 0, 0, 1000, 0, 100, 1000, 1, 0, 1000, 1, 100, 0, 1, 100, 1000};

  cilantro_hip::PrincipalComponentAnalysis3f pca(points.data(), points.size() / 3);

  std::printf("Data mean:");
  for (float v : pca.getDataMean()) std::printf(" %g", v);
  std::printf("\nEigenvalues:");
  for (float v : pca.getEigenValues()) std::printf(" %g", v);
  std::printf("\nEigenvectors: \n");      // as the reference prints its matrix: eigenvector c is column c
  const std::vector<float>& V = pca.getEigenVectors();
  for (int k = 0; k < 3; ++k) std::printf("%g %g %g\n", V[0 * 3 + k], V[1 * 3 + k], V[2 * 3 + k]);
  return 0;
}

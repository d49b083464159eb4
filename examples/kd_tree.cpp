// examples/kd_tree.cpp -- the flow of cilantro's examples/kd_tree.cpp on the GPU engine: the 8 corners of the unit cube, the query
// (0.1, 0.1, 0.4), its 2 nearest corners within the squared radius 1.001, printed; then the same question in 4-D through KDTreeXf.
//
//   g++ -O2 -std=c++17 -Iinclude examples/kd_tree.cpp -o kd_tree -Lcilantro_amd/lib -lcilantro_hip
//       -Wl,-rpath,$PWD/cilantro_amd/lib -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib      (one command line)
//   ./kd_tree
//
// Prints "Neighbor indices: 0 3" and "Neighbor distances: 0.18 0.38", as the reference example does.
#include <cilantro_hip/kd_tree.hpp>
#include <cilantro_hip/normal_estimation.hpp>

#include <iostream>
#include <vector>

using namespace cilantro_hip;

static void print(const Neighborhood& nn) {
  std::cout << "Neighbor indices: ";
  for (size_t i = 0; i < nn.size(); i++) std::cout << nn[i].index << " ";
  std::cout << std::endl;
  std::cout << "Neighbor distances: ";
  for (size_t i = 0; i < nn.size(); i++) std::cout << nn[i].value << " ";
  std::cout << std::endl;
}

int main() {
  const std::vector<float> points = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1, 1};
  const std::vector<float> query = {0.1f, 0.1f, 0.4f};

  KDTree3f tree{ConstPointsView(points)};
  print(tree.kNNInRadiusSearch(ConstPointsView(query), 2, 1.001f)[0]);

  // the 16 corners of the 4-D unit cube (corner i: the bits of i, lowest first) and a query one fifth along the new axis
  std::vector<float> points4;
  for (int i = 0; i < 16; ++i)
    for (int b = 0; b < 4; ++b) points4.push_back((float)((i >> b) & 1));
  const float query4[4] = {0.1f, 0.1f, 0.4f, 0.2f};

  KDTreeXf tree4{ConstDataView(points4, 4)};
  std::cout << "4-D:" << std::endl;
  print(tree4.kNNInRadiusSearch(query4, 2, 1.001f));
  return 0;
}

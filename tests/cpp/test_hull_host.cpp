// test_hull_host.cpp -- csrc/hull_host.hpp on its own: no HIP, no library call.
//   test_hull_host <raw f32 file> <n> <dim> <simplicial 0|1>
// reads n x dim packed floats, drops the non-finite rows, builds the hull of ALL the rest and prints it:
//   empty <0|1> failed <0|1> nonfinite <count>
//   V <input indices, ascending>
//   F <vertex-list indices of facet k>          (one line per facet, in order)
//   N <neighbour facets of facet k>
//   A <area> <volume>
// tests/test_hull_refs_cpu.py compares the lists with tests/_hull_refs.py and runs a second build of this file under ASan / UBSan.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../cilantro_amd/csrc/hull_host.hpp"

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: test_hull_host file n dim simplicial\n"); return 2; }
  const size_t n = (size_t)std::atoll(argv[2]);
  const int dim = std::atoi(argv[3]);
  const bool simplicial = std::atoi(argv[4]) != 0;
  std::vector<float> raw(n * (size_t)dim);
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  const size_t got = std::fread(raw.data(), sizeof(float), raw.size(), f);
  std::fclose(f);
  if (got != raw.size()) { std::fprintf(stderr, "short file\n"); return 2; }
  std::vector<double> P;
  std::vector<unsigned> ids;
  double M = 0.0;
  for (size_t i = 0; i < n; ++i) {
    bool fin = true;
    for (int c = 0; c < dim; ++c) fin = fin && std::isfinite(raw[i * dim + c]);
    if (!fin) continue;
    for (int c = 0; c < 3; ++c) {
      const double v = c < dim ? (double)raw[i * dim + c] : 0.0;
      P.push_back(v);
      M = std::max(M, std::fabs(v));
    }
    ids.push_back((unsigned)i);
  }
  cilhip::HullResult r;
  r.dim = dim;
  if (ids.size() >= (size_t)dim + 1) r = cilhip::hull_build(P.data(), ids.size(), dim, cilhip::hull_tol(0.0, M), simplicial);
  std::printf("empty %d failed %d nonfinite %zu\n", r.empty ? 1 : 0, r.failed ? 1 : 0, n - ids.size());
  if (r.empty) return r.failed ? 1 : 0;
  std::printf("V");
  for (const unsigned v : r.vertex_ids) std::printf(" %u", ids[v]);
  std::printf("\n");
  for (size_t k = 0; k + 1 < r.facet_offsets.size(); ++k) {
    std::printf("F");
    for (unsigned j = r.facet_offsets[k]; j < r.facet_offsets[k + 1]; ++j) std::printf(" %u", r.facet_indices[j]);
    std::printf("\nN");
    for (unsigned j = r.facet_offsets[k]; j < r.facet_offsets[k + 1]; ++j) std::printf(" %u", r.facet_neighbors[j]);
    std::printf("\n");
  }
  std::printf("A %.17g %.17g\n", r.area, r.volume);
  return 0;
}

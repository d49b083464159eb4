// tests/cpp/test_kmeans_nd.cpp -- the C++ KMeansXf (include/cilantro_hip/clustering.hpp) on an input that tests/test_gpu_kmeans_nd.py
// writes, so that its labels and centroids can be compared byte for byte with the Python mirror's:
//   test_kmeans_nd run <n> <dim> <k> <max_iter> <in> <out>
// <in>:  n * dim floats (the points, point-major), then k * dim floats (the starting centroids)
// <out>: k * dim floats (the centroids), n uint32 (the labels), one uint64 (the iterations), one uint64 (the non-empty clusters of the
//        cluster-to-points map, whose lists must hold every point once, ascending)
#include <cilantro_hip/clustering.hpp>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace cilantro_hip;

int main(int argc, char** argv) {
  if (argc != 8 || std::strcmp(argv[1], "run")) {
    std::fprintf(stderr, "usage: test_kmeans_nd run <n> <dim> <k> <max_iter> <in> <out>\n");
    return 2;
  }
  try {
    const size_t n = std::strtoull(argv[2], nullptr, 10), dim = std::strtoull(argv[3], nullptr, 10), k = std::strtoull(argv[4], nullptr, 10);
    const size_t max_iter = std::strtoull(argv[5], nullptr, 10);
    std::vector<float> x(n * dim), start(k * dim);
    std::FILE* in = std::fopen(argv[6], "rb");
    if (!in) return 1;
    const bool read = std::fread(x.data(), sizeof(float), x.size(), in) == x.size() && std::fread(start.data(), sizeof(float), start.size(), in) == start.size();
    std::fclose(in);
    if (!read) return 1;
    KMeansXf<> km(x.data(), n, dim);
    km.cluster(start, max_iter);
    if (km.getNumberOfPoints() != n || km.getNumberOfClusters() != k || km.getClusterCentroids().size() != k * dim) return 1;
    std::vector<uint32_t> labels(n);
    for (size_t i = 0; i < n; ++i) labels[i] = (uint32_t)km.getPointToClusterIndexMap()[i];
    uint64_t nonempty = 0, listed = 0;
    for (size_t c = 0; c < k; ++c) {
      const auto& list = km.getClusterToPointIndicesMap()[c];
      nonempty += list.empty() ? 0 : 1;
      for (size_t j = 0; j < list.size(); ++j, ++listed)
        if (list[j] >= n || labels[list[j]] != c || (j && list[j] <= list[j - 1])) return 1;
    }
    if (listed != n) return 1;
    const uint64_t iterations = km.getNumberOfPerformedIterations();
    std::FILE* out = std::fopen(argv[7], "wb");
    if (!out) return 1;
    const bool wrote = std::fwrite(km.getClusterCentroids().data(), sizeof(float), k * dim, out) == k * dim && std::fwrite(labels.data(), sizeof(uint32_t), n, out) == n &&
                       std::fwrite(&iterations, sizeof(iterations), 1, out) == 1 && std::fwrite(&nonempty, sizeof(nonempty), 1, out) == 1;
    if (std::fclose(out) != 0 || !wrote) return 1;
    std::printf("run OK: %zu iterations\n", (size_t)iterations);
    return 0;
  } catch (const std::exception& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return 3;
  }
}

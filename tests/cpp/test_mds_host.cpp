// csrc/mds_host.hpp alone (no device, no library): M3's sizes, the magnitude order, M4's test, the filter plan, M5's dimension estimate.
//   g++ -std=c++17 -ffp-contract=off tests/cpp/test_mds_host.cpp -o test_mds_host && ./test_mds_host
#include "../../cilantro_amd/csrc/mds_host.hpp"

#include <cstdio>
#include <vector>

using namespace cilhip;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

int main() {
  {  // M3 (:106-118, :40-42)
    MdsSizes z = mds_sizes(1000, 2, false);
    CHECK(z.dim == 2 && !z.estimate && z.nev == 2);
    z = mds_sizes(1000, 3, true);
    CHECK(z.dim == 3 && z.estimate && z.nev == 4);
    z = mds_sizes(4, 3, true);
    CHECK(z.dim == 3 && z.nev == 3);      // min(max_dim + 1, n - 1)
    z = mds_sizes(10, 0, true);
    CHECK(z.dim == 2 && !z.estimate && z.nev == 2);
    z = mds_sizes(10, 10, true);
    CHECK(z.dim == 2 && !z.estimate && z.nev == 2);
    z = mds_sizes(10, 9, false);
    CHECK(z.dim == 9 && z.nev == 9);
  }
  {  // descending magnitude, equal magnitudes by ascending index
    const double v[7] = {-1.0, 3.0, -3.0, 0.0, 2.5, -7.0, 3.0};
    int order[7];
    magnitude_order(v, 7, order);
    const int want[7] = {5, 1, 2, 6, 4, 0, 3};
    for (int i = 0; i < 7; ++i) CHECK(order[i] == want[i]);
    int one[1];
    magnitude_order(v, 1, one);
    CHECK(one[0] == 0);
  }
  {  // Spectra's test with float's literals
    const double eps23 = (double)std::pow(FLT_EPSILON, 2.0f / 3.0f), tol = (double)1e-7f;
    CHECK(mds_accepts(0.99 * tol * 500.0, 500.0) && !mds_accepts(1.01 * tol * 500.0, -500.0));
    CHECK(mds_accepts(0.99 * tol * eps23, 0.0) && !mds_accepts(1.01 * tol * eps23, 1e-9));
    CHECK(!mds_accepts(NAN, 1.0));
  }
  {  // the filter plan
    MdsFilterPlan p = mds_filter_plan(500.0, 1e-5, 500.0, 0.0, 24);      // nothing to protect below a0: the full degree
    CHECK(p.e == 1e-5 && p.degree == 24);
    p = mds_filter_plan(100.0, 1.0, 1.0, 0.0, 24);      // gain between 100 and 1 (= e): m acosh(100) <= ln 1e6 -> m = 2
    CHECK(p.e == 1.0 && p.degree == 2);
    CHECK(2.0 * std::acosh(100.0) <= std::log(1e6) && 3.0 * std::acosh(100.0) > std::log(1e6));
    p = mds_filter_plan(0.5, 0.5, 0.5, 0.0, 24);       // a flat block (the simplex): e = a0 / 2
    CHECK(p.e == 0.25 && p.degree == 24);
    p = mds_filter_plan(0.5, 0.0, 0.5, 0.0, 24);       // a zero in the block
    CHECK(p.e == 0.25);
    p = mds_filter_plan(4.0, 1.0, 4.0, 480.0, 24);     // locked pairs far above: m (acosh(480) - acosh(4)) <= ln 1e10
    const double above = std::acosh(480.0) - std::acosh(4.0);
    CHECK(p.degree == (int)std::floor(std::log(1e10) / above) && p.degree >= 1 && p.degree < 24);
    p = mds_filter_plan(1e-5, 1e-6, 1e-12, 500.0, 24);
    CHECK(p.degree >= 1);
    p = mds_filter_plan(1.0, 0.9995, 1.0, 0.0, 7);      // `least` within 1e-3 of a0
    CHECK(p.e == 0.5 && p.degree == 7);
  }
  {  // estimateEmbeddingDimensionEigengap (:10-31)
    const float a[4] = {500.0f, 500.0f, 5.0f, 0.0f};
    CHECK(mds_embedding_dim(a, 4, 3) == 2);
    const float b[3] = {9.0f, 1.0f, 0.5f};
    CHECK(mds_embedding_dim(b, 3, 2) == 1);
    const float c[4] = {2.0f, 2.0f, 2.0f, 2.0f};
    CHECK(mds_embedding_dim(c, 4, 3) == 3);      // all equal: max_dim
    const float d[3] = {4.0f, 3.0f, 0.0f};
    CHECK(mds_embedding_dim(d, 3, 2) == 2);
    const float e[1] = {1.0f};
    CHECK(mds_embedding_dim(e, 1, 5) == 5);      // one value: no spread
    const float f[3] = {1.0f, 1.0f, 1.0f + FLT_EPSILON};      // a spread of exactly epsilon is not "below epsilon"
    CHECK(mds_embedding_dim(f, 3, 2) == 1);
  }
  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

// tests/cpp/test_small_sym.cpp -- cilantro_amd/csrc/small_sym.hpp on the host: the Jacobi eigensolver and the Cholesky factorisation of the
// spectral embedding's small dense work, on random, repeated-eigenvalue, diagonal and 1 x 1 matrices, against closed forms and residuals
// <= 1e-13 ||M||.  Built and run by tests/test_spectral_refs_cpu.py, once more under -fsanitize=address,undefined.
#include "../../cilantro_amd/csrc/small_sym.hpp"

#include <cstdio>
#include <random>
#include <vector>

using namespace cilhip;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static double frob(const std::vector<double>& M) { double s = 0.0; for (double v : M) s += v * v; return std::sqrt(s); }

// ||M V - V diag(w)||_F, ||V^T V - I||_F and the order of w
static void check_eigen(const std::vector<double>& M, int m, const char* what) {
  std::vector<double> A(M), w(m), V((size_t)m * m);
  sym_jacobi(A.data(), m, w.data(), V.data());
  const double norm = frob(M) > 0.0 ? frob(M) : 1.0;
  double res = 0.0, orth = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      double mv = 0.0, vv = 0.0;
      for (int k = 0; k < m; ++k) { mv += M[(size_t)i * m + k] * V[(size_t)k * m + j]; vv += V[(size_t)k * m + i] * V[(size_t)k * m + j]; }
      const double r = mv - V[(size_t)i * m + j] * w[j], o = vv - (i == j ? 1.0 : 0.0);
      res += r * r; orth += o * o;
    }
  CHECK(std::sqrt(res) <= 1e-13 * norm, "%s (m = %d): residual %.3g of %.3g", what, m, std::sqrt(res), norm);
  CHECK(std::sqrt(orth) <= 1e-13 * m, "%s (m = %d): orthogonality %.3g", what, m, std::sqrt(orth));
  for (int i = 0; i + 1 < m; ++i) CHECK(w[i] <= w[i + 1], "%s (m = %d): eigenvalues not ascending at %d", what, m, i);
}

static void check_cholesky(const std::vector<double>& G, int m, const char* what) {
  std::vector<double> R((size_t)m * m), Ri((size_t)m * m);
  CHECK(sym_cholesky(G.data(), m, R.data()), "%s (m = %d): refused a positive definite matrix", what, m);
  upper_inverse(R.data(), m, Ri.data());
  const double norm = frob(G);
  double res = 0.0, inv = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      double rr = 0.0, ri = 0.0;
      for (int k = 0; k < m; ++k) { rr += R[(size_t)k * m + i] * R[(size_t)k * m + j]; ri += R[(size_t)i * m + k] * Ri[(size_t)k * m + j]; }
      res += (rr - G[(size_t)i * m + j]) * (rr - G[(size_t)i * m + j]);
      inv += (ri - (i == j ? 1.0 : 0.0)) * (ri - (i == j ? 1.0 : 0.0));
      if (i > j) CHECK(R[(size_t)i * m + j] == 0.0 && Ri[(size_t)i * m + j] == 0.0, "%s (m = %d): not upper triangular", what, m);
    }
  CHECK(std::sqrt(res) <= 1e-13 * norm, "%s (m = %d): R^T R residual %.3g of %.3g", what, m, std::sqrt(res), norm);
  CHECK(std::sqrt(inv) <= 1e-11 * m, "%s (m = %d): R R^-1 residual %.3g", what, m, std::sqrt(inv));
}

int main() {
  std::mt19937_64 rng(7);
  std::normal_distribution<double> normal(0.0, 1.0);
  for (int m : {1, 2, 3, 5, 8, 13, 25, 32}) {
    std::vector<double> B((size_t)m * m), M((size_t)m * m), G((size_t)m * m);
    for (double& v : B) v = normal(rng);
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) {
        M[(size_t)i * m + j] = 0.5 * (B[(size_t)i * m + j] + B[(size_t)j * m + i]);
        double g = 0.0;
        for (int k = 0; k < m; ++k) g += B[(size_t)k * m + i] * B[(size_t)k * m + j];
        G[(size_t)i * m + j] = g + (i == j ? 1.0 : 0.0);      // B^T B + I
      }
    check_eigen(M, m, "random symmetric");
    check_eigen(G, m, "random positive definite");
    check_cholesky(G, m, "random positive definite");
    // repeated eigenvalues: Q diag(0, 0, 0, 2, 2, 5, ...) Q^T with Q from the solver itself
    std::vector<double> A(M), w(m), Q((size_t)m * m), Rp((size_t)m * m, 0.0);
    sym_jacobi(A.data(), m, w.data(), Q.data());
    std::vector<double> lam(m);
    for (int i = 0; i < m; ++i) lam[i] = i < 3 ? 0.0 : i < 5 ? 2.0 : 5.0;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j)
        for (int k = 0; k < m; ++k) Rp[(size_t)i * m + j] += Q[(size_t)i * m + k] * lam[k] * Q[(size_t)j * m + k];
    check_eigen(Rp, m, "repeated eigenvalues");
    std::vector<double> A2(Rp), w2(m), V2((size_t)m * m);
    sym_jacobi(A2.data(), m, w2.data(), V2.data());
    for (int i = 0; i < m; ++i) CHECK(std::fabs(w2[i] - lam[i]) <= 1e-13 * 5.0 * m, "repeated eigenvalues (m = %d): value %d is %.17g, not %.1f", m, i, w2[i], lam[i]);
  }
  {      // closed forms
    double A[4] = {2.0, 1.0, 1.0, 2.0}, w[2], V[4];
    sym_jacobi(A, 2, w, V);
    CHECK(std::fabs(w[0] - 1.0) <= 1e-15 && std::fabs(w[1] - 3.0) <= 1e-15, "2 x 2: %.17g %.17g", w[0], w[1]);
    CHECK(std::fabs(std::fabs(V[0]) - std::sqrt(0.5)) <= 1e-15 && std::fabs(V[0] + V[2]) <= 1e-15, "2 x 2: first vector (%.17g, %.17g)", V[0], V[2]);
    double one[1] = {-4.5}, w1[1], V1[1];
    sym_jacobi(one, 1, w1, V1);
    CHECK(w1[0] == -4.5 && V1[0] == 1.0, "1 x 1 eigenpair");
    double D[9] = {3.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0, 2.0}, wd[3], Vd[9];
    sym_jacobi(D, 3, wd, Vd);
    CHECK(wd[0] == -1.0 && wd[1] == 2.0 && wd[2] == 3.0 && Vd[1 * 3 + 0] == 1.0 && Vd[2 * 3 + 1] == 1.0 && Vd[0 * 3 + 2] == 1.0, "diagonal 3 x 3: sorted by permutation");
    double Z[9] = {0.0}, wz[3], Vz[9];
    sym_jacobi(Z, 3, wz, Vz);
    CHECK(wz[0] == 0.0 && wz[2] == 0.0 && Vz[0] == 1.0 && Vz[4] == 1.0, "zero matrix");
    double g1[1] = {9.0}, r1[1], i1[1];
    CHECK(sym_cholesky(g1, 1, r1) && r1[0] == 3.0, "1 x 1 Cholesky");
    upper_inverse(r1, 1, i1);
    CHECK(i1[0] == 1.0 / 3.0, "1 x 1 inverse");
    double G2[4] = {4.0, 2.0, 2.0, 5.0}, R2[4];
    CHECK(sym_cholesky(G2, 2, R2) && R2[0] == 2.0 && R2[1] == 1.0 && R2[2] == 0.0 && R2[3] == 2.0, "2 x 2 Cholesky: [[2, 1], [0, 2]]");
    double bad[4] = {1.0, 2.0, 2.0, 1.0}, Rb[4];
    CHECK(!sym_cholesky(bad, 2, Rb), "an indefinite matrix is refused");
    double zero[1] = {0.0};
    CHECK(!sym_cholesky(zero, 1, Rb), "a zero pivot is refused");
    const double nan = std::nan("");
    double gn[1] = {nan};
    CHECK(!sym_cholesky(gn, 1, Rb), "a NaN pivot is refused");
  }
  if (failures) { std::printf("%d FAILED\n", failures); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

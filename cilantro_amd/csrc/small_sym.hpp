// small_sym.hpp -- the small dense f64 algebra of the spectral embedding (rule S4), plain C++ for the host:
//   sym_jacobi    all eigenpairs of a symmetric m x m matrix (cyclic Jacobi), eigenvalues ascending
//   sym_cholesky  G = R^T R, R upper triangular (false: a pivot is not positive)
//   upper_inverse R^-1 of an upper triangular matrix
// m <= SMALL_SYM_MAX = 32; every matrix is row-major m x m.  No allocation, no dependency: tests/cpp/test_small_sym.cpp runs it alone.
#pragma once

#include <cmath>
#include <cstddef>

namespace cilhip {

constexpr int SMALL_SYM_MAX = 32;

// A (symmetric, destroyed) -> w[m] ascending, V[m*m]: column j of V (V[i*m + j]) is the unit eigenvector of w[j].
// Cyclic Jacobi with the rotation of Rutishauser's formulation; ends when the off-diagonal mass is zero in f64 or after 64 sweeps.
inline void sym_jacobi(double* A, int m, double* w, double* V) {
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) V[i * m + j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0;
    for (int p = 0; p < m; ++p)
      for (int q = p + 1; q < m; ++q) off += A[p * m + q] * A[p * m + q];
    if (off == 0.0) break;
    for (int p = 0; p < m; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A[p * m + q];
        if (apq == 0.0) continue;
        const double app = A[p * m + p], aqq = A[q * m + q];
        // negligible against both diagonal entries: the rotation would be the identity in f64
        if (std::fabs(apq) <= 1e-300 || (std::fabs(app) + std::fabs(apq) == std::fabs(app) && std::fabs(aqq) + std::fabs(apq) == std::fabs(aqq) && sweep > 3)) {
          A[p * m + q] = A[q * m + p] = 0.0;
          continue;
        }
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < m; ++k) {      // columns p, q
          const double akp = A[k * m + p], akq = A[k * m + q];
          A[k * m + p] = c * akp - s * akq;
          A[k * m + q] = s * akp + c * akq;
        }
        for (int k = 0; k < m; ++k) {      // rows p, q
          const double apk = A[p * m + k], aqk = A[q * m + k];
          A[p * m + k] = c * apk - s * aqk;
          A[q * m + k] = s * apk + c * aqk;
        }
        A[p * m + q] = A[q * m + p] = 0.0;
        for (int k = 0; k < m; ++k) {
          const double vkp = V[k * m + p], vkq = V[k * m + q];
          V[k * m + p] = c * vkp - s * vkq;
          V[k * m + q] = s * vkp + c * vkq;
        }
      }
  }
  for (int i = 0; i < m; ++i) w[i] = A[i * m + i];
  for (int i = 0; i < m; ++i) {      // ascending (selection sort; equal values keep their order)
    int lo = i;
    for (int j = i + 1; j < m; ++j) if (w[j] < w[lo]) lo = j;
    if (lo == i) continue;
    const double wl = w[lo];
    for (int j = lo; j > i; --j) w[j] = w[j - 1];
    w[i] = wl;
    for (int k = 0; k < m; ++k) {
      const double vl = V[k * m + lo];
      for (int j = lo; j > i; --j) V[k * m + j] = V[k * m + j - 1];
      V[k * m + i] = vl;
    }
  }
}

// G (symmetric positive definite; the upper triangle is read) -> R upper triangular with G = R^T R; the strict lower triangle of R is zero.
inline bool sym_cholesky(const double* G, int m, double* R) {
  for (int i = 0; i < m * m; ++i) R[i] = 0.0;
  for (int j = 0; j < m; ++j) {
    double d = G[j * m + j];
    for (int k = 0; k < j; ++k) d -= R[k * m + j] * R[k * m + j];
    if (!(d > 0.0) || !std::isfinite(d)) return false;
    const double rjj = std::sqrt(d);
    R[j * m + j] = rjj;
    for (int c = j + 1; c < m; ++c) {
      double v = G[j * m + c];
      for (int k = 0; k < j; ++k) v -= R[k * m + j] * R[k * m + c];
      R[j * m + c] = v / rjj;
    }
  }
  return true;
}

// Rinv = R^-1, R upper triangular with a non-zero diagonal
inline void upper_inverse(const double* R, int m, double* Rinv) {
  for (int i = 0; i < m * m; ++i) Rinv[i] = 0.0;
  for (int j = 0; j < m; ++j) {
    Rinv[j * m + j] = 1.0 / R[j * m + j];
    for (int i = j - 1; i >= 0; --i) {
      double v = 0.0;
      for (int k = i + 1; k <= j; ++k) v += R[i * m + k] * Rinv[k * m + j];
      Rinv[i * m + j] = -v / R[i * m + i];
    }
  }
}

}  // namespace cilhip

// Small dense host algebra shared by the feature units (no HIP include: a plain C++ program can use it).
#pragma once

#include <cmath>
#include <utility>
#include <vector>

namespace gemma_hip {

// What small_inverse met.  The callers disagree on a NaN pivot, so it is reported and not decided here: vc carries on (NaN reaches
// its outputs, as LU in the reference would), mqs refuses the matrix.
enum SmallInverse { SMALL_INVERSE_OK = 0, SMALL_INVERSE_NAN_PIVOT = 1, SMALL_INVERSE_ZERO_PIVOT = 2 };

// Gauss-Jordan inverse with partial pivoting of the m x m matrix A, in place (LUDecomp + LUInvert of the small matrices,
// src/mathfunc.cpp).  An exactly zero pivot stops the elimination (A is left as it stands: not an inverse); a NaN pivot does not.
inline SmallInverse small_inverse(std::vector<double> &A, int m) {
  std::vector<double> I((size_t)m * m, 0.0);
  SmallInverse st = SMALL_INVERSE_OK;
  for (int i = 0; i < m; ++i) I[i * m + i] = 1.0;
  for (int k = 0; k < m; ++k) {
    int p = k;
    for (int i = k + 1; i < m; ++i)
      if (std::fabs(A[i * m + k]) > std::fabs(A[p * m + k])) p = i;
    if (A[p * m + k] == 0.0) return SMALL_INVERSE_ZERO_PIVOT;
    if (std::isnan(A[p * m + k])) st = SMALL_INVERSE_NAN_PIVOT;
    if (p != k)
      for (int j = 0; j < m; ++j) {
        std::swap(A[k * m + j], A[p * m + j]);
        std::swap(I[k * m + j], I[p * m + j]);
      }
    const double d = 1.0 / A[k * m + k];
    for (int j = 0; j < m; ++j) {
      A[k * m + j] *= d;
      I[k * m + j] *= d;
    }
    for (int i = 0; i < m; ++i) {
      if (i == k) continue;
      const double f = A[i * m + k];
      if (f == 0.0) continue;
      for (int j = 0; j < m; ++j) {
        A[i * m + j] -= f * A[k * m + j];
        I[i * m + j] -= f * I[k * m + j];
      }
    }
  }
  A = I;
  return st;
}

} // namespace gemma_hip

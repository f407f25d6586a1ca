// CPU check of gemma_amd/csrc/host_linalg.h (the one small_inverse of the vc and mqs units), a stand-alone program:
//   * A A^-1 = I on fixed 1 x 1, 3 x 3 (first pivot 0: a row swap) and 8 x 8 matrices.  Bound on the largest entry of A X - I:
//     Gauss-Jordan with partial pivoting is backward stable up to the growth factor, so the residual is of the order
//     m eps ||A|| ||X||; asserted at 8 m eps ||A||_inf ||X||_inf (a few ulps of the condition number);
//   * an exactly zero column: SMALL_INVERSE_ZERO_PIVOT;
//   * a NaN entry: the elimination completes, the result holds NaN (what the vc caller relies on: NaN reaches its outputs) and
//     the status is SMALL_INVERSE_NAN_PIVOT (what the mqs caller relies on: it refuses the matrix).
// tests/test_host_linalg_cpu.py builds it plain and with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../gemma_amd/csrc/host_linalg.h"

using namespace gemma_hip;

static int failures = 0;
#define EXPECT(cond, ...)                \
  do {                                   \
    if (!(cond)) {                       \
      ++failures;                        \
      printf("FAILED %s: ", #cond);      \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
    }                                    \
  } while (0)

static double norm_inf(const std::vector<double> &A, int m) {
  double r = 0.0;
  for (int i = 0; i < m; ++i) {
    double s = 0.0;
    for (int j = 0; j < m; ++j) s += std::fabs(A[i * m + j]);
    r = std::fmax(r, s);
  }
  return r;
}

static void check_inverse(const char *name, const std::vector<double> &A, int m) {
  std::vector<double> X = A;
  const SmallInverse st = small_inverse(X, m);
  EXPECT(st == SMALL_INVERSE_OK, "%s: status %d", name, (int)st);
  double worst = 0.0;
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) {
      long double s = 0.0L;
      for (int k = 0; k < m; ++k) s += (long double)A[i * m + k] * (long double)X[k * m + j];
      worst = std::fmax(worst, std::fabs((double)(s - (i == j ? 1.0L : 0.0L))));
    }
  const double bound = 8.0 * m * std::numeric_limits<double>::epsilon() * norm_inf(A, m) * norm_inf(X, m);
  printf("%s: max |A X - I| = %.3g, bound %.3g\n", name, worst, bound);
  EXPECT(worst <= bound, "%s: %.3g > %.3g", name, worst, bound);
}

static bool any_nan(const std::vector<double> &A) {
  for (double v : A)
    if (std::isnan(v)) return true;
  return false;
}

int main() {
  check_inverse("1 x 1", {4.0}, 1);
  check_inverse("3 x 3, zero in the first pivot position", {0.0, 2.0, 1.0, 1.0, 1.0, 0.0, 3.0, 0.0, 2.0}, 3);
  {
    std::vector<double> A(64);
    for (int i = 0; i < 8; ++i)
      for (int j = 0; j < 8; ++j) A[i * 8 + j] = (double)((i * 7 + j * 3) % 11 - 5) + (i == j ? 12.0 : 0.0) + 1.0 / (i + j + 1);
    check_inverse("8 x 8", A, 8);
  }
  {
    std::vector<double> Z = {1.0, 0.0, 2.0, 3.0, 0.0, 1.0, 2.0, 0.0, 5.0}; // column 1 is exactly zero
    const SmallInverse st = small_inverse(Z, 3);
    EXPECT(st == SMALL_INVERSE_ZERO_PIVOT, "zero column: status %d", (int)st);
    std::vector<double> z1 = {0.0};
    EXPECT(small_inverse(z1, 1) == SMALL_INVERSE_ZERO_PIVOT, "1 x 1 zero");
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  {
    std::vector<double> N = {nan, 1.0, 0.0, 1.0, 3.0, 1.0, 0.0, 1.0, 2.0}; // the first pivot itself
    const SmallInverse st = small_inverse(N, 3);
    EXPECT(st == SMALL_INVERSE_NAN_PIVOT, "NaN on the diagonal: status %d", (int)st);
    EXPECT(N.size() == 9 && any_nan(N), "NaN on the diagonal: the result holds no NaN");
  }
  {
    std::vector<double> N = {2.0, 1.0, 0.0, 1.0, 3.0, 1.0, nan, 1.0, 2.0}; // below the diagonal: never chosen, reaches the last pivot
    const SmallInverse st = small_inverse(N, 3);
    EXPECT(st == SMALL_INVERSE_NAN_PIVOT, "NaN below the diagonal: status %d", (int)st);
    EXPECT(any_nan(N), "NaN below the diagonal: the result holds no NaN");
  }
  if (failures) return 1;
  printf("ok\n");
  return 0;
}

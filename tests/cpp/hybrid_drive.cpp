// GEMMA's -vc 2 loop (VC::CalcVCreml, src/vc.cpp:1785-1809) around include/gemma_vc_hybrid.hpp, with the function handed in by
// the caller through a C callback: tests/test_reference_pin.py drives the numpy restatement of LogRL_dev12 with it, as
// gemma_amd/csrc/vc_tu.hip drives the device's.  Built as a shared library by the test.
#include <vector>

#include "gemma_vc_hybrid.hpp"

extern "C" {
// fdf(x, f, J): f (n) and J (n x n, row-major) at x; 0 = defined, 2 = not defined there (a failed step: HybridSJ::EVAL_OUTSIDE,
// as the device fit treats an H that is not positive definite), anything else = the evaluation failed (the solve stops)
typedef int (*hybrid_fdf)(const double *x, double *f, double *J);

// x (n): the start in, the solution out.  iters (iter_cap x n): x of iteration 0 .. the last.  *status: 0 converged
// (sum |f| < epsabs), 1 max_iter reached, 2 / 3 no progress (GSL_ENOPROG / GSL_ENOPROGJ), -1 the function failed.
// Returns the iteration count.
int hybrid_drive(int n, double *x, hybrid_fdf fdf, int max_iter, double epsabs, double *iters, int iter_cap, int *status) {
  gemma_vc::HybridSJ s((size_t)n, [&](const std::vector<double> &xx, std::vector<double> &f, std::vector<double> &J, bool) {
    f.assign(n, 0.0);
    J.assign((size_t)n * n, 0.0);
    const int rc = fdf(xx.data(), f.data(), J.data());
    return rc == 0 ? (int)gemma_vc::HybridSJ::EVAL_OK
                   : rc == 2 ? (int)gemma_vc::HybridSJ::EVAL_OUTSIDE : (int)gemma_vc::HybridSJ::EVAL_FAIL;
  });
  std::vector<double> x0(x, x + n);
  int rows = 0;
  auto push = [&](const std::vector<double> &v) {
    if (rows < iter_cap)
      for (int i = 0; i < n; ++i) iters[rows * n + i] = v[i];
    ++rows;
  };
  push(x0);
  *status = -1;
  if (s.set(x0) != gemma_vc::HybridSJ::OK) return 0;
  int iter = 0, st = 0;
  *status = 1;
  do {
    ++iter;
    st = s.iterate();
    if (st) break;
    push(s.x);
    if (s.residual_below(epsabs)) {
      *status = 0;
      break;
    }
  } while (iter < max_iter);
  if (st == gemma_vc::HybridSJ::ENOPROG) *status = 2;
  else if (st == gemma_vc::HybridSJ::ENOPROGJ) *status = 3;
  else if (st != gemma_vc::HybridSJ::OK) *status = -1;
  for (int i = 0; i < n; ++i) x[i] = s.x[i];
  return iter;
}
}

// Roots found by include/gemma_vc_hybrid.hpp (GSL hybridsj restated) on standard nonlinear systems, for tests/test_vc_cpu.py:
//   hybrid_check <system> <x0...>  ->  "status iterations x..." (the GEMMA loop: residual sum |f| < 1e-10 here, 1000 iterations)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemma_vc_hybrid.hpp"

typedef std::vector<double> V;

static bool sys(const std::string &name, const V &x, V &f, V &J) {
  const size_t n = x.size();
  f.assign(n, 0.0);
  J.assign(n * n, 0.0);
  if (name == "rosenbrock") { // f = (10 (x1 - x0^2), 1 - x0)
    f[0] = 10 * (x[1] - x[0] * x[0]);
    f[1] = 1 - x[0];
    J = {-20 * x[0], 10, -1, 0};
  } else if (name == "powell_badly_scaled") {
    f[0] = 1e4 * x[0] * x[1] - 1;
    f[1] = std::exp(-x[0]) + std::exp(-x[1]) - 1.0001;
    J = {1e4 * x[1], 1e4 * x[0], -std::exp(-x[0]), -std::exp(-x[1])};
  } else if (name == "trig") { // f_i = n - sum cos x_j + i (1 - cos x_i) - sin x_i
    double sc = 0;
    for (double v : x) sc += std::cos(v);
    for (size_t i = 0; i < n; ++i) {
      f[i] = n - sc + (i + 1) * (1 - std::cos(x[i])) - std::sin(x[i]);
      for (size_t j = 0; j < n; ++j) J[i * n + j] = std::sin(x[j]);
      J[i * n + i] += (i + 1) * std::sin(x[i]) - std::cos(x[i]);
    }
  } else if (name == "quadratic3") { // x_i^2 + sum x - c_i
    const double c[3] = {5, 7, 10};
    double s = x[0] + x[1] + x[2];
    for (size_t i = 0; i < 3; ++i) {
      f[i] = x[i] * x[i] + s - c[i];
      for (size_t j = 0; j < 3; ++j) J[i * 3 + j] = 1.0 + (i == j ? 2 * x[i] : 0.0);
    }
  } else {
    return false;
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string name = argv[1];
  V x0;
  for (int i = 2; i < argc; ++i) x0.push_back(atof(argv[i]));
  gemma_vc::HybridSJ s(x0.size(), [&](const V &x, V &f, V &J, bool) { return sys(name, x, f, J) ? 0 : 1; });
  int st = s.set(x0), iter = 0;
  while (st == 0 && iter < 1000) {
    ++iter;
    st = s.iterate();
    if (st || s.residual_below(1e-10)) break;
  }
  printf("%d %d", st, iter);
  for (double v : s.x) printf(" %.17g", v);
  printf("\n");
  return 0;
}

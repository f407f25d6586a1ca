// Powell's hybrid method with an analytic Jacobian, scaled (MINPACK hybrj, Moré, Garbow & Hillstrom, ANL-80-74, 1980): the
// algorithm behind GSL's gsl_multiroot_fdfsolver_hybridsj, which GEMMA's REML variance-component fit drives
// (VC::CalcVCreml, src/vc.cpp:1726-1931).  Written from the published algorithm; dense form for the small systems of a
// variance-component fit (n_vc + 1 <= 9 unknowns):
//  - a trust region of radius delta in the norm ||D x||, D = the running maximum of the Jacobian's column norms (scaled mode);
//    delta starts at 100 ||D x0|| (or 100 when that is 0);
//  - each iteration takes ONE trial step: the dogleg combination of the Gauss-Newton step (R p = Q^T f, J = Q R) and the scaled
//    steepest-descent step, then one evaluation of f at x - p;
//  - the ratio of actual to predicted reduction of ||f|| shrinks (ratio < 0.1: delta / 2) or grows (delta = max(delta, 2 ||D p||),
//    or 2 ||D p|| when the ratio is within 0.1 of 1) the region; the step is accepted when ratio >= 1e-4;
//  - after each trial the Jacobian takes Broyden's rank-1 update J += (f(x - p) - f(x) + J p) (D^2 (-p))^T / ||D p||^2 (MINPACK
//    updates its QR factors by Givens rotations; here the small dense J is refactored);
//  - after two consecutive failures, the analytic Jacobian is evaluated again at the current point;
//  - no progress over 5 Jacobian evaluations or 10 iterations ends the solve with a status (GSL_ENOPROGJ / GSL_ENOPROG).
// The caller runs the loop as GEMMA does: iterate, then stop on sum |f| < 1e-3 (gsl_multiroot_test_residual) or 100 iterations.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

namespace gemma_vc {

class HybridSJ {
 public:
  // fdf(x, f, J): f (n) and J (n x n, row-major, J[i * n + j] = d f_i / d x_j) at x.  want_j = false: only f is used (the
  // library's evaluator computes both at once and caches the point).  Returns EVAL_OK, EVAL_FAIL (the solve stops) or
  // EVAL_OUTSIDE: f is not defined at a trial point (H not numerically positive definite there), and the trial counts as a
  // failed step (the region halves) -- where GSL would evaluate the function anyway and, in practice, reject the step.
  enum { EVAL_OK = 0, EVAL_FAIL = 1, EVAL_OUTSIDE = 2 };
  typedef std::function<int(const std::vector<double> &x, std::vector<double> &f, std::vector<double> &J, bool want_j)> Fdf;
  enum { OK = 0, EBADFUNC = 1, ENOPROG = 2, ENOPROGJ = 3 };

  HybridSJ(size_t n, Fdf fdf) : n_(n), fdf_(fdf) {}

  int set(const std::vector<double> &x0) {
    x = x0;
    f.assign(n_, 0.0);
    J.assign(n_ * n_, 0.0);
    if (fdf_(x, f, J, true) != EVAL_OK) return EBADFUNC;
    diag.assign(n_, 0.0);
    update_diag(true);
    double xn = scaled_norm(x);
    delta_ = 100.0 * xn;
    if (delta_ == 0.0) delta_ = 100.0;
    fnorm_ = norm(f);
    ncfail_ = ncsuc_ = nslow1_ = nslow2_ = 0;
    jeval_ = true;
    iter_ = 1;
    factor();
    return OK;
  }

  int iterate() {
    const size_t n = n_;
    std::vector<double> p(n), xt(n), ft(n), Jt;
    dogleg(p);
    for (size_t j = 0; j < n; ++j) xt[j] = x[j] - p[j];
    std::vector<double> dp(n);
    for (size_t j = 0; j < n; ++j) dp[j] = diag[j] * p[j];
    const double pnorm = norm(dp);
    if (iter_ == 1) delta_ = std::min(delta_, pnorm);
    const int ev = fdf_(xt, ft, Jt, false);
    if (ev == EVAL_FAIL) return EBADFUNC;
    if (ev == EVAL_OUTSIDE) { // a failed step: no Broyden update
      ncsuc_ = 0;
      ++ncfail_;
      delta_ *= 0.5;
      ++nslow1_;
      if (jeval_) ++nslow2_;
      jeval_ = false;
      return after_step();
    }
    const double fnorm1 = norm(ft);
    const double actred = fnorm1 < fnorm_ ? 1.0 - (fnorm1 / fnorm_) * (fnorm1 / fnorm_) : -1.0;
    // predicted: ||f - J p||
    std::vector<double> lin(n);
    for (size_t i = 0; i < n; ++i) {
      double s = f[i];
      for (size_t j = 0; j < n; ++j) s -= J[i * n + j] * p[j];
      lin[i] = s;
    }
    const double t = norm(lin);
    const double prered = t < fnorm_ ? 1.0 - (t / fnorm_) * (t / fnorm_) : 0.0;
    const double ratio = prered > 0.0 ? actred / prered : 0.0;
    if (ratio < 0.1) {
      ncsuc_ = 0;
      ++ncfail_;
      delta_ *= 0.5;
    } else {
      ncfail_ = 0;
      ++ncsuc_;
      if (ratio >= 0.5 || ncsuc_ > 1) delta_ = std::max(delta_, pnorm / 0.5);
      if (std::fabs(ratio - 1.0) <= 0.1) delta_ = pnorm / 0.5;
    }
    // Broyden: J += (ft - f - J (-p)) (D^2 (-p))^T / pnorm^2
    if (pnorm > 0.0) {
      for (size_t i = 0; i < n; ++i) {
        double jp = 0.0;
        for (size_t j = 0; j < n; ++j) jp -= J[i * n + j] * p[j];
        const double r = (ft[i] - f[i] - jp) / pnorm;
        for (size_t j = 0; j < n; ++j) J[i * n + j] += r * (diag[j] * (diag[j] * -p[j]) / pnorm);
      }
    }
    if (ratio >= 1e-4) {
      x = xt;
      f = ft;
      fnorm_ = fnorm1;
      ++iter_;
    }
    nslow1_ = actred >= 0.001 ? 0 : nslow1_ + 1;
    if (jeval_) ++nslow2_; // counted after a Jacobian evaluation, cleared by any good step
    if (actred >= 0.1) nslow2_ = 0;
    jeval_ = false;
    return after_step();
  }

  // gsl_multiroot_test_residual: sum |f_i| < epsabs
  bool residual_below(double epsabs) const {
    double s = 0.0;
    for (double v : f) s += std::fabs(v);
    return s < epsabs;
  }

  std::vector<double> x, f, J, diag;

 private:
  int after_step() {
    const size_t n = n_;
    if (ncfail_ == 2) { // the analytic Jacobian at the current point
      std::vector<double> fx(n);
      if (fdf_(x, fx, J, true) != EVAL_OK) return EBADFUNC;
      f = fx;
      fnorm_ = norm(f);
      update_diag(false);
      ncfail_ = 0;
      jeval_ = true;
    }
    factor();
    if (nslow2_ == 5) return ENOPROGJ;
    if (nslow1_ == 10) return ENOPROG;
    return OK;
  }

  size_t n_;
  Fdf fdf_;
  std::vector<double> Q_, R_; // J = Q R (Householder, dense)
  double delta_ = 0.0, fnorm_ = 0.0;
  int ncfail_ = 0, ncsuc_ = 0, nslow1_ = 0, nslow2_ = 0, iter_ = 0;
  bool jeval_ = true;

  static double norm(const std::vector<double> &v) {
    double s = 0.0;
    for (double a : v) s += a * a;
    return std::sqrt(s);
  }
  double scaled_norm(const std::vector<double> &v) const {
    double s = 0.0;
    for (size_t j = 0; j < n_; ++j) s += (diag[j] * v[j]) * (diag[j] * v[j]);
    return std::sqrt(s);
  }
  void update_diag(bool first) {
    for (size_t j = 0; j < n_; ++j) {
      double s = 0.0;
      for (size_t i = 0; i < n_; ++i) s += J[i * n_ + j] * J[i * n_ + j];
      s = std::sqrt(s);
      if (first) diag[j] = (s == 0.0) ? 1.0 : s;
      else diag[j] = std::max(diag[j], s);
    }
  }
  void factor() { // Householder QR of J: Q (n x n), R upper
    const size_t n = n_;
    R_ = J;
    Q_.assign(n * n, 0.0);
    for (size_t i = 0; i < n; ++i) Q_[i * n + i] = 1.0;
    std::vector<double> v(n);
    for (size_t k = 0; k < n; ++k) {
      double a = 0.0;
      for (size_t i = k; i < n; ++i) a += R_[i * n + k] * R_[i * n + k];
      a = std::sqrt(a);
      if (a == 0.0) continue;
      if (R_[k * n + k] > 0) a = -a;
      for (size_t i = 0; i < n; ++i) v[i] = (i < k) ? 0.0 : R_[i * n + k];
      v[k] -= a;
      double vv = 0.0;
      for (size_t i = k; i < n; ++i) vv += v[i] * v[i];
      if (vv == 0.0) continue;
      for (size_t j = 0; j < n; ++j) { // R = (I - 2 v v^T / vv) R
        double s = 0.0;
        for (size_t i = k; i < n; ++i) s += v[i] * R_[i * n + j];
        s = 2.0 * s / vv;
        for (size_t i = k; i < n; ++i) R_[i * n + j] -= s * v[i];
      }
      for (size_t i = 0; i < n; ++i) { // Q = Q (I - 2 v v^T / vv)
        double s = 0.0;
        for (size_t j = k; j < n; ++j) s += Q_[i * n + j] * v[j];
        s = 2.0 * s / vv;
        for (size_t j = k; j < n; ++j) Q_[i * n + j] -= s * v[j];
      }
    }
  }
  // MINPACK dogleg: p minimising ||f - J p|| on the dogleg path inside ||D p|| <= delta
  void dogleg(std::vector<double> &p) const {
    const size_t n = n_;
    std::vector<double> qtf(n), gn(n, 0.0);
    for (size_t j = 0; j < n; ++j) {
      double s = 0.0;
      for (size_t i = 0; i < n; ++i) s += Q_[i * n + j] * f[i];
      qtf[j] = s;
    }
    double rmax = 0.0;
    for (size_t j = 0; j < n; ++j) rmax = std::max(rmax, std::fabs(R_[j * n + j]));
    const double eps = 2.220446049250313e-16;
    for (size_t jj = n; jj-- > 0;) { // Gauss-Newton: R gn = qtf; a zero pivot takes eps * max |R_jj|
      double s = qtf[jj];
      for (size_t k = jj + 1; k < n; ++k) s -= R_[jj * n + k] * gn[k];
      double d = R_[jj * n + jj];
      if (d == 0.0) d = eps * (rmax > 0.0 ? rmax : 1.0);
      gn[jj] = s / d;
    }
    double qnorm = 0.0;
    for (size_t j = 0; j < n; ++j) qnorm += (diag[j] * gn[j]) * (diag[j] * gn[j]);
    qnorm = std::sqrt(qnorm);
    if (qnorm <= delta_) {
      p = gn;
      return;
    }
    std::vector<double> g(n, 0.0), Rg(n, 0.0);
    for (size_t j = 0; j < n; ++j) { // scaled gradient direction: (R^T qtf)_j / D_j
      double s = 0.0;
      for (size_t i = 0; i <= j; ++i) s += R_[i * n + j] * qtf[i];
      g[j] = s / diag[j];
    }
    const double gnorm = norm(g);
    double sgnorm = 0.0, alpha = delta_ / qnorm;
    if (gnorm != 0.0) {
      for (size_t j = 0; j < n; ++j) g[j] = (g[j] / gnorm) / diag[j];
      for (size_t i = 0; i < n; ++i) {
        double s = 0.0;
        for (size_t j = i; j < n; ++j) s += R_[i * n + j] * g[j];
        Rg[i] = s;
      }
      const double t = norm(Rg);
      sgnorm = (gnorm / t) / t;
      alpha = 0.0;
      if (sgnorm < delta_) {
        const double bnorm = norm(qtf);
        double t2 = (bnorm / gnorm) * (bnorm / qnorm) * (sgnorm / delta_);
        t2 = t2 - (delta_ / qnorm) * (sgnorm / delta_) * (sgnorm / delta_) +
             std::sqrt((t2 - delta_ / qnorm) * (t2 - delta_ / qnorm) +
                       (1.0 - (delta_ / qnorm) * (delta_ / qnorm)) * (1.0 - (sgnorm / delta_) * (sgnorm / delta_)));
        alpha = ((delta_ / qnorm) * (1.0 - (sgnorm / delta_) * (sgnorm / delta_))) / t2;
      }
    }
    const double t = (1.0 - alpha) * std::min(sgnorm, delta_);
    p.assign(n, 0.0);
    for (size_t j = 0; j < n; ++j) p[j] = t * g[j] + alpha * gn[j];
  }
};

} // namespace gemma_vc

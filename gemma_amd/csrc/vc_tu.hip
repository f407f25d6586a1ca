// Variance-component estimation with one or more kinships (GEMMA -vc 1 / -vc 2) as its own translation unit (see vc_tu.h):
// the SPD inverse (spd_inv.hip.h), the memory-bound passes (vc.hip.h), their orchestration, and the host algebra of
//   VC::CalcVChe   src/vc.cpp:1503-1724  (Haseman-Elston regression)
//   VC::CalcVCreml src/vc.cpp:1726-1931  (REML, average information, GSL hybridsj on log sigma2)
//   UpdateParam / LogRL_dev1 / LogRL_dev2 / LogRL_dev12  src/vc.cpp:168-380
// restated line by line where the arithmetic is O(n_vc^2) and moved to the device where it is O(n^2) or O(n^3).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gemma_hip.h"
#include "../../include/gemma_vc_hybrid.hpp"
#include "tu_common.h"
#include "host_linalg.h"
#include "spd_inv.hip.h"
#include "vc.hip.h"
#include "vc_tu.h"

namespace gemma_hip {

namespace {

struct VcState {
  bool ready = false;
  long n = 0, ld = 0, ldk = 0;
  int nvc = 0, c = 0;
  std::vector<const double *> K; // device, ldk
  DevBuf Kown;                   // host kinships copied here (nvc x n x ld)
  DevBuf H;                      // H -> H^-1 -> P (n x ld)
  DevBuf Wd, Xd, Yd, partial;    // W (n x c); mat-vec operands (n x 2c or n x 16)
  std::vector<double> W, y, traceG;
  SpdWork spd;
  hipEvent_t ev[6] = {};
  // the last two evaluated points of the REML fit: x -> (f, J)
  struct Cached {
    std::vector<double> x, f, J;
  } cache[2];
  int cache_next = 0;
  long evals = 0, invs = 0;
  double t[5] = {0, 0, 0, 0, 0};
} g_vc;

const hipStream_t S0 = nullptr;

// true when W^T W (m x m) is numerically rank-deficient, whatever the units of W's columns: the test runs on the equilibrated
// S = D^-1/2 W^T W D^-1/2 (D = its diagonal, so S_jj = 1), where a pivot of the partially pivoted elimination at or below
// 16 m eps counts as 0.  An exactly repeated column leaves a pivot of a few eps there, not 0: the pivot row is scaled by the
// rounded reciprocal 1 / A_kk, so its twin no longer cancels exactly -- small_inverse alone would return the inverse of a
// singular matrix.  A zero (or NaN) column is rank-deficient.
bool rank_deficient(const std::vector<double> &A, int m) {
  std::vector<double> r(m), S(m * m);
  for (int j = 0; j < m; ++j) {
    if (!(A[j * m + j] > 0.0)) return true;
    r[j] = 1.0 / std::sqrt(A[j * m + j]);
  }
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < m; ++j) S[i * m + j] = A[i * m + j] * r[i] * r[j];
  const double tol = 16.0 * m * 2.220446049250313e-16;
  for (int k = 0; k < m; ++k) {
    int p = k;
    for (int i = k + 1; i < m; ++i)
      if (std::fabs(S[i * m + k]) > std::fabs(S[p * m + k])) p = i;
    if (!(std::fabs(S[p * m + k]) > tol)) return true;
    if (p != k)
      for (int j = 0; j < m; ++j) std::swap(S[k * m + j], S[p * m + j]);
    for (int i = k + 1; i < m; ++i) {
      const double f = S[i * m + k] / S[k * m + k];
      for (int j = k; j < m; ++j) S[i * m + j] -= f * S[k * m + j];
    }
  }
  return false;
}

double dot(const double *a, const double *b, long n, long sa = 1, long sb = 1) {
  double s = 0.0;
  for (long i = 0; i < n; ++i) s += a[i * sa] * b[i * sb];
  return s;
}

// out (n x m, host) = M X, X (n x m, host), m <= 16: one pass over M
int matvec(const double *M, long ldm, const std::vector<double> &X, int m, std::vector<double> &out, std::string &msg) {
  double *const Xd = g_vc.Xd.as<double>(), *const Yd = g_vc.Yd.as<double>();
  const long n = g_vc.n;
  TU_CHK(hipMemcpyAsync(Xd, X.data(), (size_t)n * m * 8, hipMemcpyHostToDevice, S0));
  hipLaunchKernelGGL(vc_matvec_kernel, dim3((unsigned)((n + 3) / 4)), dim3(VC_THREADS), 0, S0, M, n, ldm, Xd, m, Yd);
  TU_CHK(hipGetLastError());
  out.resize((size_t)n * m);
  TU_CHK(hipMemcpyAsync(out.data(), Yd, (size_t)n * m * 8, hipMemcpyDeviceToHost, S0));
  TU_CHK(hipStreamSynchronize(S0));
  return GEMMA_HIP_OK;
}

// tr(A_p B_p) for the given pairs, one pass; partial sums added on the host in workgroup order
int traces(const std::vector<std::pair<const double *, long>> &a, const std::vector<std::pair<const double *, long>> &b,
           std::vector<double> &tr, std::string &msg) {
  VcPairs pr;
  pr.count = (int)a.size();
  for (int p = 0; p < pr.count; ++p) {
    pr.a[p] = a[p].first;
    pr.lda[p] = a[p].second;
    pr.b[p] = b[p].first;
    pr.ldb[p] = b[p].second;
  }
  hipLaunchKernelGGL(vc_trace_kernel, dim3(VC_TRACE_BLOCKS), dim3(VC_THREADS), 0, S0, pr, g_vc.n, g_vc.partial.as<double>());
  TU_CHK(hipGetLastError());
  std::vector<double> part((size_t)VC_TRACE_BLOCKS * pr.count);
  TU_CHK(hipMemcpyAsync(part.data(), g_vc.partial.p, part.size() * 8, hipMemcpyDeviceToHost, S0));
  TU_CHK(hipStreamSynchronize(S0));
  tr.assign(pr.count, 0.0);
  for (int blk = 0; blk < VC_TRACE_BLOCKS; ++blk)
    for (int p = 0; p < pr.count; ++p) tr[p] += part[(size_t)blk * pr.count + p];
  return GEMMA_HIP_OK;
}

int diagonal(const double *M, long ldm, std::vector<double> &d, std::string &msg) {
  d.resize(g_vc.n);
  TU_CHK(hipMemcpy2D(d.data(), 8, M, (ldm + 1) * 8, 8, g_vc.n, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

// M (n x n, ldm, device) = sum_l s_l K_l + s_e I  (out may alias the single input)
int assemble(const std::vector<const double *> &Ks, long ldk, const std::vector<double> &s, double s_e, double *out, long ldo,
             std::string &msg) {
  VcMats mats;
  mats.count = (int)Ks.size();
  for (int l = 0; l < mats.count; ++l) {
    mats.m[l] = Ks[l];
    mats.s[l] = s[l];
  }
  const unsigned grid = (unsigned)std::min<long>(g_vc.n, 4096);
  hipLaunchKernelGGL(vc_assemble_kernel, dim3(grid), dim3(VC_THREADS), 0, S0, mats, g_vc.n, ldk, s_e, out, ldo);
  TU_CHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

// CenterVector(y, W), src/mathfunc.cpp:455-475
void center_vector(std::vector<double> &v) {
  const long n = g_vc.n;
  const int c = g_vc.c;
  std::vector<double> WtW(c * c), Wty(c), b(c, 0.0);
  for (int a = 0; a < c; ++a) {
    for (int e = 0; e < c; ++e) WtW[a * c + e] = dot(&g_vc.W[a], &g_vc.W[e], n, c, c);
    Wty[a] = dot(&g_vc.W[a], v.data(), n, c, 1);
  }
  small_inverse(WtW, c);
  for (int a = 0; a < c; ++a)
    for (int e = 0; e < c; ++e) b[a] += WtW[a * c + e] * Wty[e];
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a) v[i] -= g_vc.W[i * c + a] * b[a];
}

double vector_var(const std::vector<double> &v) { // VectorVar, src/mathfunc.cpp:134-144
  double m = 0.0, m2 = 0.0;
  for (double d : v) {
    m += d;
    m2 += d * d;
  }
  m /= (double)v.size();
  m2 /= (double)v.size();
  return m2 - m * m;
}

} // namespace

int spd_inverse_x(double *A, long n, long lda, double *logdet, long *bad_pivot, hipStream_t s, std::string &msg) {
  const bool inplace = (lda % 2) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0;
  if (inplace) return spd_inverse_device(A, n, lda, logdet, bad_pivot, g_vc.spd, s, msg);
  const long ld = (n + 1) & ~1L; // odd leading dimension: through an aligned copy
  ScopedBuf Tb;
  int rc = Tb.reserve((size_t)n * ld * 8, "vc", msg);
  if (rc) return rc;
  double *T = Tb.as<double>();
  hipError_t e = hipMemcpy2DAsync(T, ld * 8, A, lda * 8, n * 8, n, hipMemcpyDeviceToDevice, s);
  if (e == hipSuccess) {
    rc = spd_inverse_device(T, n, ld, logdet, bad_pivot, g_vc.spd, s, msg);
    if (rc == 0) e = hipMemcpy2DAsync(A, lda * 8, T, ld * 8, n * 8, n, hipMemcpyDeviceToDevice, s);
    if (rc == 0 && e == hipSuccess) e = hipStreamSynchronize(s);
  }
  if (e != hipSuccess) return hip_err(e, "spd_inverse", msg);
  return rc;
}

void vc_release_x() {
  g_vc.Kown.release(); g_vc.H.release(); g_vc.Wd.release(); g_vc.Xd.release(); g_vc.Yd.release(); g_vc.partial.release();
  g_vc.K.clear();
  g_vc.ready = false;
  for (auto &c : g_vc.cache) c.x.clear();
}

void vc_tu_shutdown() {
  vc_release_x();
  g_vc.spd.release();
  for (auto &e : g_vc.ev)
    if (e) (void)hipEventDestroy(e);
  for (auto &e : g_vc.ev) e = nullptr;
}

int vc_setup_x(long n, int n_vc, const double *const *K, long ldk, bool device, const double *W, int c, const double *y,
               std::string &msg) {
  vc_release_x();
  if (!g_vc.ev[0])
    for (auto &e : g_vc.ev) TU_CHK(hipEventCreate(&e));
  g_vc.n = n;
  g_vc.nvc = n_vc;
  g_vc.c = c;
  g_vc.ld = (n + 1) & ~1L;
  g_vc.W.assign(W, W + (size_t)n * c);
  g_vc.y.assign(y, y + n);
  int rc;
  const size_t nn = (size_t)n * g_vc.ld;
  if (device) {
    g_vc.ldk = ldk;
    for (int l = 0; l < n_vc; ++l) g_vc.K.push_back(K[l]);
  } else {
    g_vc.ldk = g_vc.ld;
    if ((rc = g_vc.Kown.reserve(nn * n_vc * 8, "vc", msg))) return rc;
    for (int l = 0; l < n_vc; ++l) {
      TU_CHK(hipMemcpy2D(g_vc.Kown.as<double>() + l * nn, g_vc.ld * 8, K[l], ldk * 8, n * 8, n, hipMemcpyHostToDevice));
      g_vc.K.push_back(g_vc.Kown.as<double>() + l * nn);
    }
  }
  const int xw = std::max(2 * c, VC_MAX_VEC);
  if ((rc = g_vc.H.reserve(nn * 8, "vc", msg)) || (rc = g_vc.Wd.reserve((size_t)n * c * 8, "vc", msg)) ||
      (rc = g_vc.Xd.reserve((size_t)n * xw * 8, "vc", msg)) || (rc = g_vc.Yd.reserve((size_t)n * xw * 8, "vc", msg)) ||
      (rc = g_vc.partial.reserve((size_t)VC_TRACE_BLOCKS * VC_MAX_PAIRS * 8, "vc", msg)))
    return rc;
  TU_CHK(hipMemcpy(g_vc.Wd.p, W, (size_t)n * c * 8, hipMemcpyHostToDevice));
  // v_traceG: the mean diagonal of each (CenterMatrix(G)-centred) kinship, src/gemma.cpp:2341-2351
  g_vc.traceG.clear();
  for (int l = 0; l < n_vc; ++l) {
    std::vector<double> d;
    if ((rc = diagonal(g_vc.K[l], g_vc.ldk, d, msg))) return rc;
    double s = 0.0;
    for (double v : d) s += v;
    g_vc.traceG.push_back(s / (double)n);
  }
  g_vc.evals = g_vc.invs = 0;
  for (double &t : g_vc.t) t = 0.0;
  g_vc.ready = true;
  return GEMMA_HIP_OK;
}

int vc_he_x(VcResult &R, std::string &msg) {
  double *const Wd = g_vc.Wd.as<double>(), *const Xd = g_vc.Xd.as<double>(), *const Yd = g_vc.Yd.as<double>();
  const long n = g_vc.n, ld = g_vc.ld;
  const int nvc = g_vc.nvc, c = g_vc.c;
  const double r = (double)n / (double)(n - c);
  int rc;
  // K_scale: the W-centred, mean-diagonal-scaled copies (released at the end of the fit)
  ScopedBuf Ksb;
  const size_t nn = (size_t)n * ld;
  if ((rc = Ksb.reserve(nn * nvc * 8, "vc", msg))) return rc;
  double *Ks = Ksb.as<double>();
  std::vector<const double *> Kt;
  std::vector<double> traceG_new;
  // Q = W (W^T W)^-1
  std::vector<double> WtW(c * c), Q((size_t)n * c, 0.0);
  for (int a = 0; a < c; ++a)
    for (int e = 0; e < c; ++e) WtW[a * c + e] = dot(&g_vc.W[a], &g_vc.W[e], n, c, c);
  if (rank_deficient(WtW, c) || small_inverse(WtW, c) == SMALL_INVERSE_ZERO_PIVOT) { // no HE fit, no REML start
    msg = "vc: W^T W is singular";
    return GEMMA_HIP_EINVAL;
  }
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a)
      for (int e = 0; e < c; ++e) Q[i * c + a] += g_vc.W[i * c + e] * WtW[e * c + a];
  for (int l = 0; l < nvc; ++l) {
    double *T = Ks + l * nn;
    TU_CHK(hipMemcpy2DAsync(T, ld * 8, g_vc.K[l], g_vc.ldk * 8, n * 8, n, hipMemcpyDeviceToDevice, S0));
    // CenterMatrix(G, W) = G - Q (GW)^T - GW Q^T + Q (W^T G W) Q^T = G - [Q B] [B Q]^T, B = GW - Q (W^T G W) / 2
    TU_CHK(launch_dgemm('N', 'N', n, c, n, 1.0, T, ld, Wd, c, 0.0, Yd, c, false, false, S0));
    std::vector<double> GW((size_t)n * c), M(c * c), LR((size_t)n * 4 * c);
    TU_CHK(hipMemcpyAsync(GW.data(), Yd, GW.size() * 8, hipMemcpyDeviceToHost, S0));
    TU_CHK(hipStreamSynchronize(S0));
    for (int a = 0; a < c; ++a)
      for (int e = 0; e < c; ++e) M[a * c + e] = dot(&g_vc.W[a], &GW[e], n, c, c);
    for (long i = 0; i < n; ++i)
      for (int a = 0; a < c; ++a) {
        double b = GW[i * c + a];
        for (int e = 0; e < c; ++e) b -= 0.5 * Q[i * c + e] * M[e * c + a];
        LR[i * 2 * c + a] = Q[i * c + a];                      // L = [Q B]
        LR[i * 2 * c + c + a] = b;
        LR[(size_t)n * 2 * c + i * 2 * c + a] = b;             // R = [B Q]
        LR[(size_t)n * 2 * c + i * 2 * c + c + a] = Q[i * c + a];
      }
    TU_CHK(hipMemcpyAsync(Xd, LR.data(), (size_t)n * 2 * c * 8, hipMemcpyHostToDevice, S0));
    TU_CHK(hipMemcpyAsync(Yd, LR.data() + (size_t)n * 2 * c, (size_t)n * 2 * c * 8, hipMemcpyHostToDevice, S0));
    TU_CHK(launch_dgemm('N', 'T', n, n, 2 * c, -1.0, Xd, 2 * c, Yd, 2 * c, 1.0, T, ld, false, false, S0));
    // ScaleMatrix: mean diagonal -> 1
    std::vector<double> dg;
    if ((rc = diagonal(T, ld, dg, msg))) return rc;
    double d = 0.0;
    for (double v : dg) d += v;
    d /= (double)n;
    if (d != 0.0 && (rc = assemble({T}, ld, {1.0 / d}, 0.0, T, ld, msg))) return rc;
    traceG_new.push_back(d);
    Kt.push_back(T);
  }
  // y: centred by W, standardised
  std::vector<double> ys = g_vc.y;
  center_vector(ys);
  const double var_y = vector_var(g_vc.y), var_y_new = vector_var(ys);
  {
    double m = 0.0, v = 0.0;
    for (double a : ys) {
      m += a;
      v += a * a;
    }
    m /= (double)n;
    v /= (double)n;
    v -= m * m;
    for (double &a : ys) a = (a - m) / std::sqrt(v);
  }
  // Kry_i = K_i y - r y ; q_i = Kry_i . y
  std::vector<double> Kry((size_t)n * nvc), q(nvc), out;
  for (int i = 0; i < nvc; ++i) {
    if ((rc = matvec(Kt[i], ld, ys, 1, out, msg))) return rc;
    for (long k = 0; k < n; ++k) Kry[k * nvc + i] = out[k] - r * ys[k];
    q[i] = dot(&Kry[i], ys.data(), n, nvc, 1);
  }
  // yKrKKry (nvc x nvc (nvc + 1))
  const int w = nvc * (nvc + 1);
  std::vector<double> yK((size_t)nvc * w, 0.0);
  for (int l = 0; l < nvc; ++l) {
    if ((rc = matvec(Kt[l], ld, Kry, nvc, out, msg))) return rc; // out[:, i] = K_l Kry_i
    for (int i = 0; i < nvc; ++i)
      for (int j = i; j < nvc; ++j) {
        const double d = dot(&Kry[j], &out[i], n, nvc, nvc);
        yK[i * w + l * nvc + j] = d;
        yK[j * w + l * nvc + i] = d;
      }
  }
  for (int i = 0; i < nvc; ++i)
    for (int j = i; j < nvc; ++j) {
      const double d = dot(&Kry[i], &Kry[j], n, nvc, nvc);
      yK[i * w + nvc * nvc + j] = d;
      yK[j * w + nvc * nvc + i] = d;
    }
  // S_ij = tr(K_i K_j) - r n
  std::vector<std::pair<const double *, long>> pa, pb;
  for (int i = 0; i < nvc; ++i)
    for (int j = i; j < nvc; ++j) {
      pa.push_back({Kt[i], ld});
      pb.push_back({Kt[j], ld});
    }
  std::vector<double> tr;
  if ((rc = traces(pa, pb, tr, msg))) return rc;
  std::vector<double> S(nvc * nvc);
  for (int i = 0, p = 0; i < nvc; ++i)
    for (int j = i; j < nvc; ++j, ++p) S[i * nvc + j] = S[j * nvc + i] = tr[p] - r * (double)n;
  std::vector<double> Si = S;
  if (small_inverse(Si, nvc) == SMALL_INVERSE_ZERO_PIVOT) {
    msg = "vc: the Haseman-Elston matrix S is singular";
    return GEMMA_HIP_ERUNTIME;
  }
  std::vector<double> pve(nvc, 0.0), qvar(nvc * nvc, 0.0), tmp(nvc * nvc, 0.0), Var(nvc * nvc, 0.0);
  for (int i = 0; i < nvc; ++i)
    for (int j = 0; j < nvc; ++j) pve[i] += Si[i * nvc + j] * q[j];
  double s = 1.0;
  for (int i = 0; i < nvc; ++i) {
    for (int a = 0; a < nvc; ++a)
      for (int b = 0; b < nvc; ++b) qvar[a * nvc + b] += yK[a * w + i * nvc + b] * pve[i];
    s -= pve[i];
  }
  for (int a = 0; a < nvc; ++a)
    for (int b = 0; b < nvc; ++b) qvar[a * nvc + b] = 2.0 * (qvar[a * nvc + b] + yK[a * w + nvc * nvc + b] * s);
  for (int a = 0; a < nvc; ++a)
    for (int b = 0; b < nvc; ++b)
      for (int k = 0; k < nvc; ++k) tmp[a * nvc + b] += Si[a * nvc + k] * qvar[k * nvc + b];
  for (int a = 0; a < nvc; ++a)
    for (int b = 0; b < nvc; ++b)
      for (int k = 0; k < nvc; ++k) Var[a * nvc + b] += tmp[a * nvc + k] * Si[k * nvc + b];
  s = 1.0;
  double v = 0.0;
  R.pve_total = R.se_pve_total = 0.0;
  for (int i = 0; i < nvc; ++i) {
    const double d = pve[i], f = (var_y_new / traceG_new[i]) * (g_vc.traceG[i] / var_y);
    R.sigma2[i] = d * var_y_new / traceG_new[i];
    R.pve[i] = d * f;
    s -= d;
    R.pve_total += d * f;
    const double sd = std::sqrt(Var[i * nvc + i]);
    R.se_sigma2[i] = sd * var_y_new / traceG_new[i];
    R.se_pve[i] = sd * f;
    for (int j = 0; j < nvc; ++j) {
      v += Var[i * nvc + j];
      R.se_pve_total += Var[i * nvc + j] * f * (var_y_new / traceG_new[j]) * (g_vc.traceG[j] / var_y);
    }
  }
  R.sigma2[nvc] = s * r * var_y_new;
  R.se_sigma2[nvc] = std::sqrt(v) * r * var_y_new;
  R.se_pve_total = std::sqrt(R.se_pve_total);
  R.iterations = 0;
  R.status = 0;
  R.evaluations = R.inverses = 0;
  R.t_asm = R.t_inv = R.t_pcor = R.t_mv = R.t_tr = 0.0;
  return GEMMA_HIP_OK;
}

namespace {

// UpdateParam + LogRL_dev12 at x (log sigma2, or sigma2 with noconstrain): f = dev1, J = dev2 (the AI matrix)
int reml_eval(const std::vector<double> &x, bool noconstrain, std::vector<double> &f, std::vector<double> &J, std::string &msg) {
  double *const H = g_vc.H.as<double>(), *const Wd = g_vc.Wd.as<double>(), *const Xd = g_vc.Xd.as<double>(), *const Yd = g_vc.Yd.as<double>();
  for (auto &cc : g_vc.cache)
    if (!cc.x.empty() && cc.x == x) {
      f = cc.f;
      J = cc.J;
      return GEMMA_HIP_OK;
    }
  const long n = g_vc.n, ld = g_vc.ld;
  const int nvc = g_vc.nvc, c = g_vc.c, m = nvc + 1;
  std::vector<double> sig(m);
  for (int i = 0; i < m; ++i) sig[i] = noconstrain ? x[i] : std::exp(x[i]);
  int rc;
  TU_CHK(hipEventRecord(g_vc.ev[0], S0));
  if ((rc = assemble(g_vc.K, g_vc.ldk, std::vector<double>(sig.begin(), sig.begin() + nvc), sig[nvc], H, ld, msg))) return rc;
  TU_CHK(hipEventRecord(g_vc.ev[1], S0));
  double logdet = 0.0;
  long bad = -1;
  ++g_vc.evals;
  ++g_vc.invs;
  rc = spd_inverse_device(H, n, ld, &logdet, &bad, g_vc.spd, S0, msg);
  if (rc) {
    if (rc == GEMMA_HIP_ENOTPD) {
      char b[256];
      snprintf(b, sizeof b, "vc: H = sum sigma2_i K_i + sigma2_e I is not positive definite at sigma2 = (");
      msg = b;
      for (int i = 0; i < m; ++i) msg += std::to_string(sig[i]) + (i + 1 < m ? ", " : ")");
      msg += " (pivot " + std::to_string(bad) + "); the fit stops here";
    }
    return rc;
  }
  TU_CHK(hipEventRecord(g_vc.ev[2], S0));
  // P = H^-1 - H^-1 W (W^T H^-1 W)^-1 W^T H^-1: HiW on the device, the c x c inverse on the host, a rank-c update on the GEMM
  TU_CHK(launch_dgemm('N', 'N', n, c, n, 1.0, H, ld, Wd, c, 0.0, Yd, c, false, false, S0));
  std::vector<double> HiW((size_t)n * c), WHW(c * c), Qh((size_t)n * c, 0.0);
  TU_CHK(hipMemcpyAsync(HiW.data(), Yd, HiW.size() * 8, hipMemcpyDeviceToHost, S0));
  TU_CHK(hipStreamSynchronize(S0));
  for (int a = 0; a < c; ++a)
    for (int e = 0; e < c; ++e) WHW[a * c + e] = dot(&g_vc.W[a], &HiW[e], n, c, c);
  if (small_inverse(WHW, c) == SMALL_INVERSE_ZERO_PIVOT) {
    msg = "vc: W^T H^-1 W is singular";
    return GEMMA_HIP_ERUNTIME;
  }
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a)
      for (int e = 0; e < c; ++e) Qh[i * c + a] += HiW[i * c + e] * WHW[e * c + a];
  TU_CHK(hipMemcpyAsync(Xd, Qh.data(), Qh.size() * 8, hipMemcpyHostToDevice, S0));
  TU_CHK(launch_dgemm('N', 'T', n, n, c, -1.0, Xd, c, Yd, c, 1.0, H, ld, false, false, S0));
  TU_CHK(hipEventRecord(g_vc.ev[3], S0));
  // Py, K_i Py, P [K_i Py]
  std::vector<double> Py, KPy((size_t)n * m), PKPy, out;
  if ((rc = matvec(H, ld, g_vc.y, 1, Py, msg))) return rc;
  for (int i = 0; i < nvc; ++i) {
    if ((rc = matvec(g_vc.K[i], g_vc.ldk, Py, 1, out, msg))) return rc;
    for (long k = 0; k < n; ++k) KPy[k * m + i] = out[k];
  }
  for (long k = 0; k < n; ++k) KPy[k * m + nvc] = Py[k];
  if ((rc = matvec(H, ld, KPy, m, PKPy, msg))) return rc;
  for (auto &d : KPy)
    if (std::isnan(d)) d = 0.0;
  for (auto &d : PKPy)
    if (std::isnan(d)) d = 0.0;
  TU_CHK(hipEventRecord(g_vc.ev[4], S0));
  // tr(P K_i), tr(P)
  std::vector<std::pair<const double *, long>> pa, pb;
  for (int i = 0; i < nvc; ++i) {
    pa.push_back({H, ld});
    pb.push_back({g_vc.K[i], g_vc.ldk});
  }
  std::vector<double> tr, dg;
  if ((rc = traces(pa, pb, tr, msg))) return rc;
  if ((rc = diagonal(H, ld, dg, msg))) return rc;
  double trP = 0.0;
  for (double v : dg) trP += v;
  tr.push_back(trP);
  TU_CHK(hipEventRecord(g_vc.ev[5], S0));
  TU_CHK(hipEventSynchronize(g_vc.ev[5]));
  for (int k = 0; k < 5; ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, g_vc.ev[k], g_vc.ev[k + 1]) == hipSuccess) g_vc.t[k] += ms * 1e-3;
  }
  f.assign(m, 0.0);
  J.assign(m * m, 0.0);
  for (int i = 0; i < m; ++i) {
    const double d = dot(Py.data(), &KPy[i], n, 1, m);
    f[i] = noconstrain ? (-0.5 * tr[i] + 0.5 * d) : (-0.5 * tr[i] + 0.5 * d) * sig[i];
    for (int j = i; j < m; ++j) {
      double e = dot(&KPy[i], &PKPy[j], n, m, m);
      e *= noconstrain ? -0.5 : -0.5 * sig[i] * sig[j];
      J[i * m + j] = J[j * m + i] = e;
    }
  }
  auto &slot = g_vc.cache[g_vc.cache_next];
  g_vc.cache_next ^= 1;
  slot.x = x;
  slot.f = f;
  slot.J = J;
  return GEMMA_HIP_OK;
}

} // namespace

int vc_reml_x(bool noconstrain, VcResult &R, std::vector<double> *iters, std::string &msg) {
  const int nvc = g_vc.nvc, m = nvc + 1;
  int rc = vc_he_x(R, msg);
  if (rc) return rc;
  for (auto &cc : g_vc.cache) cc.x.clear();
  g_vc.evals = g_vc.invs = 0;
  for (double &t : g_vc.t) t = 0.0;
  std::vector<double> x(m);
  for (int i = 0; i < m; ++i) x[i] = noconstrain ? R.sigma2[i] : (R.sigma2[i] <= 0 ? std::log(0.1) : std::log(R.sigma2[i]));
  auto push = [&](const std::vector<double> &v) {
    if (iters)
      for (int i = 0; i < m; ++i) iters->push_back(noconstrain ? v[i] : std::exp(v[i]));
  };
  push(x);
  int err = 0;
  std::string err_msg;
  // a trial point where H is not numerically positive definite (a step of the log-scale solver to sigma2 ~ e^200 leaves
  // H ~ sigma2 K, singular to rounding) is a failed step; with noconstrain it ends the fit (the header's ENOTPD divergence)
  gemma_vc::HybridSJ solver(m, [&](const std::vector<double> &xx, std::vector<double> &f, std::vector<double> &J, bool) {
    if (err) return (int)gemma_vc::HybridSJ::EVAL_FAIL;
    int e = reml_eval(xx, noconstrain, f, J, err_msg);
    if (e == GEMMA_HIP_ENOTPD && !noconstrain) return (int)gemma_vc::HybridSJ::EVAL_OUTSIDE;
    if (e) err = e;
    return e == 0 ? (int)gemma_vc::HybridSJ::EVAL_OK : (int)gemma_vc::HybridSJ::EVAL_FAIL;
  });
  int st = solver.set(x);
  int iter = 0, status = 1; // 0 converged (sum |dev1| < 1e-3), 1 iteration limit, 2 / 3 no progress (GSL ENOPROG / ENOPROGJ)
  if (st == 0) {
    do {
      ++iter;
      st = solver.iterate();
      if (st) break;
      push(solver.x);
      if (solver.residual_below(1e-3)) {
        status = 0;
        break;
      }
    } while (iter < 100);
  }
  if (err) {
    msg = err_msg;
    return err;
  }
  if (st == gemma_vc::HybridSJ::ENOPROG) status = 2;
  if (st == gemma_vc::HybridSJ::ENOPROGJ) status = 3;
  // Hessian at the solution, inverted by LU on the host (src/vc.cpp:1820-1826)
  std::vector<double> f, J;
  if ((rc = reml_eval(solver.x, noconstrain, f, J, msg))) return rc;
  std::vector<double> Hi = J;
  if (small_inverse(Hi, m) == SMALL_INVERSE_ZERO_PIVOT) {
    msg = "vc: the average-information matrix is singular at the solution";
    return GEMMA_HIP_ERUNTIME;
  }
  const std::vector<double> &xs = solver.x;
  std::vector<double> s2(m);
  for (int i = 0; i < m; ++i) {
    const double d = noconstrain ? xs[i] : std::exp(xs[i]);
    s2[i] = d;
    R.sigma2[i] = d;
    const double h = noconstrain ? -Hi[i * m + i] : -d * d * Hi[i * m + i];
    R.se_sigma2[i] = std::sqrt(h);
  }
  const std::vector<double> &tg = g_vc.traceG;
  double s = s2[nvc];
  for (int i = 0; i < nvc; ++i) s += tg[i] * s2[i];
  R.pve_total = 0.0;
  for (int i = 0; i < nvc; ++i) {
    R.pve[i] = tg[i] * s2[i] / s;
    R.pve_total += R.pve[i];
  }
  // se(pve) by the delta method, k = n_vc: the total (src/vc.cpp:1860-1918)
  auto grad = [&](int k, int i) {
    double d1 = noconstrain ? 1.0 : std::exp(xs[i]);
    if (k < nvc) {
      if (i == k) d1 *= tg[k] * (s - s2[k] * tg[k]) / (s * s);
      else if (i == nvc) d1 *= -1 * tg[k] * s2[k] / (s * s);
      else d1 *= -1 * tg[i] * tg[k] * s2[k] / (s * s);
    } else {
      if (i == k) d1 *= -1 * (s - s2[nvc]) / (s * s);
      else d1 *= tg[i] * s2[nvc] / (s * s);
    }
    return d1;
  };
  for (int k = 0; k < m; ++k) {
    double d = 0.0;
    for (int i = 0; i < m; ++i)
      for (int j = 0; j < m; ++j) d += -1.0 * grad(k, i) * grad(k, j) * Hi[i * m + j];
    if (k < nvc) R.se_pve[k] = std::sqrt(d);
    else R.se_pve_total = std::sqrt(d);
  }
  R.iterations = iter;
  R.status = status;
  R.evaluations = g_vc.evals;
  R.inverses = g_vc.invs;
  R.t_asm = g_vc.t[0];
  R.t_inv = g_vc.t[1];
  R.t_pcor = g_vc.t[2];
  R.t_mv = g_vc.t[3];
  R.t_tr = g_vc.t[4];
  return GEMMA_HIP_OK;
}

} // namespace gemma_hip

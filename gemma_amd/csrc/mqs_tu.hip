// MQS summary-statistic variance components (GEMMA -gs, -vc 1 -beta) as its own translation unit (see mqs_tu.h): the kernels of
// mqs.hip.h, this unit's instance of the fp64 MFMA SYRK, and the host restatement of
//   PARAM::CalcS      src/param.cpp:1717-1812  (weighted multi-category kinship, CenterMatrix + ScaleMatrix per category)
//   compAKtoS         src/param.cpp:1325-1378
//   JackknifeAKtoS    src/param.cpp:1596-1713  (O(n^3 n_vc^2) scalar loops there; O(n^2 n_vc^2) here)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gemma_hip.h"
#include "dgemm_mfma.hip.h"
#include "mqs.hip.h"
#include "mqs_tu.h"

namespace gemma_hip {

namespace {

struct MqsState {
  bool active = false, haveK = false, haveA = false;
  long n = 0, ni_total = 0, ld = 0, cap = 0;
  int nvc = 0, c = 0, slot = 0;
  double *K = nullptr, *A = nullptr; // n_vc matrices of n x ld each; A == nullptr: A is K
  int *idx = nullptr;
  double *Wt = nullptr, *Wi = nullptr;
  double *X = nullptr, *P = nullptr, *var = nullptr, *w_d = nullptr;
  int *pos = nullptr, *cnt = nullptr, *cat_d = nullptr; // cnt: n_vc counts, then the bad-category flag
  void *stage = nullptr;
  size_t stage_cap = 0;
  long ns[MQS_VCMAX] = {};
  hipStream_t last = nullptr;
} g_mqs;

int herr(hipError_t e, const char *what, std::string &msg) {
  msg = std::string(what) + ": " + hipGetErrorString(e);
  return GEMMA_HIP_ERUNTIME;
}
#define MQCHK(expr)                                    \
  do {                                                 \
    hipError_t e_ = (expr);                            \
    if (e_ != hipSuccess) return herr(e_, #expr, msg); \
  } while (0)

template <class T> int dalloc(T **p, size_t count, std::string &msg) {
  if (hipMalloc((void **)p, std::max<size_t>(count, 2) * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    *p = nullptr;
    msg = "mqs: cannot allocate " + std::to_string(count * sizeof(T)) + " bytes of device memory";
    return GEMMA_HIP_ENOMEM;
  }
  return GEMMA_HIP_OK;
}
template <class T> void dfree(T *&p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

void free_block_buffers() {
  dfree(g_mqs.X);
  dfree(g_mqs.P);
  dfree(g_mqs.var);
  dfree(g_mqs.w_d);
  dfree(g_mqs.pos);
  dfree(g_mqs.cat_d);
  if (g_mqs.stage) (void)hipFree(g_mqs.stage);
  g_mqs.stage = nullptr;
  g_mqs.stage_cap = 0;
  g_mqs.cap = 0;
}

// Gauss-Jordan inverse with partial pivoting of the c x c matrix W^T W (LUDecomp + LUInvert, src/gemma_io.cpp:2977-2980)
bool small_inverse(std::vector<double> &A, int m) {
  std::vector<double> I((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) I[i * m + i] = 1.0;
  for (int k = 0; k < m; ++k) {
    int p = k;
    for (int i = k + 1; i < m; ++i)
      if (std::fabs(A[i * m + k]) > std::fabs(A[p * m + k])) p = i;
    if (!(std::fabs(A[p * m + k]) > 0.0)) return false;
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
  return true;
}

// compAKtoS + JackknifeAKtoS for one ordered pair from the O(n) quantities of the passes.  All sums in
// index order; long double costs nothing at n values per pair.
void finish_pair(long n, int c, const double *sA, const double *dA, const double *sK, const double *dK, const double *h,
                 const double *u, const double *v, double *S_out, double *Svar_out) {
  typedef long double R;
  R SA = 0, SK = 0, trA = 0, trK = 0, T = 0, dot = 0;
  for (long t = 0; t < n; ++t) {
    SA += sA[t];
    SK += sK[t];
    trA += dA[t];
    trK += dK[t];
    T += h[t];
    dot += (R)sA[t] * (R)sK[t];
  }
  const R nn = (R)n;
  R d;
  {
    const R sum_A = SA / nn, sum_K = SK / nn, sum_AK = dot / nn, tA = trA - sum_A, tK = trK - sum_K;
    d = T - 2 * sum_AK + sum_A * sum_K;
    if (tA == 0 || tK == 0) d = 0;
    else d = d / (tA * tK) - 1 / (R)(n - c);
  }
  std::vector<R> dt((size_t)n);
  R m = 0;
  for (long t = 0; t < n; ++t) {
    const R trAK_t = T - 2 * (R)h[t] + (R)dA[t] * (R)dK[t];
    const R sumA_t = (SA - 2 * (R)sA[t] + (R)dA[t]) / (nn - 1), sumK_t = (SK - 2 * (R)sK[t] + (R)dK[t]) / (nn - 1);
    const R trA_t = trA - (R)dA[t], trK_t = trK - (R)dK[t];
    const R sumAK_t = (dot - (R)u[t] - (R)v[t] + (R)h[t] - ((R)sA[t] - (R)dA[t]) * ((R)sK[t] - (R)dK[t])) / (nn - 1);
    const R fa = trA_t - sumA_t, fk = trK_t - sumK_t;
    R e = 0;
    if (!(fa == 0 || fk == 0)) e = (trAK_t - 2 * sumAK_t + sumA_t * sumK_t) / (fa * fk) - 1 / (R)(n - c - 1);
    dt[t] = e;
    m += e;
  }
  m /= nn;
  R var = 0; // around the mean, in a second pass: mean(d^2) - m^2 cancels (ratio 4e8 at n = 1500)
  for (long t = 0; t < n; ++t) var += (dt[t] - m) * (dt[t] - m);
  var = var / nn * (nn - 1);
  *Svar_out = (double)var;
  *S_out = (double)(c == 1 ? nn * d - (nn - 1) * m : d);
}

} // namespace

void mqs_release_x() {
  free_block_buffers();
  dfree(g_mqs.K);
  dfree(g_mqs.A);
  dfree(g_mqs.idx);
  dfree(g_mqs.Wt);
  dfree(g_mqs.Wi);
  dfree(g_mqs.cnt);
  g_mqs.active = g_mqs.haveK = g_mqs.haveA = false;
  g_mqs.n = g_mqs.ni_total = g_mqs.ld = 0;
  g_mqs.nvc = g_mqs.c = 0;
}

void mqs_tu_shutdown() {
  mqs_release_x();
  gemm_aux_destroy();
}

bool mqs_active_x() { return g_mqs.active; }
long mqs_ni_total_x() { return g_mqs.ni_total; }

int mqs_begin_x(long ni_total, const int *indicator, int n_vc, const double *W, int c, int slot, std::string &msg) {
  std::vector<int> idx;
  for (long i = 0; i < ni_total; ++i)
    if (!indicator || indicator[i] != 0) idx.push_back((int)i);
  const long n = (long)idx.size();
  if (n < 2 || n <= c + 1) {
    msg = "mqs_begin: " + std::to_string(n) + " analysed individuals for " + std::to_string(c) + " covariates";
    return GEMMA_HIP_EINVAL;
  }
  if (slot == 1) {
    if (!g_mqs.haveK || g_mqs.active) {
      msg = "mqs_begin: slot 1 fills A beside the K of a finished slot 0 session, and there is none";
      return GEMMA_HIP_EINVAL;
    }
    if (g_mqs.n != n || g_mqs.nvc != n_vc || g_mqs.ni_total != ni_total) {
      msg = "mqs_begin: slot 1 with n = " + std::to_string(n) + ", n_vc = " + std::to_string(n_vc) + "; the kept K has n = " +
            std::to_string(g_mqs.n) + ", n_vc = " + std::to_string(g_mqs.nvc);
      return GEMMA_HIP_EINVAL;
    }
  }
  // (W^T W)^-1 on the host
  std::vector<double> WtW((size_t)c * c, 0.0);
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a)
      for (int e = 0; e < c; ++e) WtW[a * c + e] += W[i * c + a] * W[i * c + e];
  if (!small_inverse(WtW, c)) {
    msg = "mqs_begin: W^T W is singular";
    return GEMMA_HIP_EINVAL;
  }
  if (slot == 0) mqs_release_x();
  else {
    dfree(g_mqs.A);
    dfree(g_mqs.idx);
    dfree(g_mqs.Wt);
    dfree(g_mqs.Wi);
    g_mqs.haveA = false;
  }
  gemm_aux_init();
  const long ld = (n + 1) & ~1L;
  g_mqs.n = n;
  g_mqs.ni_total = ni_total;
  g_mqs.ld = ld;
  g_mqs.nvc = n_vc;
  g_mqs.c = c;
  g_mqs.slot = slot;
  g_mqs.last = nullptr;
  for (long &v : g_mqs.ns) v = 0;
  int rc;
  double **M = slot == 0 ? &g_mqs.K : &g_mqs.A;
  const size_t total = (size_t)n_vc * n * ld;
  if ((rc = dalloc(M, total, msg)) || (rc = dalloc(&g_mqs.idx, (size_t)n, msg)) || (rc = dalloc(&g_mqs.Wt, (size_t)c * ld, msg)) ||
      (rc = dalloc(&g_mqs.Wi, (size_t)c * c, msg)) || (!g_mqs.cnt && (rc = dalloc(&g_mqs.cnt, (size_t)MQS_VCMAX + 1, msg)))) {
    if (slot == 0) mqs_release_x();
    else dfree(g_mqs.A);
    return rc;
  }
  MQCHK(hipMemset(*M, 0, total * 8));
  std::vector<double> Wt((size_t)c * ld, 0.0);
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a) Wt[(size_t)a * ld + i] = W[i * c + a];
  MQCHK(hipMemcpy(g_mqs.idx, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  MQCHK(hipMemcpy(g_mqs.Wt, Wt.data(), Wt.size() * 8, hipMemcpyHostToDevice));
  MQCHK(hipMemcpy(g_mqs.Wi, WtW.data(), WtW.size() * 8, hipMemcpyHostToDevice));
  if (slot == 0) g_mqs.haveK = false;
  g_mqs.active = true;
  return GEMMA_HIP_OK;
}

int mqs_add_x(int geno_kind, const void *geno, long l, long ld_src, const int *cat, const double *weight, bool device, hipStream_t s,
              std::string &msg) {
  const long n = g_mqs.n, ld = g_mqs.ld;
  const int nvc = g_mqs.nvc;
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  int rc;
  if (l > g_mqs.cap) {
    MQCHK(hipDeviceSynchronize());
    free_block_buffers();
    if ((rc = dalloc(&g_mqs.X, (size_t)l * ld, msg)) || (rc = dalloc(&g_mqs.P, (size_t)l * ld, msg)) ||
        (rc = dalloc(&g_mqs.var, (size_t)l, msg)) || (rc = dalloc(&g_mqs.w_d, (size_t)l, msg)) ||
        (rc = dalloc(&g_mqs.pos, (size_t)l, msg)) || (rc = dalloc(&g_mqs.cat_d, (size_t)l, msg))) {
      free_block_buffers();
      return rc;
    }
    g_mqs.cap = l;
  }
  const void *src = geno;
  const int *cat_d = cat;
  const double *w_d = weight;
  if (!device) {
    for (long t = 0; t < l; ++t)
      if (cat[t] >= nvc) {
        msg = "mqs_add: category " + std::to_string(cat[t]) + " of SNP " + std::to_string(t) + " with n_vc = " + std::to_string(nvc);
        return GEMMA_HIP_EINVAL;
      }
    const size_t row = plink ? (size_t)((g_mqs.ni_total + 3) / 4) : (size_t)g_mqs.ni_total * 8, pitch = (size_t)ld_src * (plink ? 1 : 8);
    const size_t bytes = (size_t)l * row;
    if (bytes > g_mqs.stage_cap) {
      MQCHK(hipDeviceSynchronize());
      if (g_mqs.stage) (void)hipFree(g_mqs.stage);
      g_mqs.stage = nullptr;
      g_mqs.stage_cap = 0;
      if (hipMalloc(&g_mqs.stage, bytes) != hipSuccess) {
        (void)hipGetLastError();
        msg = "mqs_add: cannot allocate " + std::to_string(bytes) + " bytes of device memory";
        return GEMMA_HIP_ENOMEM;
      }
      g_mqs.stage_cap = bytes;
    }
    MQCHK(hipMemcpy2DAsync(g_mqs.stage, row, geno, pitch, row, (size_t)l, hipMemcpyHostToDevice, s));
    MQCHK(hipMemcpyAsync(g_mqs.cat_d, cat, (size_t)l * sizeof(int), hipMemcpyHostToDevice, s));
    if (weight) MQCHK(hipMemcpyAsync(g_mqs.w_d, weight, (size_t)l * 8, hipMemcpyHostToDevice, s));
    src = g_mqs.stage;
    ld_src = plink ? (long)row : g_mqs.ni_total;
    cat_d = g_mqs.cat_d;
    w_d = weight ? g_mqs.w_d : nullptr;
  }
  MqsIngest g;
  g.src = src;
  g.ld = ld_src;
  g.l = l;
  g.idx = g_mqs.idx;
  g.n = (int)n;
  g.c = g_mqs.c;
  g.Wt = g_mqs.Wt;
  g.Wi = g_mqs.Wi;
  g.X = g_mqs.X;
  g.ldx = ld;
  g.var = g_mqs.var;
  if (plink) hipLaunchKernelGGL(mqs_ingest_kernel<true>, dim3((unsigned)l), dim3(MQS_THREADS), 0, s, g);
  else hipLaunchKernelGGL(mqs_ingest_kernel<false>, dim3((unsigned)l), dim3(MQS_THREADS), 0, s, g);
  MQCHK(hipGetLastError());
  MQCHK(hipMemsetAsync(g_mqs.cnt, 0, (MQS_VCMAX + 1) * sizeof(int), s));
  hipLaunchKernelGGL(mqs_scan_kernel, dim3((unsigned)nvc), dim3(MQS_SCAN_THREADS), 0, s, cat_d, g_mqs.var, l, nvc, g_mqs.pos, g_mqs.cnt,
                     g_mqs.cnt + MQS_VCMAX);
  MQCHK(hipGetLastError());
  int cnt[MQS_VCMAX + 1];
  MQCHK(hipMemcpyAsync(cnt, g_mqs.cnt, sizeof cnt, hipMemcpyDeviceToHost, s));
  MQCHK(hipStreamSynchronize(s));
  if (cnt[MQS_VCMAX]) { // nothing was accumulated from this block
    msg = "mqs_add: a category index of the block is >= n_vc = " + std::to_string(nvc);
    return GEMMA_HIP_EINVAL;
  }
  hipLaunchKernelGGL(mqs_compact_kernel, dim3((unsigned)l), dim3(MQS_THREADS), 0, s, g_mqs.X, ld, l, cat_d, g_mqs.var, w_d, nvc,
                     g_mqs.pos, g_mqs.cnt, g_mqs.P);
  MQCHK(hipGetLastError());
  double *M = g_mqs.slot == 0 ? g_mqs.K : g_mqs.A;
  long base = 0;
  for (int k = 0; k < nvc; ++k) {
    if (cnt[k] > 0) {
      // K_c (upper tiles) += X_c^T X_c: the panel rows of category c as [k = snp][m = individual] -> ('T', 'N')
      const double *Pc = g_mqs.P + (size_t)base * ld;
      MQCHK(launch_dgemm('T', 'N', n, n, (long)cnt[k], 1.0, Pc, ld, Pc, ld, 1.0, M + (size_t)k * n * ld, ld, true, false, s));
      g_mqs.ns[k] += cnt[k];
    }
    base += cnt[k];
  }
  g_mqs.last = s;
  return GEMMA_HIP_OK;
}

namespace {

const hipStream_t S0 = nullptr;

int row_stats(const double *M, long n, long ld, double *rs, double *dg, hipStream_t s, std::string &msg) {
  hipLaunchKernelGGL(mqs_rowstat_kernel, dim3((unsigned)((n + 3) / 4)), dim3(MQS_THREADS), 0, s, M, n, ld, rs, dg);
  MQCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

// PlinkKin's division by ns_c and mirror, then CenterMatrix and ScaleMatrix; work: 2 ld + 2 doubles
int finish_matrix(double *M, long n, long ld, long ns, double *work, std::string &msg) {
  int rc;
  double *rs = work, *dg = work + ld, *tot = work + 2 * ld;
  const unsigned nb = (unsigned)((n + 31) / 32), ny = (unsigned)std::min<long>(n, 65535), nx = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(mqs_symm_scale_kernel, dim3(nb, nb), dim3(32, 8), 0, S0, M, n, ld, ns > 0 ? (double)ns : 1.0);
  MQCHK(hipGetLastError());
  if ((rc = row_stats(M, n, ld, rs, dg, S0, msg))) return rc;
  hipLaunchKernelGGL(mqs_total_kernel, dim3(1), dim3(1024), 0, S0, rs, n, tot);
  hipLaunchKernelGGL(mqs_center_kernel, dim3(nx, ny), dim3(256), 0, S0, M, n, ld, rs, tot);
  MQCHK(hipGetLastError());
  if ((rc = row_stats(M, n, ld, rs, dg, S0, msg))) return rc;
  hipLaunchKernelGGL(mqs_total_kernel, dim3(1), dim3(1024), 0, S0, dg, n, tot + 1);
  hipLaunchKernelGGL(mqs_scale_kernel, dim3(nx, ny), dim3(256), 0, S0, M, n, ld, tot + 1);
  MQCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

} // namespace

int mqs_S_x(long n, int n_vc, const double *A, const double *K, long ld, int c, double *S, hipStream_t s, std::string &msg) {
  const bool same = (A == K);
  const long lv = (n + 1) & ~1L; // stride of the per-matrix vectors: even, so that two-double loads stay aligned
  const bool vec = (ld % 2) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0;
  double *work = nullptr;
  int rc = dalloc(&work, (size_t)4 * n_vc * lv + 3 * (size_t)lv, msg);
  if (rc) return rc;
  struct Free {
    double *&p;
    ~Free() { dfree(p); }
  } free_work{work};
  double *sK = work, *dK = sK + (size_t)n_vc * lv, *sA = dK + (size_t)n_vc * lv, *dA = sA + (size_t)n_vc * lv, *huv = dA + (size_t)n_vc * lv;
  for (int j = 0; j < n_vc; ++j) {
    if ((rc = row_stats(K + (size_t)j * n * ld, n, ld, sK + (size_t)j * lv, dK + (size_t)j * lv, s, msg))) return rc;
    if (!same && (rc = row_stats(A + (size_t)j * n * ld, n, ld, sA + (size_t)j * lv, dA + (size_t)j * lv, s, msg))) return rc;
  }
  std::vector<double> hs((size_t)4 * n_vc * lv), hp((size_t)3 * n);
  MQCHK(hipMemcpyAsync(hs.data(), work, hs.size() * 8, hipMemcpyDeviceToHost, s));
  MQCHK(hipStreamSynchronize(s));
  const double *h_sK = hs.data(), *h_dK = h_sK + (size_t)n_vc * lv;
  const double *h_sA = same ? h_sK : h_dK + (size_t)n_vc * lv, *h_dA = same ? h_dK : h_sA + (size_t)n_vc * lv;
  const double *d_sA = same ? sK : sA;
  for (int i = 0; i < n_vc; ++i)
    for (int j = same ? i : 0; j < n_vc; ++j) {
      const double *Ai = A + (size_t)i * n * ld, *Kj = K + (size_t)j * n * ld;
      if (vec)
        hipLaunchKernelGGL(mqs_pair_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(MQS_THREADS), 0, s, Ai, Kj, n, ld,
                           d_sA + (size_t)i * lv, sK + (size_t)j * lv, huv);
      else
        hipLaunchKernelGGL(mqs_pair_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(MQS_THREADS), 0, s, Ai, Kj, n, ld,
                           d_sA + (size_t)i * lv, sK + (size_t)j * lv, huv);
      MQCHK(hipGetLastError());
      MQCHK(hipMemcpyAsync(hp.data(), huv, hp.size() * 8, hipMemcpyDeviceToHost, s));
      MQCHK(hipStreamSynchronize(s));
      double sv, vv;
      finish_pair(n, c, h_sA + (size_t)i * lv, h_dA + (size_t)i * lv, h_sK + (size_t)j * lv, h_dK + (size_t)j * lv, hp.data(),
                  hp.data() + n, hp.data() + 2 * n, &sv, &vv);
      S[i * n_vc + j] = sv;
      S[(n_vc + i) * n_vc + j] = vv;
      if (same && j != i) { // the pair (j, i) is the transpose: h the same, u and v exchanged
        S[j * n_vc + i] = sv;
        S[(n_vc + j) * n_vc + i] = vv;
      }
    }
  return GEMMA_HIP_OK;
}

int mqs_end_x(double *S, double *ns, std::string &msg) {
  const long n = g_mqs.n, ld = g_mqs.ld;
  const int nvc = g_mqs.nvc;
  int rc;
  if (g_mqs.last) MQCHK(hipStreamSynchronize(g_mqs.last));
  g_mqs.active = false;
  free_block_buffers();
  double *work = nullptr;
  if ((rc = dalloc(&work, (size_t)2 * ld + 2, msg))) return rc;
  double *M = g_mqs.slot == 0 ? g_mqs.K : g_mqs.A;
  for (int k = 0; k < nvc && !rc; ++k) rc = finish_matrix(M + (size_t)k * n * ld, n, ld, g_mqs.ns[k], work, msg);
  hipError_t e = hipStreamSynchronize(S0);
  dfree(work);
  if (rc) return rc;
  if (e != hipSuccess) return herr(e, "mqs_end", msg);
  if (g_mqs.slot == 0) g_mqs.haveK = true;
  else g_mqs.haveA = true;
  if (ns)
    for (int k = 0; k < nvc; ++k) ns[k] = (double)g_mqs.ns[k];
  if (!S) return GEMMA_HIP_OK;
  return mqs_S_x(n, nvc, g_mqs.haveA ? g_mqs.A : g_mqs.K, g_mqs.K, ld, g_mqs.c, S, S0, msg);
}

int mqs_get_x(int slot, int i_vc, double *out, std::string &msg) {
  if (g_mqs.active || !g_mqs.haveK || i_vc < 0 || i_vc >= g_mqs.nvc || (slot != 0 && slot != 1)) {
    msg = "mqs_get: slot " + std::to_string(slot) + ", matrix " + std::to_string(i_vc) + " of a finished session with n_vc = " +
          std::to_string(g_mqs.nvc);
    return GEMMA_HIP_EINVAL;
  }
  const double *M = (slot == 1 && g_mqs.haveA) ? g_mqs.A : g_mqs.K;
  const long n = g_mqs.n, ld = g_mqs.ld;
  MQCHK(hipMemcpy2D(out, (size_t)n * 8, M + (size_t)i_vc * n * ld, (size_t)ld * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

} // namespace gemma_hip

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
#include "tu_common.h"
#include "host_linalg.h"
#include "dgemm.h"
#include "mqs.hip.h"
#include "ci.hip.h"
#include "mqs_tu.h"

namespace gemma_hip {

namespace {

struct MqsState {
  bool active = false, haveK = false, haveA = false;
  long n = 0, ni_total = 0, ld = 0, cap = 0;
  int nvc = 0, c = 0, slot = 0;
  DevBuf K, A;                // n_vc matrices of n x ld doubles each; !haveA: A is K
  DevBuf idx;                 // ints
  DevBuf Wt, Wi;              // doubles
  DevBuf X, P, var, w_d;      // doubles
  DevBuf pos, cnt, cat_d;     // ints; cnt: n_vc counts, then the bad-category flag
  DevBuf stage;               // host blocks land here
  long ns[MQS_VCMAX] = {};
  hipStream_t last = nullptr;
} g_mqs;

// the buffers of one block, sized for g_mqs.cap SNPs
void free_block_buffers() {
  g_mqs.X.release(); g_mqs.P.release(); g_mqs.var.release(); g_mqs.w_d.release(); g_mqs.pos.release(); g_mqs.cat_d.release();
  g_mqs.stage.release();
  g_mqs.cap = 0;
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
  g_mqs.K.release(); g_mqs.A.release(); g_mqs.idx.release(); g_mqs.Wt.release(); g_mqs.Wi.release(); g_mqs.cnt.release();
  g_mqs.active = g_mqs.haveK = g_mqs.haveA = false;
  g_mqs.n = g_mqs.ni_total = g_mqs.ld = 0;
  g_mqs.nvc = g_mqs.c = 0;
}

void mqs_tu_shutdown() {
  mqs_release_x();
  ci_release_x();
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
  const bool carry = slot == 2; // slot 2: slot 1 with A starting from the kept K instead of 0
  if (carry) slot = 1;
  if (slot == 1) {
    if (!g_mqs.haveK || g_mqs.active) {
      msg = std::string("mqs_begin: slot ") + (carry ? "2" : "1") + " fills A beside the K of a finished slot 0 session, and there is none";
      return GEMMA_HIP_EINVAL;
    }
    if (g_mqs.n != n || g_mqs.nvc != n_vc || g_mqs.ni_total != ni_total) {
      msg = std::string("mqs_begin: slot ") + (carry ? "2" : "1") + " with n = " + std::to_string(n) + ", n_vc = " + std::to_string(n_vc) + "; the kept K has n = " +
            std::to_string(g_mqs.n) + ", n_vc = " + std::to_string(g_mqs.nvc);
      return GEMMA_HIP_EINVAL;
    }
  }
  // (W^T W)^-1 on the host
  std::vector<double> WtW((size_t)c * c, 0.0);
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a)
      for (int e = 0; e < c; ++e) WtW[a * c + e] += W[i * c + a] * W[i * c + e];
  if (small_inverse(WtW, c) != SMALL_INVERSE_OK) { // a NaN pivot is refused too
    msg = "mqs_begin: W^T W is singular";
    return GEMMA_HIP_EINVAL;
  }
  if (slot == 0) mqs_release_x();
  else {
    g_mqs.A.release(); g_mqs.idx.release(); g_mqs.Wt.release(); g_mqs.Wi.release();
    g_mqs.haveA = false;
  }
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
  DevBuf &M = slot == 0 ? g_mqs.K : g_mqs.A;
  const size_t total = (size_t)n_vc * n * ld;
  if ((rc = M.reserve(total * 8, "mqs", msg)) || (rc = g_mqs.idx.reserve((size_t)n * sizeof(int), "mqs", msg)) ||
      (rc = g_mqs.Wt.reserve((size_t)c * ld * 8, "mqs", msg)) || (rc = g_mqs.Wi.reserve((size_t)c * c * 8, "mqs", msg)) ||
      (rc = g_mqs.cnt.reserve((size_t)(MQS_VCMAX + 1) * sizeof(int), "mqs", msg))) {
    if (slot == 0) mqs_release_x();
    else g_mqs.A.release();
    return rc;
  }
  // The reference's second CalcS hands PlinkKin the A of the first one (the centred + scaled copy of K) and PlinkKin adds to what it
  // is given (src/gemma_io.cpp:3103, :3120, :3136: beta = 1, no set_zero): slot 2 reproduces that sum, slot 1 starts from 0.
  if (carry) TU_CHK(hipMemcpy(M.p, g_mqs.K.p, total * 8, hipMemcpyDeviceToDevice));
  else TU_CHK(hipMemset(M.p, 0, total * 8));
  std::vector<double> Wt((size_t)c * ld, 0.0);
  for (long i = 0; i < n; ++i)
    for (int a = 0; a < c; ++a) Wt[(size_t)a * ld + i] = W[i * c + a];
  TU_CHK(hipMemcpy(g_mqs.idx.p, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  TU_CHK(hipMemcpy(g_mqs.Wt.p, Wt.data(), Wt.size() * 8, hipMemcpyHostToDevice));
  TU_CHK(hipMemcpy(g_mqs.Wi.p, WtW.data(), WtW.size() * 8, hipMemcpyHostToDevice));
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
    TU_CHK(hipDeviceSynchronize());
    free_block_buffers();
    if ((rc = g_mqs.X.reserve((size_t)l * ld * 8, "mqs", msg)) || (rc = g_mqs.P.reserve((size_t)l * ld * 8, "mqs", msg)) ||
        (rc = g_mqs.var.reserve((size_t)l * 8, "mqs", msg)) || (rc = g_mqs.w_d.reserve((size_t)l * 8, "mqs", msg)) ||
        (rc = g_mqs.pos.reserve((size_t)l * sizeof(int), "mqs", msg)) || (rc = g_mqs.cat_d.reserve((size_t)l * sizeof(int), "mqs", msg))) {
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
    if ((size_t)l * row > g_mqs.stage.cap) TU_CHK(hipDeviceSynchronize()); // an earlier add may still read the buffer that grows
    if ((rc = stage_rows(g_mqs.stage, geno, (size_t)l, row, pitch, plink ? 1 : 8, s, "mqs_add", msg, src, ld_src))) return rc;
    TU_CHK(hipMemcpyAsync(g_mqs.cat_d.p, cat, (size_t)l * sizeof(int), hipMemcpyHostToDevice, s));
    if (weight) TU_CHK(hipMemcpyAsync(g_mqs.w_d.p, weight, (size_t)l * 8, hipMemcpyHostToDevice, s));
    cat_d = g_mqs.cat_d.as<int>();
    w_d = weight ? g_mqs.w_d.as<double>() : nullptr;
  }
  double *const X = g_mqs.X.as<double>(), *const P = g_mqs.P.as<double>(), *const var = g_mqs.var.as<double>();
  int *const pos = g_mqs.pos.as<int>(), *const cnt_d = g_mqs.cnt.as<int>();
  MqsIngest g;
  g.src = src;
  g.ld = ld_src;
  g.l = l;
  g.idx = g_mqs.idx.as<int>();
  g.n = (int)n;
  g.c = g_mqs.c;
  g.Wt = g_mqs.Wt.as<double>();
  g.Wi = g_mqs.Wi.as<double>();
  g.X = X;
  g.ldx = ld;
  g.var = var;
  if (plink) hipLaunchKernelGGL(mqs_ingest_kernel<true>, dim3((unsigned)l), dim3(MQS_THREADS), 0, s, g);
  else hipLaunchKernelGGL(mqs_ingest_kernel<false>, dim3((unsigned)l), dim3(MQS_THREADS), 0, s, g);
  TU_CHK(hipGetLastError());
  TU_CHK(hipMemsetAsync(cnt_d, 0, (MQS_VCMAX + 1) * sizeof(int), s));
  hipLaunchKernelGGL(mqs_scan_kernel, dim3((unsigned)nvc), dim3(MQS_SCAN_THREADS), 0, s, cat_d, var, l, nvc, pos, cnt_d, cnt_d + MQS_VCMAX);
  TU_CHK(hipGetLastError());
  int cnt[MQS_VCMAX + 1];
  TU_CHK(hipMemcpyAsync(cnt, cnt_d, sizeof cnt, hipMemcpyDeviceToHost, s));
  TU_CHK(hipStreamSynchronize(s));
  if (cnt[MQS_VCMAX]) { // nothing was accumulated from this block
    msg = "mqs_add: a category index of the block is >= n_vc = " + std::to_string(nvc);
    return GEMMA_HIP_EINVAL;
  }
  hipLaunchKernelGGL(mqs_compact_kernel, dim3((unsigned)l), dim3(MQS_THREADS), 0, s, X, ld, l, cat_d, var, w_d, nvc, pos, cnt_d, P);
  TU_CHK(hipGetLastError());
  double *M = (g_mqs.slot == 0 ? g_mqs.K : g_mqs.A).as<double>();
  long base = 0;
  for (int k = 0; k < nvc; ++k) {
    if (cnt[k] > 0) {
      // K_c (upper tiles) += X_c^T X_c: the panel rows of category c as [k = snp][m = individual] -> ('T', 'N')
      const double *Pc = P + (size_t)base * ld;
      TU_CHK(launch_dgemm('T', 'N', n, n, (long)cnt[k], 1.0, Pc, ld, Pc, ld, 1.0, M + (size_t)k * n * ld, ld, true, false, s));
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
  TU_CHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

// PlinkKin's division by ns_c and mirror, then CenterMatrix and ScaleMatrix; work: 2 ld + 2 doubles
int finish_matrix(double *M, long n, long ld, long ns, double *work, std::string &msg) {
  int rc;
  double *rs = work, *dg = work + ld, *tot = work + 2 * ld;
  const unsigned nb = (unsigned)((n + 31) / 32), ny = (unsigned)std::min<long>(n, 65535), nx = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(mqs_symm_scale_kernel, dim3(nb, nb), dim3(32, 8), 0, S0, M, n, ld, ns > 0 ? (double)ns : 1.0);
  TU_CHK(hipGetLastError());
  if ((rc = row_stats(M, n, ld, rs, dg, S0, msg))) return rc;
  hipLaunchKernelGGL(mqs_total_kernel, dim3(1), dim3(1024), 0, S0, rs, n, tot);
  hipLaunchKernelGGL(mqs_center_kernel, dim3(nx, ny), dim3(256), 0, S0, M, n, ld, rs, tot);
  TU_CHK(hipGetLastError());
  if ((rc = row_stats(M, n, ld, rs, dg, S0, msg))) return rc;
  hipLaunchKernelGGL(mqs_total_kernel, dim3(1), dim3(1024), 0, S0, dg, n, tot + 1);
  hipLaunchKernelGGL(mqs_scale_kernel, dim3(nx, ny), dim3(256), 0, S0, M, n, ld, tot + 1);
  TU_CHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

} // namespace

int mqs_S_x(long n, int n_vc, const double *A, const double *K, long ld, int c, double *S, hipStream_t s, std::string &msg) {
  const bool same = (A == K);
  const long lv = (n + 1) & ~1L; // stride of the per-matrix vectors: even, so that two-double loads stay aligned
  const bool vec = (ld % 2) == 0 && (reinterpret_cast<uintptr_t>(A) & 15) == 0 && (reinterpret_cast<uintptr_t>(K) & 15) == 0;
  ScopedBuf wb;
  int rc = wb.reserve(((size_t)4 * n_vc * lv + 3 * (size_t)lv) * 8, "mqs", msg);
  if (rc) return rc;
  double *work = wb.as<double>();
  double *sK = work, *dK = sK + (size_t)n_vc * lv, *sA = dK + (size_t)n_vc * lv, *dA = sA + (size_t)n_vc * lv, *huv = dA + (size_t)n_vc * lv;
  for (int j = 0; j < n_vc; ++j) {
    if ((rc = row_stats(K + (size_t)j * n * ld, n, ld, sK + (size_t)j * lv, dK + (size_t)j * lv, s, msg))) return rc;
    if (!same && (rc = row_stats(A + (size_t)j * n * ld, n, ld, sA + (size_t)j * lv, dA + (size_t)j * lv, s, msg))) return rc;
  }
  std::vector<double> hs((size_t)4 * n_vc * lv), hp((size_t)3 * n);
  TU_CHK(hipMemcpyAsync(hs.data(), work, hs.size() * 8, hipMemcpyDeviceToHost, s));
  TU_CHK(hipStreamSynchronize(s));
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
      TU_CHK(hipGetLastError());
      TU_CHK(hipMemcpyAsync(hp.data(), huv, hp.size() * 8, hipMemcpyDeviceToHost, s));
      TU_CHK(hipStreamSynchronize(s));
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
  if (g_mqs.last) TU_CHK(hipStreamSynchronize(g_mqs.last));
  g_mqs.active = false;
  free_block_buffers();
  ScopedBuf wb;
  if ((rc = wb.reserve(((size_t)2 * ld + 2) * 8, "mqs", msg))) return rc;
  double *work = wb.as<double>();
  double *M = (g_mqs.slot == 0 ? g_mqs.K : g_mqs.A).as<double>();
  for (int k = 0; k < nvc && !rc; ++k) rc = finish_matrix(M + (size_t)k * n * ld, n, ld, g_mqs.ns[k], work, msg);
  hipError_t e = hipStreamSynchronize(S0);
  wb.release();
  if (rc) return rc;
  if (e != hipSuccess) return hip_err(e, "mqs_end", msg);
  if (g_mqs.slot == 0) g_mqs.haveK = true;
  else g_mqs.haveA = true;
  if (ns)
    for (int k = 0; k < nvc; ++k) ns[k] = (double)g_mqs.ns[k];
  if (!S) return GEMMA_HIP_OK;
  return mqs_S_x(n, nvc, (g_mqs.haveA ? g_mqs.A : g_mqs.K).as<double>(), g_mqs.K.as<double>(), ld, g_mqs.c, S, S0, msg);
}

int mqs_get_x(int slot, int i_vc, double *out, std::string &msg) {
  if (g_mqs.active || !g_mqs.haveK || i_vc < 0 || i_vc >= g_mqs.nvc || (slot != 0 && slot != 1)) {
    msg = "mqs_get: slot " + std::to_string(slot) + ", matrix " + std::to_string(i_vc) + " of a finished session with n_vc = " +
          std::to_string(g_mqs.nvc);
    return GEMMA_HIP_EINVAL;
  }
  const double *M = ((slot == 1 && g_mqs.haveA) ? g_mqs.A : g_mqs.K).as<double>();
  const long n = g_mqs.n, ld = g_mqs.ld;
  TU_CHK(hipMemcpy2D(out, (size_t)n * 8, M + (size_t)i_vc * n * ld, (size_t)ld * 8, (size_t)n * 8, (size_t)n, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

// ------------------------------------------------------------------------------------------------ -ci 1 / -ci 2
// The two genotype passes of the MQS confidence intervals (kernels: ci.hip.h), in place of
//   PlinkXwz / BimbamXwz        src/vc.cpp:2314-2437, :2225-2312   (pass 1: one seekg, one daxpy per SNP there)
//   PlinkXtXwz / BimbamXtXwz    src/vc.cpp:2568-2688, :2480-2566   (pass 2: n_vc ddots per SNP there)
namespace {

struct CiState {
  int pass = 0;               // 0: none, 1: pass 1 open, 2: XWz finished, pass 2 open
  long n = 0, ni_total = 0, words = 0, ldx = 0;
  int nvc = 0;
  DevBuf idx, amask;          // ints, 2-bit group mask
  DevBuf acc;                 // n x 16: Xz | XWz over the analysed individuals
  DevBuf Bf;                  // pass 2, 2-bit rows: XWz scattered to all individuals, 16 columns, zero rows between
  DevBuf Bc;                  // pass 2, fp64 rows: XWz over the analysed individuals, 16 columns
  DevBuf st, tab, bm, cat_d, z_d, w_d, flags, part, X, P, out, stage;
} g_ci;

// a buffer earlier asynchronous work may still read grows only after that work is done
int ci_grow(DevBuf &b, size_t bytes, std::string &msg) {
  if (bytes <= b.cap) return GEMMA_HIP_OK;
  TU_CHK(hipDeviceSynchronize());
  return b.reserve(bytes, "ci", msg);
}

int ci_stage(int geno_kind, const void *geno, long l, long &ld, hipStream_t s, const void *&src, std::string &msg) {
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  const size_t row = plink ? (size_t)((g_ci.ni_total + 3) / 4) : (size_t)g_ci.ni_total * 8, pitch = (size_t)ld * (plink ? 1 : 8);
  if ((size_t)l * row > g_ci.stage.cap) TU_CHK(hipDeviceSynchronize());
  return stage_rows(g_ci.stage, geno, (size_t)l, row, pitch, plink ? 1 : 8, s, "ci", msg, src, ld);
}

// the per-SNP moments of a block (and, for fp64 rows, the centred rows in g_ci.X)
int ci_stats(bool plink, const void *src, long l, long ld, hipStream_t s, std::string &msg) {
  int rc;
  if ((rc = ci_grow(g_ci.st, (size_t)l * sizeof(double2), msg))) return rc;
  double2 *st = g_ci.st.as<double2>();
  if (plink) {
    const unsigned char *G = reinterpret_cast<const unsigned char *>(src);
    const bool al = ((reinterpret_cast<uintptr_t>(src) & 3) == 0) && ((ld & 3) == 0);
    const unsigned rows4 = (unsigned)((l + 3) / 4);
    if (al)
      hipLaunchKernelGGL(ci_stats_plink_kernel<true>, dim3(rows4), dim3(256), 0, s, G, ld, l, g_ci.amask.as<unsigned>(), g_ci.ni_total,
                         g_ci.words, (int)g_ci.n, st);
    else
      hipLaunchKernelGGL(ci_stats_plink_kernel<false>, dim3(rows4), dim3(256), 0, s, G, ld, l, g_ci.amask.as<unsigned>(), g_ci.ni_total,
                         g_ci.words, (int)g_ci.n, st);
  } else {
    if ((rc = ci_grow(g_ci.X, (size_t)l * g_ci.ldx * 8, msg))) return rc;
    hipLaunchKernelGGL(ci_ingest_f64_kernel, dim3((unsigned)l), dim3(256), 0, s, reinterpret_cast<const double *>(src), ld, l,
                       g_ci.idx.as<int>(), (int)g_ci.n, g_ci.X.as<double>(), g_ci.ldx, st);
  }
  TU_CHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

} // namespace

void ci_release_x() {
  DevBuf *all[] = {&g_ci.idx, &g_ci.amask, &g_ci.acc, &g_ci.Bf, &g_ci.Bc, &g_ci.st, &g_ci.tab, &g_ci.bm, &g_ci.cat_d, &g_ci.z_d,
                   &g_ci.w_d, &g_ci.flags, &g_ci.part, &g_ci.X, &g_ci.P, &g_ci.out, &g_ci.stage};
  for (DevBuf *b : all) b->release();
  g_ci.pass = 0;
  g_ci.n = g_ci.ni_total = g_ci.words = g_ci.ldx = 0;
  g_ci.nvc = 0;
}

int ci_pass_x() { return g_ci.pass; }
long ci_ni_total_x() { return g_ci.ni_total; }

int ci_begin_x(long ni_total, const int *indicator, int n_vc, std::string &msg) {
  std::vector<int> idx;
  for (long i = 0; i < ni_total; ++i)
    if (!indicator || indicator[i] != 0) idx.push_back((int)i);
  const long n = (long)idx.size();
  if (n < 1) {
    msg = "ci_begin: no analysed individual";
    return GEMMA_HIP_EINVAL;
  }
  TU_CHK(hipDeviceSynchronize());
  ci_release_x();
  const long words = (ni_total + 15) / 16;
  std::vector<unsigned> am((size_t)words, 0u);
  for (int p : idx) am[(size_t)(p >> 4)] |= 1u << (2 * (p & 15));
  int rc;
  if ((rc = g_ci.idx.reserve((size_t)n * sizeof(int), "ci", msg)) || (rc = g_ci.amask.reserve((size_t)words * sizeof(unsigned), "ci", msg)) ||
      (rc = g_ci.acc.reserve((size_t)n * CI_COLS * 8, "ci", msg)) || (rc = g_ci.flags.reserve(2 * sizeof(int), "ci", msg))) {
    ci_release_x();
    return rc;
  }
  TU_CHK(hipMemcpy(g_ci.idx.p, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  TU_CHK(hipMemcpy(g_ci.amask.p, am.data(), (size_t)words * sizeof(unsigned), hipMemcpyHostToDevice));
  TU_CHK(hipMemset(g_ci.acc.p, 0, (size_t)n * CI_COLS * 8));
  g_ci.n = n;
  g_ci.ni_total = ni_total;
  g_ci.words = words;
  g_ci.ldx = (n + 1) & ~1L;
  g_ci.nvc = n_vc;
  g_ci.pass = 1;
  return GEMMA_HIP_OK;
}

int ci_xwz_x(int geno_kind, const void *geno, long l, long ld, const int *cat, const double *z, const double *w, bool device,
             hipStream_t s, size_t *n_skipped, std::string &msg) {
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  const long n = g_ci.n, words = g_ci.words;
  const int nvc = g_ci.nvc;
  int rc;
  const void *src = geno;
  const int *cat_d = cat;
  const double *z_d = z, *w_d = w;
  if (!device) {
    for (long t = 0; t < l; ++t)
      if (cat[t] < 0 || cat[t] >= nvc) {
        msg = "ci_xwz: category " + std::to_string(cat[t]) + " of SNP " + std::to_string(t) + " with n_vc = " + std::to_string(nvc);
        return GEMMA_HIP_EINVAL;
      }
    if ((rc = ci_grow(g_ci.cat_d, (size_t)l * sizeof(int), msg)) || (rc = ci_grow(g_ci.z_d, (size_t)l * 8, msg)) ||
        (rc = ci_grow(g_ci.w_d, (size_t)l * 8, msg)) || (rc = ci_stage(geno_kind, geno, l, ld, s, src, msg)))
      return rc;
    TU_CHK(hipMemcpyAsync(g_ci.cat_d.p, cat, (size_t)l * sizeof(int), hipMemcpyHostToDevice, s));
    TU_CHK(hipMemcpyAsync(g_ci.z_d.p, z, (size_t)l * 8, hipMemcpyHostToDevice, s));
    if (w) TU_CHK(hipMemcpyAsync(g_ci.w_d.p, w, (size_t)l * 8, hipMemcpyHostToDevice, s));
    cat_d = g_ci.cat_d.as<int>();
    z_d = g_ci.z_d.as<double>();
    w_d = w ? g_ci.w_d.as<double>() : nullptr;
  }
  const int parts = ci_parts(l, words);
  const long ldp = words * 16;
  if ((rc = ci_grow(g_ci.bm, (size_t)l * CI_COLS * 8, msg)) || (plink && (rc = ci_grow(g_ci.tab, (size_t)l * sizeof(double4), msg))) ||
      (plink && (rc = ci_grow(g_ci.part, (size_t)parts * ldp * CI_COLS * 8, msg))) || (rc = ci_stats(plink, src, l, ld, s, msg)))
    return rc;
  int *flags = g_ci.flags.as<int>();
  TU_CHK(hipMemsetAsync(flags, 0, 2 * sizeof(int), s));
  const unsigned lb = (unsigned)((l + 255) / 256);
  if (plink)
    hipLaunchKernelGGL(ci_table_kernel<true>, dim3(lb), dim3(256), 0, s, g_ci.st.as<double2>(), cat_d, z_d, w_d, l, nvc,
                       g_ci.tab.as<double4>(), g_ci.bm.as<double>(), flags);
  else
    hipLaunchKernelGGL(ci_table_kernel<false>, dim3(lb), dim3(256), 0, s, g_ci.st.as<double2>(), cat_d, z_d, w_d, l, nvc,
                       (double4 *)nullptr, g_ci.bm.as<double>(), flags);
  TU_CHK(hipGetLastError());
  int fl[2];
  TU_CHK(hipMemcpyAsync(fl, flags, sizeof fl, hipMemcpyDeviceToHost, s));
  TU_CHK(hipStreamSynchronize(s));
  if (fl[1]) { // nothing of the block is accumulated
    msg = "ci_xwz: a category index of the block is outside 0 .. n_vc - 1 = " + std::to_string(nvc - 1);
    return GEMMA_HIP_EINVAL;
  }
  if (n_skipped) *n_skipped = (size_t)fl[0];
  double *acc = g_ci.acc.as<double>();
  if (plink) {
    const unsigned char *G = reinterpret_cast<const unsigned char *>(src);
    const bool al = ((reinterpret_cast<uintptr_t>(src) & 3) == 0) && ((ld & 3) == 0);
    const int rpp = (int)((l + parts - 1) / parts);
    const dim3 grid((unsigned)((words + 4 * CI_TILES - 1) / (4 * CI_TILES)), (unsigned)parts);
    if (al)
      hipLaunchKernelGGL(ci_xwz_plink_kernel<true>, grid, dim3(256), 0, s, G, ld, l, g_ci.amask.as<unsigned>(), g_ci.ni_total, words,
                         g_ci.tab.as<double4>(), g_ci.bm.as<double>(), rpp, g_ci.part.as<double>(), ldp);
    else
      hipLaunchKernelGGL(ci_xwz_plink_kernel<false>, grid, dim3(256), 0, s, G, ld, l, g_ci.amask.as<unsigned>(), g_ci.ni_total, words,
                         g_ci.tab.as<double4>(), g_ci.bm.as<double>(), rpp, g_ci.part.as<double>(), ldp);
    TU_CHK(hipGetLastError());
    hipLaunchKernelGGL(ci_combine_kernel, dim3((unsigned)((n * CI_COLS + 255) / 256)), dim3(256), 0, s, g_ci.part.as<double>(), ldp, parts,
                       g_ci.idx.as<int>(), n, acc);
    TU_CHK(hipGetLastError());
  } else {
    // acc (n x 16) += X^T (n x l) bm (l x 16): the centred rows as [k = snp][m = individual] -> ('T', 'N')
    TU_CHK(launch_dgemm('T', 'N', n, CI_COLS, l, 1.0, g_ci.X.as<double>(), g_ci.ldx, g_ci.bm.as<double>(), CI_COLS, 1.0, acc, CI_COLS,
                        false, false, s));
  }
  if (!device) TU_CHK(hipStreamSynchronize(s)); // the caller's rows and the staging buffers are free again
  return GEMMA_HIP_OK;
}

int ci_xwz_end_x(double *Xz, double *XWz, std::string &msg) {
  const long n = g_ci.n;
  const int nvc = g_ci.nvc;
  TU_CHK(hipDeviceSynchronize());
  std::vector<double> acc((size_t)n * CI_COLS);
  TU_CHK(hipMemcpy(acc.data(), g_ci.acc.p, acc.size() * 8, hipMemcpyDeviceToHost));
  std::vector<int> idx((size_t)n);
  TU_CHK(hipMemcpy(idx.data(), g_ci.idx.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
  const long rows = ((g_ci.words + CI_GROUP - 1) / CI_GROUP) * CI_GROUP * 16;
  std::vector<double> Bf((size_t)rows * CI_COLS, 0.0), Bc((size_t)n * CI_COLS, 0.0);
  for (long j = 0; j < n; ++j)
    for (int k = 0; k < nvc; ++k) {
      const double xz = acc[(size_t)j * CI_COLS + k], xwz = acc[(size_t)j * CI_COLS + nvc + k];
      if (Xz) Xz[j * nvc + k] = xz;
      if (XWz) XWz[j * nvc + k] = xwz;
      Bf[(size_t)idx[j] * CI_COLS + k] = xwz;
      Bc[(size_t)j * CI_COLS + k] = xwz;
    }
  int rc;
  if ((rc = g_ci.Bf.reserve(Bf.size() * 8, "ci", msg)) || (rc = g_ci.Bc.reserve(Bc.size() * 8, "ci", msg))) return rc;
  TU_CHK(hipMemcpy(g_ci.Bf.p, Bf.data(), Bf.size() * 8, hipMemcpyHostToDevice));
  TU_CHK(hipMemcpy(g_ci.Bc.p, Bc.data(), Bc.size() * 8, hipMemcpyHostToDevice));
  g_ci.part.release(); // pass 1 only
  g_ci.pass = 2;
  return GEMMA_HIP_OK;
}

int ci_xtxwz_x(int geno_kind, const void *geno, long l, long ld, double *out, bool device, hipStream_t s, std::string &msg) {
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  const long n = g_ci.n;
  const int nvc = g_ci.nvc;
  int rc;
  const void *src = geno;
  if (!device && (rc = ci_stage(geno_kind, geno, l, ld, s, src, msg))) return rc;
  double *out_d = out;
  if (!device) {
    if ((rc = ci_grow(g_ci.out, (size_t)l * nvc * 8, msg))) return rc;
    out_d = g_ci.out.as<double>();
  }
  if ((rc = ci_stats(plink, src, l, ld, s, msg))) return rc;
  if (plink) {
    const unsigned char *G = reinterpret_cast<const unsigned char *>(src);
    const bool al = ((reinterpret_cast<uintptr_t>(src) & 3) == 0) && ((ld & 3) == 0);
    const unsigned nb = (unsigned)((l + 15) / 16);
    if (al)
      hipLaunchKernelGGL(ci_xtxwz_plink_kernel<true>, dim3(nb), dim3(256), 0, s, G, ld, l, g_ci.ni_total, g_ci.words, g_ci.st.as<double2>(),
                         g_ci.Bf.as<double>(), nvc, out_d);
    else
      hipLaunchKernelGGL(ci_xtxwz_plink_kernel<false>, dim3(nb), dim3(256), 0, s, G, ld, l, g_ci.ni_total, g_ci.words, g_ci.st.as<double2>(),
                         g_ci.Bf.as<double>(), nvc, out_d);
    TU_CHK(hipGetLastError());
  } else {
    if ((rc = ci_grow(g_ci.P, (size_t)l * CI_COLS * 8, msg))) return rc;
    TU_CHK(launch_dgemm('N', 'N', l, CI_COLS, n, 1.0, g_ci.X.as<double>(), g_ci.ldx, g_ci.Bc.as<double>(), CI_COLS, 0.0, g_ci.P.as<double>(),
                        CI_COLS, false, false, s));
    hipLaunchKernelGGL(ci_scale_rows_kernel, dim3((unsigned)((l * nvc + 255) / 256)), dim3(256), 0, s, g_ci.P.as<double>(),
                       g_ci.st.as<double2>(), l, nvc, out_d);
    TU_CHK(hipGetLastError());
  }
  if (!device) {
    TU_CHK(hipMemcpyAsync(out, out_d, (size_t)l * nvc * 8, hipMemcpyDeviceToHost, s));
    TU_CHK(hipStreamSynchronize(s));
  }
  return GEMMA_HIP_OK;
}

} // namespace gemma_hip

// Null fits of a whole phenotype panel (gemma_hip_lmm_null_panel): the body of the single fit, null_model<M> of lmm_assoc.hip.h,
// run by ONE WAVEFRONT PER PHENOTYPE on the phenotype's row of the transposed panel (Yt: T x n).  The three kernel families are the
// ones gemma_hip_lmm_null dispatches over -- FixedC<0..4> in registers, GenericC with its tables in per-wave LDS, the wide form with
// dynamic LDS -- and the arithmetic of a phenotype is the single fit's, instruction for instruction: fit t equals the single fit of
// column t in every bit.  No wavefront reads what another wrote: a phenotype whose fit is NaN leaves its neighbours alone.
#pragma once
#include "lmm_assoc.hip.h"
#include "lmm_score_panel.hip.h"
#define GEMMA_HIP_KERNEL_BODIES // a unit that includes this file instantiates what it launches: lmm_null_panel.h leaves out its extern templates
#include "lmm_null_panel.h"

namespace gemma_hip {

template <int CP>
__global__ __launch_bounds__(64 * NP_WAVES) void lmm_null_panel_kernel(AssocArgs g, const double *__restrict__ Yt, int T,
                                                                      NullOut *__restrict__ out) {
  const int t = (int)blockIdx.x * NP_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (t >= T) return;
  null_model(g, FixedC<CP>(), CP, threadIdx.x & 63, Yt + (long)t * g.n, out + t);
}

__global__ __launch_bounds__(64 * NP_WAVES) void lmm_null_panel_generic_kernel(AssocArgs g, int cp, const double *__restrict__ Yt,
                                                                              int T, NullOut *__restrict__ out) {
  __shared__ double lds[NP_WAVES * GEN_LDS_PER_WAVE];
  const int wave = threadIdx.x >> 6;
  const int t = (int)blockIdx.x * NP_WAVES + wave;
  if (t >= T) return;
  GenericC m;
  m.cc = cp;
  m.L = lds + wave * GEN_LDS_PER_WAVE;
  null_model(g, m, cp, threadIdx.x & 63, Yt + (long)t * g.n, out + t);
}

// more than GEN_CMAX + 1 covariates: one wavefront per workgroup, tables in dynamic LDS (6 * gen_ni_for(cp) doubles)
__global__ __launch_bounds__(64) void lmm_null_panel_wide_kernel(AssocArgs g, int cp, const double *__restrict__ Yt, int T,
                                                                 NullOut *__restrict__ out) {
  extern __shared__ double wide_lds[];
  const int t = (int)blockIdx.x;
  if (t >= T) return;
  GenericC m;
  m.cc = cp;
  m.L = wide_lds;
  m.ni = gen_ni_for(cp);
  null_model(g, m, cp, threadIdx.x & 63, Yt + (long)t * g.n, out + t);
}

// out8 of gemma_hip_lmm_null from a fit, in the operations and the order of its host code (CalcPve, src/lmm.cpp:2197-2200; ve and
// vg, :2258-2259).  Every product, sum and quotient is rounded on its own: a fused a * b + c moves pve by an ulp.  The header's
// __dmul_rn / __dadd_rn are plain `*` and `+` once inlined, which the compiler may contract like any other; the product that feeds a
// sum goes through rounded(), an empty asm the contraction cannot see through.
__device__ __forceinline__ double rounded(double v) {
  asm volatile("" : "+v"(v));
  return v;
}
__global__ __launch_bounds__(256) void null_panel_derive_kernel(const NullOut *__restrict__ in, int T, double trace_G, double df,
                                                               NullFit8 *__restrict__ fit) {
  const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (t >= T) return;
  const NullOut h = in[t];
  NullFit8 o;
  o.l_mle_null = h.l_mle; o.logl_mle_H0 = h.logl_mle; o.l_remle_null = h.l_remle; o.logl_remle_H0 = h.logl_remle;
  const double arg = __ddiv_rn(-1.0, h.dev2_remle);
  double d1 = arg;
  if (arg < 0.001) d1 = fabs(arg);
  const double se = (d1 < 0.0) ? NAN : __dsqrt_rn(d1);
  const double tl = rounded(__dmul_rn(trace_G, h.l_remle)), tl1 = __dadd_rn(tl, 1.0);
  o.pve = __ddiv_rn(tl, tl1);
  o.pve_se = __dmul_rn(__ddiv_rn(trace_G, __dmul_rn(tl1, tl1)), se);
  o.ve_remle = __ddiv_rn(h.Pyy_remle, df);
  o.vg_remle = __dmul_rn(o.ve_remle, h.l_remle);
  fit[t] = o;
}

// Covariate effects at the REML fit (CalcLmmVgVeBeta, src/lmm.cpp:2210-2281): per phenotype, at its l_remle, W^T H W (upper
// triangle) and W^T H y with h_i = 1 / (l eval_i + 1), one pass over the individuals per covariate row; lane 0 factors by Cholesky,
// beta = (W^T H W)^-1 W^T H y, se_beta[a] = safe_sqrt(ve [(W^T H W)^-1]_aa) with ve = P_yy / (n - c).  A Gram matrix that is not
// positive definite (a pivot below SP_PIVOT_MIN of its diagonal element, or a non-finite lambda) leaves NaN in the phenotype's row.
// UtWt: c x n, Yt: T x n, beta / se_beta: T x c.  c <= NP_CMAX.
__global__ __launch_bounds__(64 * NP_WAVES) void null_panel_beta_kernel(int n, int c, int T, const double *__restrict__ eval,
                                                                       const double *__restrict__ UtWt, const double *__restrict__ Yt,
                                                                       const NullOut *__restrict__ fit, double *__restrict__ beta,
                                                                       double *__restrict__ se_beta) {
  __shared__ double Sm[NP_WAVES][NP_CMAX][NP_CMAX + 1]; // the Gram matrix, then L in its lower triangle; written and read by lane 0
  __shared__ double bm[NP_WAVES][NP_CMAX];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = (int)blockIdx.x * NP_WAVES + wave;
  if (t >= T) return;
  const double l = fit[t].l_remle;
  const double *__restrict__ y = Yt + (long)t * n;
  double(*S)[NP_CMAX + 1] = Sm[wave];
  double *bv = bm[wave];
  for (int a = 0; a < c; ++a) {
    const double *__restrict__ wa = UtWt + (long)a * n;
    double acc[NP_CMAX], ay = 0.0;
#pragma unroll
    for (int b = 0; b < NP_CMAX; ++b) acc[b] = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double u = wa[i] / (l * eval[i] + 1.0);
      ay += u * y[i];
#pragma unroll
      for (int b = 0; b < NP_CMAX; ++b)
        if (b >= a && b < c) acc[b] += u * UtWt[(long)b * n + i];
    }
    ay = wave_sum(ay);
    if (lane == 0) bv[a] = ay;
#pragma unroll
    for (int b = 0; b < NP_CMAX; ++b) {
      if (b >= a && b < c) {
        const double s = wave_sum(acc[b]);
        if (lane == 0) { S[a][b] = s; S[b][a] = s; }
      }
    }
  }
  if (lane != 0) return;
  double *bo = beta + (long)t * c, *so = se_beta + (long)t * c;
  bool good = true;
  for (int j = 0; j < c && good; ++j) {
    const double sjj = S[j][j];
    double d = sjj;
    for (int k = 0; k < j; ++k) d -= S[j][k] * S[j][k];
    if (!(d > SP_PIVOT_MIN * sjj) || !(d <= DBL_MAX)) { good = false; break; }
    const double ljj = sqrt(d);
    S[j][j] = ljj;
    for (int i = j + 1; i < c; ++i) {
      double e = S[i][j];
      for (int k = 0; k < j; ++k) e -= S[i][k] * S[j][k];
      S[i][j] = e / ljj;
    }
  }
  if (!good) {
    for (int a = 0; a < c; ++a) { bo[a] = NAN; so[a] = NAN; }
    return;
  }
  for (int a = 0; a < c; ++a) { // L z = W^T H y
    double z = bv[a];
    for (int k = 0; k < a; ++k) z -= S[a][k] * bv[k];
    bv[a] = z / S[a][a];
  }
  for (int a = c - 1; a >= 0; --a) { // L^T beta = z
    double z = bv[a];
    for (int k = a + 1; k < c; ++k) z -= S[k][a] * bv[k];
    bv[a] = z / S[a][a];
    bo[a] = bv[a];
  }
  const double ve = __ddiv_rn(fit[t].Pyy_remle, (double)(n - c));
  for (int a = 0; a < c; ++a) { // [(L L^T)^-1]_aa = |L^-1 e_a|^2: the forward solve starts at row a, z in the padding column
    double q = 0.0;
    for (int i = a; i < c; ++i) {
      double z = (i == a) ? 1.0 : 0.0;
      for (int k = a; k < i; ++k) z -= S[i][k] * S[k][NP_CMAX];
      z /= S[i][i];
      S[i][NP_CMAX] = z;
      q += z * z;
    }
    so[a] = safe_sqrt_dev(ve * q);
  }
}

} // namespace gemma_hip

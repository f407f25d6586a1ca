// Wald and likelihood-ratio statistics of a list of (SNP, phenotype) pairs (gemma_hip_lmm_score_panel_refine_*): the `-lmm 4` body
// of the per-SNP stage run by ONE WAVEFRONT PER PAIR on row `snp` of the block's U^T x and row `pheno` of the transposed panel
// (Yt: T x n), with that phenotype's l_mle_null and logl_mle_H0.  Every evaluation streams the two rows (no fixed-lambda table, no
// series: a scattered list has no table to share), which is the form the single-phenotype launch takes with
// GEMMA_HIP_ASSOC_GRID=0 -- record i equals row `snp` of that launch on column `pheno` in every bit.
// pair_body is a sibling of assoc_one_snp (lmm_assoc.hip.h), not a factor of it: handing assoc_one_snp's body its x, y, nulls and
// slot as arguments moved the register allocation of every lmm_assoc kernel (scripts/device_text_digest.py --per-kernel), and
// those kernels stay byte for byte what they were.  wald_score, logdet_iw_of, calc_lambda, wald_score_from and the tails -- all the
// arithmetic -- are the shared code.  A failed lambda search follows the BIMBAM rule: a pair has no previous SNP to carry beta and
// se from.  A pair with snp >= g.l or pheno >= T gets an all-NaN record and reads nothing.  No wavefront reads what another wrote.
#pragma once
#include "lmm_assoc.hip.h"
#define GEMMA_HIP_KERNEL_BODIES // a unit that includes this file instantiates what it launches: lmm_pair.h leaves out its extern templates
#include "lmm_pair.h"

namespace gemma_hip {

// a_mode 4 of assoc_one_snp with plink_nan_rule 0, in its order: the score test at the null lambda ("3 is before 1",
// src/lmm.cpp:1540-1543), REML + Wald, ML + LRT
template <class M>
__device__ __forceinline__ void pair_body(const AssocArgs &g, const M &model, const double *x, const double *y, double l_mle_null,
                                          double logl_mle_H0, SumStat *slot, int lane) {
  SnpCtx<M> cx;
  cx.g = &g;
  cx.x = x;
  cx.y = y;
  cx.lane = lane;
  cx.m = model;
  cx.logdet_iw = 0.0;
  cx.trow = nullptr;
  cx.cslots = nullptr;
  double lambda_mle = 0.0, lambda_remle = 0.0, beta = 0.0, se = 0.0, p_wald = 0.0;
  double p_lrt = 0.0, p_score = 0.0, logl_H1 = 0.0;
  wald_score<M, true>(cx, l_mle_null, beta, se, p_score);
  cx.logdet_iw = logdet_iw_of(cx);
  Agg at_remle;
  calc_lambda<M, true>(cx, lambda_remle, logl_H1, at_remle);
  if (isnan(logl_H1)) { // failed search: CalcRLWald(NaN) (src/lmm.cpp:1548) -> NaN statistics
    beta = NAN; se = NAN; p_wald = NAN;
  } else {
    wald_score_from<M, false>(cx, at_remle, beta, se, p_wald);
  }
  Agg at_mle;
  calc_lambda<M, false>(cx, lambda_mle, logl_H1, at_mle);
  p_lrt = chisq_Q1_dev(2.0 * (logl_H1 - logl_mle_H0));
  if (isnan(logl_H1)) p_lrt = NAN;
  if (lane == 0) {
    SumStat o;
    o.beta = beta; o.se = se; o.lambda_remle = lambda_remle; o.lambda_mle = lambda_mle;
    o.p_wald = p_wald; o.p_lrt = p_lrt; o.p_score = p_score; o.logl_H1 = logl_H1;
    *slot = o;
  }
}

template <class M>
__device__ __forceinline__ void pair_one(const AssocArgs &g, const PairArgs &p, const M &model, long i, int lane) {
  const unsigned int snp = __builtin_amdgcn_readfirstlane(p.pairs[i].snp);
  const unsigned int ph = __builtin_amdgcn_readfirstlane(p.pairs[i].pheno);
  SumStat *slot = g.out + i;
  if ((long)snp >= g.l || ph >= (unsigned int)p.T) {
    if (lane == 0) {
      SumStat o;
      o.beta = NAN; o.se = NAN; o.lambda_remle = NAN; o.lambda_mle = NAN;
      o.p_wald = NAN; o.p_lrt = NAN; o.p_score = NAN; o.logl_H1 = NAN;
      *slot = o;
    }
    return;
  }
  pair_body(g, model, g.UtX + (long)snp * g.ld, p.Yt + (long)ph * g.n, uniform(p.l_mle_null[ph]), uniform(p.logl_mle_H0[ph]), slot,
            lane);
}

template <int C, int UNR, int WPS>
__global__ __launch_bounds__(64 * PR_WAVES, WPS) void lmm_pair_kernel(AssocArgs g, PairArgs p) {
  const long i = (long)blockIdx.x * PR_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (i >= p.m) return;
  pair_one(g, p, FixedC<C, UNR>(), i, threadIdx.x & 63);
}

__global__ __launch_bounds__(64 * PR_WAVES) void lmm_pair_generic_kernel(AssocArgs g, int c, PairArgs p) {
  __shared__ double lds[PR_WAVES * GEN_LDS_PER_WAVE];
  const int wave = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * PR_WAVES + wave;
  if (i >= p.m) return;
  GenericC m;
  m.cc = c;
  m.L = lds + wave * GEN_LDS_PER_WAVE;
  pair_one(g, p, m, i, threadIdx.x & 63);
}

} // namespace gemma_hip

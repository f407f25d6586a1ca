// The two-trait null fit of one pair of a panel (gemma_hip_mvlmm_null_pairs): the argument struct, the layout of a pair's raw result,
// the body one wavefront runs and the step that turns the raw result into a gemma_mvpair_fit.  Like mvlmm.hip.h the source also
// runs on one CPU "lane" (tests/host/mvpair_harness.cpp).
#pragma once
#include "mvlmm.hip.h"

namespace gemma_hip {

constexpr int MV_PAIR_CMAX = 6; // covariates of the fixed two-trait instances
// one pair's raw result: MvNullArgs::out of a (2, c) fit, then the MvNullSe block of it
constexpr int mv_pair_out_doubles(int c) { return 2 * (2 * 4 + 2 * c + 1); }
constexpr int mv_pair_raw_doubles(int c) { return mv_pair_out_doubles(c) + 2 * mv_null_se_doubles(2, c); }

struct MvPairArgs {
  int n, c;             // individuals, covariates (1..MV_PAIR_CMAX)
  long m;               // pairs of this launch
  const double *eval;   // n
  const double *Wt;     // c x n
  const double *Yp;     // m x 2 x n: rows i and j of U^T Y transposed, pair by pair (mvpair_gather_kernel)
  const int *pairs;     // 2 m: (i, j)
  const double *start;  // T x 8, gemma_null_fit per trait: [6] vg_remle, [7] ve_remle -- MphInitial's diagonals (:2780-2797)
  int em_iter, nr_iter;
  double em_prec, nr_prec;
  double *raw;          // m x mv_pair_raw_doubles(c)
};

// mirror of gemma_mvpair_block / gemma_mvpair_fit (include/gemma_hip.h; sizes asserted where both are visible)
struct MvPairBlock {
  double Vg[3], Ve[3], VVg[3], VVe[3], rg, var_rg, re, var_re, logl;
};
struct MvPairFit {
  int i, j, status, pad;
  MvPairBlock remle, mle;
};

MV_HD bool mv_finite(double v) { return fabs(v) <= 1.7976931348623157e308; } // false for NaN

// pair q: mv_null_fit<2, C> on its two gathered rows from the start diag(vg_i, vg_j), diag(ve_i, ve_j) -- exactly what
// gemma_hip_mvlmm_null builds for d = 2 -- with the variance epilogue; scratch: MvNrScratch<2, C>::DOUBLES doubles of this lane group
template <int C, class Lanes> MV_HD void mv_pair_fit(const MvPairArgs &p, long q, double *scratch) {
  const int i = p.pairs[2 * q], j = p.pairs[2 * q + 1];
  const double vgi = p.start[8 * (long)i + 6], vei = p.start[8 * (long)i + 7];
  const double vgj = p.start[8 * (long)j + 6], vej = p.start[8 * (long)j + 7];
  constexpr int RAW = mv_pair_raw_doubles(C);
  double *raw = p.raw + q * RAW;
  if (!(mv_finite(vgi) && mv_finite(vei) && mv_finite(vgj) && mv_finite(vej))) {
    // a trait without a univariate fit (a non-finite value in its column): no start, no fit -- the pair reports NaN throughout
    for (int k = Lanes::lane(); k < RAW; k += Lanes::N) raw[k] = 0.0 / 0.0;
    return;
  }
  MvNullArgs a;
  a.g.n = p.n;
  a.g.eval = p.eval;
  a.g.Wt = p.Wt;
  a.g.Yt = p.Yp + 2 * q * (long)p.n;
  a.g.nr_iter = p.nr_iter;
  a.g.nr_prec = p.nr_prec;
  a.g.crt = 0;
  a.g.d = 2;
  a.g.c = C;
  a.em_iter = p.em_iter;
  a.em_prec = p.em_prec;
  a.Vg0[0] = vgi; a.Vg0[1] = 0.0; a.Vg0[2] = 0.0; a.Vg0[3] = vgj;
  a.Ve0[0] = vei; a.Ve0[1] = 0.0; a.Ve0[2] = 0.0; a.Ve0[3] = vej;
  a.out = raw;
  MvNullSe se;
  se.p = raw + mv_pair_out_doubles(C);
  mv_null_fit<2, C, Lanes>(a, scratch, se);
}

// r = V01 / sqrt(V00 V11) and its delta-method variance g^T S g, g = (-r / (2 V00), 1 / sqrt(V00 V11), -r / (2 V11)), S the 3 x 3
// block of the variance matrix in the order (00, 01, 11).  A non-finite or non-positive diagonal gives NaN.
MV_HD void mv_pair_corr(const double *V3, const double *S, double &r, double &var_r) {
  const double v00 = V3[0], v01 = V3[1], v11 = V3[2];
  r = var_r = 0.0 / 0.0;
  if (!(mv_finite(v00) && mv_finite(v11) && v00 > 0.0 && v11 > 0.0)) return;
  const double sq = sqrt(v00 * v11);
  r = v01 / sq;
  const double g[3] = {-r / (2.0 * v00), 1.0 / sq, -r / (2.0 * v11)};
  double v = 0.0;
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) v += g[a] * S[a * 3 + b] * g[b];
  var_r = v;
}

// raw result of pair q -> gemma_mvpair_fit, and B / VB (pair x pass x trait x covariate) unless B is null
MV_HD void mv_pair_finish(const MvPairArgs &p, long q, MvPairFit *fit, double *B, double *VB) {
  const int c = p.c, blk = 2 * 4 + 2 * c + 1, seb = mv_null_se_doubles(2, c);
  const double *raw = p.raw + q * mv_pair_raw_doubles(c);
  MvPairFit f;
  f.i = p.pairs[2 * q];
  f.j = p.pairs[2 * q + 1];
  f.pad = 0;
  bool ok = true;
  for (int pass = 0; pass < 2; ++pass) {
    const double *o = raw + pass * blk, *s = raw + 2 * blk + pass * seb;
    MvPairBlock &b = pass == 0 ? f.remle : f.mle;
    b.Vg[0] = o[0]; b.Vg[1] = o[1]; b.Vg[2] = o[3];
    b.Ve[0] = o[4]; b.Ve[1] = o[5]; b.Ve[2] = o[7];
    b.logl = o[8 + 2 * c];
    for (int v = 0; v < 3; ++v) {
      b.VVg[v] = s[v];
      b.VVe[v] = s[3 + v];
    }
    const double *cov = s + 6 + 2 * c;
    mv_pair_corr(b.Vg, cov, b.rg, b.var_rg);
    mv_pair_corr(b.Ve, cov + 9, b.re, b.var_re);
    for (int v = 0; v < 3; ++v) ok = ok && mv_finite(b.Vg[v]) && mv_finite(b.Ve[v]) && mv_finite(b.VVg[v]) && mv_finite(b.VVe[v]);
    ok = ok && mv_finite(b.rg) && mv_finite(b.var_rg) && mv_finite(b.re) && mv_finite(b.var_re) && mv_finite(b.logl);
    if (B)
      for (int t = 0; t < 2 * c; ++t) {
        B[(q * 2 + pass) * 2 * c + t] = o[8 + t];
        VB[(q * 2 + pass) * 2 * c + t] = s[6 + t];
      }
  }
  f.status = ok ? 0 : 1;
  fit[q] = f;
}

} // namespace gemma_hip

// What the host side of lmm_score_panel.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in lmm_score_panel.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include "dgemm.h"
#include "lmm_assoc.h"

namespace gemma_hip {

struct ScoreRec {
  double beta, se, p_score;
};
struct ScoreHit { // gemma_score_hit
  unsigned int snp, pheno;
  double beta, se, p_score;
};
struct ScoreBest { // gemma_score_best
  double beta, se, p_score;
  long long snp;
};
// a wave's best pair of one phenotype over its 32 rows: the largest finite F, the smallest row among equals (row -1: none)
struct ScoreCell {
  double F, P_xx, P_xy;
  long long row;
};

constexpr int SP_CMAX = 16; // covariates
constexpr int SP_KP = 4;    // kinds per K pass: SP_RG * SP_PG * SP_KP accumulator blocks of 4 doubles = 128 registers of a wave's 256
constexpr int SP_RG = 2;    // 16-row groups of SNPs per wave
constexpr int SP_PG = 2;    // 16-column groups of phenotypes per wave
constexpr int SP_NPOS = SP_RG * SP_PG * 4; // (SNP, phenotype) pairs per lane
// a pivot of the Cholesky factor of S_ww below this fraction of its diagonal element: not positive definite.  Two equal covariate
// columns leave a pivot of a few ulp of either sign; statistics of a Gram matrix this close to singular would be rounding noise.
constexpr double SP_PIVOT_MIN = 1e-12;

// ---- the hits form (gemma_hip_lmm_score_panel_hits_*): pairs with p_score <= p_max and the best pair of every phenotype ----
// Degenerate pairs.  A row that is collinear with the covariates (monomorphic: a multiple of the intercept) has a P_xx that is
// the rounding of sum h x^2 - sum_a (sum h x w~_a)^2, 1e-16 to 1e-13 of sum h x^2 and of either sign, and statistics that are
// noise (p_score near 1, NaN, or 0 where the difference happens to vanish).  The records form prints them as they come; a hits
// list must not carry them to its top, so a pair with P_xx < SP_PXX_FLOOR * sum h x^2 (or a NaN there: an all-missing row) is
// neither a hit nor a best.  1e-8 is 1 - R^2 of x on the covariates: 1e5 above the noise, and the floor under which the tests of
// the records form leave a pair out of their comparison.  sum h x^2 is kept as a float per position (the test needs one digit).
constexpr double SP_PXX_FLOOR = 1e-8;
// The pre-filter.  p = Q(F; 1, df) decreases in F, so a pair can be a hit only at F >= F*(p_max).  score_fcrit_kernel brackets
// F* by bisection on fdist_Q1_dev itself and hands out its LOWER end `lo`, with computed Q^(lo) > p_max, times 1 - SP_FCRIT_MARGIN.
// Derivation of the margin.  Write Q^ = Q (1 + e), |e| <= eps, for the computed function.  Its rounding: on the branch
// F < about 3 the value is 1 - I with p >= 0.08, error <= 1e-14 of p; elsewhere p = exp(ln_pre) cf / b is formed without a
// cancellation, |ln_pre| <= 745 before p underflows, so exp carries <= 745 x a few ulp = 5e-13 and the continued fraction (it
// stops at |delta - 1| < 2 ulp within 512 steps) <= 2e-13: eps = 1e-12.  Suppose a pair has Q^(F) <= p_max and F < lo (1 - m).
// With s = -d ln Q / d ln F (the elasticity; s >= 0.3 for every df >= 1 once Q <= 1/2: df = 1 has 0.318 at Q = 1/2 rising to
// 1/2, df = infinity 0.43 rising without bound), Q(F) >= Q(lo) (1 - m)^-s >= Q(lo) (1 + s m), hence
//     Q^(F) >= Q^(lo) (1 + s m) (1 - eps) / (1 + eps) > p_max (1 + s m) (1 - 2 eps) >= p_max   once   m >= 2 eps / s = 6.7e-12,
// a contradiction.  SP_FCRIT_MARGIN = 1e-9 is 150 times that; it lets through a further 1e-9 s p_max of the pairs, which the
// decision on the computed p_score then rejects.  Two ends are cut off: p_max >= SP_FCRIT_PMAX = 1/2, where s falls to 0 with F
// (no pre-filter: the threshold is -inf, every second pair would pass anyway), and p_max < SP_FCRIT_PMIN = 1e-280, where
// p_score is close to the subnormals and eps no longer holds (the threshold of 1e-280 is used: a superset).  A NaN from the
// function ends the bisection where it stands: `lo` only ever moves to a point with Q^ > p_max.
constexpr double SP_FCRIT_MARGIN = 1e-9;
constexpr double SP_FCRIT_PMAX = 0.5;
constexpr double SP_FCRIT_PMIN = 1e-280;

struct ScoreGeom {
  int n, nc; // individuals, 16-k chunks
  int c, nk; // covariates, kinds = c + 2
  int T, ng; // phenotypes, groups of 16
};

__global__ __launch_bounds__(256) void score_setup_kernel(ScoreGeom g, const double *__restrict__ eval,
                                                         const double *__restrict__ UtWt, const double *__restrict__ Yt,
                                                         const double *__restrict__ lam, double *__restrict__ Rp,
                                                         double *__restrict__ Pyy, int *__restrict__ bad);

struct ScoreArgs {
  const double *UtX; // l x n, leading dimension ld
  long ld, l;
  ScoreGeom g;
  const double *Rp;
  const double *Pyy;
  ScoreRec *out; // out[t * l + s]
  double lnbeta_half_df;
  // the hits form only
  double p_max;
  const double *f_thr;          // the pre-filter's threshold on F (score_fcrit_kernel)
  ScoreHit *hits;               // cap entries
  unsigned long long cap;
  unsigned long long *n_hits;   // counts every hit, stored or not
  ScoreCell *cells;             // [ceil(l / 32)][T], nullptr: no best wanted
};

__global__ void score_fcrit_kernel(double p_max, double df, double lnbeta_half_df, double *__restrict__ out);

template <bool AL, bool HITS = false>
__global__ __launch_bounds__(256, 2) void score_panel_kernel(ScoreArgs a);

__global__ __launch_bounds__(256) void score_best_kernel(ScoreGeom g, long ntile, const ScoreCell *__restrict__ cells,
                                                        const double *__restrict__ Pyy, double lnbeta_half_df,
                                                        ScoreBest *__restrict__ best);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define LMM_SCORE_PANEL_INSTANCES(T) \
  T void score_panel_kernel<false, false>(ScoreArgs); \
  T void score_panel_kernel<false, true>(ScoreArgs); \
  T void score_panel_kernel<true, false>(ScoreArgs); \
  T void score_panel_kernel<true, true>(ScoreArgs);
#ifndef GEMMA_HIP_KERNEL_BODIES
LMM_SCORE_PANEL_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

// What the host side of lmm_assoc.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in lmm_assoc.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <float.h>
#include "lmm_search.hip.h"

namespace gemma_hip {

struct SumStat {
  double beta, se, lambda_remle, lambda_mle, p_wald, p_lrt, p_score, logl_H1;
};

constexpr int ASSOC_MAX_REGION = 64;

// outcome of one bracket's Brent + Newton polish (polish_bracket of lmm_search.hip.h) computed ahead of the per-SNP kernel
struct ChebResult {
  double l;
  int status; // PB_OK / PB_STOP / PB_FAILED; PB_OUTSIDE or CHEB_NONE: not available, polish with streaming evaluations
  int pad;
};
constexpr int CHEB_NONE = 7;

struct AssocArgs {
  const double *UtX;   // l x ld, SNP-major
  const double *UtZ;   // GXE only: l x ld rows U^T (x_s . env)
  const int *flip;     // GXE only: l flags, genotypes recoded 2 - x
  long ld;
  long l;
  const double *eval;  // n
  const double *Uty;   // n
  const double *UtWt;  // c x n (covariate-major copy of UtW)
  SumStat *out;
  int n;
  int a_mode;
  int n_region;
  int plink_nan_rule;
  double l_min, l_max;
  double l_mle_null, logl_mle_H0;
  double lnbeta_half_df;  // ln B(df/2, 1/2), df = n - c - 1 (host lgamma)
  double logdet_lmin, logdet_lmax; // sum_i log|l*delta_i + 1| at l_min / l_max (SNP independent; logdet_ends_kernel)
  int have_logdet_ends;
  // fixed-lambda table (lmm_grid.hip.h): per SNP the x-dependent sums at the grid lambdas, plus the SNP-independent
  // sums; columns of T: [q] = sum x^2 w_q,  [grid_xa0 + a * grid_nq + q] = sum x u_a w_q (a < c: U^T W column, a = c: U^T y)
  const double *grid_T; // l x grid_ld (this batch), nullptr when the table path is off
  const double *grid_F; // grid_nq x 16: pair sums among (w_1..w_c, y) in upper-triangle order, [15] = sum w_q
  int grid_ld, grid_nq, grid_xa0;
  int have_grid;
  double lam_grid[ASSOC_MAX_REGION + 1]; // l_min*exp(i*log(l_max/l_min)/n_region), host libm
  // Brackets already polished from Chebyshev-in-log(lambda) series (lmm_search.hip.h; cheb_scan_kernel / cheb_search_kernel
  // of lmm_grid.hip.h) for the grid intervals cheb_j0 .. cheb_j0 + cheb_nint - 1: cheb_slots[snp * cheb_nint + k] = the
  // SNP's slot in interval k or -1, cheb_res[(func * cheb_nint + k) * cheb_cap + slot] = what polish_bracket returned
  // (func 0: REML, 1: ML).  Everything else of this block describes the tables to those two kernels.
  const double *cheb_T;   // [k][col][slot]: series of the x-dependent sums, column-major over the interval's slots
  const double *cheb_F;   // [k][cheb_fld]: SNP-independent series
  const int *cheb_slots;
  const ChebResult *cheb_res;
  long cheb_cap;
  int cheb_ld, cheb_fld, cheb_xa0;
  int cheb_j0, cheb_nint;
  int have_cheb;
  unsigned long long cheb_qmask; // bit k: interval k is tabulated in Q form (series of sum a b delta H; lmm_search.hip.h)
  int cheb_final;          // 1: the final likelihood at lambda-hat (and with it CalcRLWald's sums) is assembled from the bracket's
                           //    series too -- the SNP's row is not read at all when its search ran on the tables
  int cheb_logdet_off;     // offset of the series of sum_i log(lambda delta_i + 1) inside an interval's cheb_F block
  const double *cheb_iv;   // [k][2] = {mid, 1 / half} of interval k in t = log(lambda)
  double cheb_mid[ASSOC_MAX_REGION], cheb_inv_half[ASSOC_MAX_REGION];
};

// any number of covariates (c <= GEN_CMAX): the (c+2) x (c+2) product table is covered by 4 x 4 register
// tiles, one streaming pass per tile pair; row-0 sums and the projection recursion live in per-wave LDS.
constexpr int GEN_CMAX = 16;
constexpr int GEN_NI = (GEN_CMAX + 3) * (GEN_CMAX + 2) / 2;
constexpr int GEN_LDS_PER_WAVE = 6 * GEN_NI;
// Beyond 16 covariates (20 principal components + age + sex is an everyday GWAS model; the reference is generic in n_cvt,
// src/lmm.cpp:283-357) the same code runs with ONE wavefront per workgroup and its six tables in dynamic LDS:
// 6 (c + 3)(c + 2) / 2 doubles = 106 KiB at c = 64.  "wide" kernels below; slow (the product table takes (c + 2)^2 / 32 passes
// per evaluation) but complete.
constexpr int GEN_CMAX_WIDE = 64;
__host__ __device__ inline int gen_ni_for(int c) { return (c + 3) * (c + 2) / 2; }

template <int C>
__global__ __launch_bounds__(256, (C == 1 ? 3 : (C == 2 ? 2 : 1))) void lmm_assoc_kernel(AssocArgs g);

template <int UNR, int WPS>
__global__ __launch_bounds__(256, WPS) void lmm_assoc1_variant_kernel(AssocArgs g);

__global__ __launch_bounds__(256) void lmm_assoc_generic_kernel(AssocArgs g, int c);

__global__ __launch_bounds__(64) void lmm_assoc_wide_kernel(AssocArgs g, int c);

template <int C>
__global__ __launch_bounds__(256, (C <= 2 ? 2 : 1)) void lmm_gene_kernel(AssocArgs g);

__global__ __launch_bounds__(256) void lmm_gene_generic_kernel(AssocArgs g, int c);

__global__ __launch_bounds__(64) void lmm_gene_wide_kernel(AssocArgs g, int c);

template <int CT>
__global__ __launch_bounds__(256, (CT <= 3 ? 2 : 1)) void lmm_gxe_kernel(AssocArgs g);

__global__ __launch_bounds__(256) void lmm_gxe_generic_kernel(AssocArgs g, int ct);

__global__ __launch_bounds__(64) void logdet_ends_kernel(const double *__restrict__ eval, int n, double l_min,
                                                         double l_max, double *__restrict__ out2);

// ------------------------------------------------------------------ null model
// CalcLambda(func, eval, UtW, Uty, ...) with calc_null = true (GEMMA src/lmm.cpp:2143-2180,
// called at src/gemma.cpp:2711,2734), CalcPve's LogRL_dev2 (:2197) and CalcLmmVgVeBeta's P_yy
// (:2253-2258).  Projecting out w_1..w_c (nc_total = c, df = n - c) is the alternative-model code
// with c - 1 covariates and the last covariate in the role of x.
struct NullOut {
  double l_mle, logl_mle, l_remle, logl_remle, dev2_remle, Pyy_remle, Pyy_mle;
};

__global__ __launch_bounds__(64) void lmm_gxe_wide_kernel(AssocArgs g, int ct);

__global__ __launch_bounds__(64) void lmm_null_wide_kernel(AssocArgs g, int cp, NullOut *out);

template <int CP>
__global__ __launch_bounds__(64) void lmm_null_kernel(AssocArgs g, NullOut *out);

__global__ __launch_bounds__(64) void lmm_null_generic_kernel(AssocArgs g, int cp, NullOut *out);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define LMM_ASSOC_INSTANCES(T) \
  T void lmm_assoc_kernel<1>(AssocArgs); \
  T void lmm_assoc_kernel<2>(AssocArgs); \
  T void lmm_assoc_kernel<3>(AssocArgs); \
  T void lmm_assoc_kernel<4>(AssocArgs); \
  T void lmm_assoc1_variant_kernel<2, 4>(AssocArgs); \
  T void lmm_assoc1_variant_kernel<4, 2>(AssocArgs); \
  T void lmm_assoc1_variant_kernel<4, 3>(AssocArgs); \
  T void lmm_assoc1_variant_kernel<4, 4>(AssocArgs); \
  T void lmm_assoc1_variant_kernel<8, 3>(AssocArgs); \
  T void lmm_gene_kernel<1>(AssocArgs); \
  T void lmm_gene_kernel<2>(AssocArgs); \
  T void lmm_gene_kernel<3>(AssocArgs); \
  T void lmm_gene_kernel<4>(AssocArgs); \
  T void lmm_gxe_kernel<3>(AssocArgs); \
  T void lmm_gxe_kernel<4>(AssocArgs); \
  T void lmm_null_kernel<0>(AssocArgs, NullOut *); \
  T void lmm_null_kernel<1>(AssocArgs, NullOut *); \
  T void lmm_null_kernel<2>(AssocArgs, NullOut *); \
  T void lmm_null_kernel<3>(AssocArgs, NullOut *); \
  T void lmm_null_kernel<4>(AssocArgs, NullOut *);
#ifndef GEMMA_HIP_KERNEL_BODIES
LMM_ASSOC_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

// What the host side of lmm_grid.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in lmm_grid.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "dgemm.h"
#include "lmm_assoc.h"

namespace gemma_hip {

constexpr int GRID_FIX_LD = 16; // per weight: (c+1)(c+2)/2 <= 15 pair sums + the trace sum_i w_q(i)

struct GridGeom {
  int nq;    // weights: 1 + 2 * (n_region + 1)
  int nbx;   // 16-column MFMA blocks of the x.x group (nq columns)
  int nba;   // 16-column MFMA blocks of the x.u_a group ((c+1) * nq columns, a-major)
  int nc;    // 16-row K chunks: ceil(n / 16)
};

__global__ void grid_weights_kernel(AssocArgs g, GridGeom gg, int c, double *__restrict__ Rp);

__global__ __launch_bounds__(256) void grid_fixed_kernel(AssocArgs g, int c, double *__restrict__ F);

// T[s][cb * 16 + col] = sum_k A(s, k) * R(k, col),  A = x^2 for the first NBX column blocks, x for the rest.
// One block = 16 SNP rows; its 4 waves split K; v_mfma_f64_16x16x4_f64 with the A operand read straight from
// the UtX rows (lane (i, kq) takes x[s0 + i][16 chunk + 4 kq .. + 3]: a full 128-byte line per row per chunk;
// the k order inside a chunk is permuted identically on both operands).
// GATHER (the Chebyshev tables of the bracket intervals): blockIdx.y = interval k; the rows are the SNPs listed in
// list[k * cap ..] (count[k] of them, written by cheb_scan_kernel), the weights Rp + k * rp_stride, and the series of
// `slot` is column `slot` of the interval's plane: T[(k * NB * 16 + col) * cap + slot].  A SNP's sums depend on its own row only (fixed k order), so its series
// is the same bits whichever slot and whichever neighbours it gets.
struct TableGather {
  const int *list;
  const int *count;
  long cap;
  long rp_stride;
};

template <int NBX, int NBA, bool GATHER>
__global__ __launch_bounds__(256) void grid_table_kernel(const double *__restrict__ UtX, long ld, long l, int n,
                                                        int nc, const double *__restrict__ Rp,
                                                        double *__restrict__ T, TableGather tg);

// ---- the same table product, tiled for reuse (default): one WAVE owns RG * 16 SNP rows and one slice of K, so that a
// 16-k chunk of the weight matrix (NB * 2 KiB) feeds RG * NB * 4 MFMAs instead of NB * 4; a block's four waves take four
// different row sets over the SAME K slice (their weight reads coincide in the L1), blockIdx.y picks the K slice.  The K
// slices leave partial sums P[ks][row][col]; table_reduce_kernel adds them in slice order (fixed order, no atomics: a
// SNP's sums do not depend on its neighbours, its slot or the batch size -- the number of slices depends on n alone).
struct TableV2 {
  const double *UtX;
  long ld;
  long l;        // rows (dense) -- GATHER: unused, count[kint] rules
  int n, nc;     // individuals, 16-k chunks
  int ksplit;    // K slices
  const double *Rp;
  double *P;     // partial sums: [(kint * ksplit + ks) * cap + row] * NB16 + col
  long cap;      // rows allocated per interval / batch
  TableGather tg;
};

template <int NBX, int NBA, int RG, bool GATHER, bool PF>
__global__ __launch_bounds__(256, PF ? 1 : 2) void table_v2_kernel(TableV2 a);

template <bool GATHER>
__global__ __launch_bounds__(256) void table_reduce_kernel(const double *__restrict__ P, int ksplit, long cap, int nb16,
                                                          long l, const int *__restrict__ count, double *__restrict__ T);

// ---- the dense fixed-lambda tables of a GROUP of phenotypes from one read of U^T x (gemma_hip_lmm_multi_batch).  Of the columns
// of [X.X | X] * R only the nq columns x . y_t w_q belong to a phenotype; the weight matrix of a group is
//   [ x.x : NBX blocks | x . w_a : c * nq columns | x . y_1 : nq | ... | x . y_G : nq ]   (the x . u group packed, MULTI_NBA blocks)
// in the operand order of grid_weights_kernel, and the product is table_v2_kernel<2, MULTI_NBA, MULTI_RG> ITSELF on that matrix
// (one body: a wrapper around a shared device function changed the code generated for the existing instantiations).
// An entry of a table is one row of U^T x against one weight column over one k sequence -- the chunk order, the k order inside a
// chunk, the K slices (a function of n alone) and the slice-order sum are table_v2_kernel's and table_reduce_kernel's -- so every
// entry is the same bits as the phenotype's own table_v2_kernel + table_reduce_kernel give, whichever column block it sits in
// and however many row groups the wave holds.
// table_multi_reduce_kernel sums the slices and scatters the columns into G tables of the single-phenotype layout (grid_ld,
// grid_xa0, columns a * nq + q): the y columns of a phenotype start at c * nq, no multiple of 16, and straddle column blocks.
// The accumulator budget is that instantiation's, the one c = 4 runs today (2 row groups x 10 column blocks of
// v_mfma_f64_16x16x4_f64: 160 accumulator registers of 256): 128 columns of the x . u group hold c + G <= 5 vectors.
constexpr int MULTI_NBA = 8, MULTI_RG = 2, MULTI_GMAX = 4;
struct MultiWeights {
  const double *Uty[MULTI_GMAX];
  int G;
};

__global__ void grid_weights_multi_kernel(AssocArgs g, GridGeom gg, int c, MultiWeights mw, double *__restrict__ Rp);
struct TableMulti {
  const double *P; // partial sums of the product: [ks * cap + row] * nb16m + col
  int ksplit;
  long cap, l;
  int nb16m;       // columns of P
  int nb16;        // columns of one phenotype's table (grid_ld)
  int y0, nq;      // a table's y columns: [y0, y0 + nq); phenotype g of the group has them at y0 + g * nq in P
  double *T;       // G tables, tstride doubles apart
  long tstride;
};

__global__ __launch_bounds__(256) void table_multi_reduce_kernel(TableMulti m);

// ------------------------------------------------------------------ Chebyshev tables of the bracket intervals
// (lmm_search.hip.h).  Per lmm_setup and interval: c_k(delta_i), the series coefficients of t -> H_i(t) and of
// t -> 1 - H_i(t) (cheb_coeff_kernel), from them the weight matrix of the table product in MFMA operand order
// (cheb_weights_kernel; columns: [k] for x^2, [a * CHEB_N + k] for x u_a) and the SNP-independent series
// (cheb_fixed_kernel).  Per batch: cheb_scan_kernel finds every SNP's bracket intervals from the fixed-lambda table and
// hands out slots, grid_table_kernel<.., GATHER> computes the series of exactly those (SNP, interval) pairs.
constexpr double CHEB_MARGIN = 0.15; // of the interval's length, either side
constexpr double CHEB_MIN_LAMBDA = 1e-3; // intervals below are tabulated in Q form (lmm_search.hip.h): dS/dt is O(lambda) of S
                                         // there, and a series good to 1e-15 of S would carry 1e-13/lambda of relative error in it

struct ChebNodes {
  double lam[CHEB_N]; // exp(node m)
};

__global__ void cheb_coeff_kernel(const double *__restrict__ eval, int n, ChebNodes nd, const double *__restrict__ Dfit,
                                  int qform, double *__restrict__ Ck, double *__restrict__ Gk, double *__restrict__ Lk,
                                  double *__restrict__ G2k);

__global__ void cheb_weights_kernel(AssocArgs g, GridGeom gg, int c, const double *__restrict__ Ck,
                                    double *__restrict__ Rp);

__global__ __launch_bounds__(256) void cheb_fixed_kernel(AssocArgs g, int c, const double *__restrict__ Ck,
                                                        const double *__restrict__ Gk, const double *__restrict__ Lk,
                                                        const double *__restrict__ G2k, double *__restrict__ F);

// Which grid intervals bracket a sign change of dev1 for this SNP (REML and / or ML search, as a_mode asks): the
// same dev1_grid values calc_lambda computes from the fixed-lambda table.  Every (SNP, tabulated interval) pair with a
// bracket gets a slot of that interval's table (slots[snp * nint + k], -1 = none) and the bracket's end values
// dends[(func * nint + k) * cap + slot] = {dev1(lambda_lo), dev1(lambda_hi)} (NaN = func has no bracket there).
struct ChebScanArgs {
  int *count;     // nint, zeroed before the launch
  int *list;      // nint x cap
  int *slots;     // l x nint
  double2 *dends; // 2 x nint x cap
  long cap;
};

template <int C>
__global__ __launch_bounds__(256) void cheb_scan_kernel(AssocArgs g, ChebScanArgs sc);

// One THREAD per (slot, interval, func): Brent + Newton of that bracket on the SNP's series (polish_bracket over
// ChebEvaluator, lmm_search.hip.h -- the code tests/cpp/cheb_search_check.cpp runs on the CPU).  The series are read
// column-major over the slots (coalesced across the wave), the SNP-independent series are the same addresses for every
// thread.  grid = (ceil(cap / 64), nint, 2).
struct ChebSearchArgs {
  const int *count;
  const int *list;            // [k * cap + slot] = SNP index (the constants of a Q-form interval come from its fixed-lambda row)
  unsigned long long qmask;   // bit k: interval k is in Q form
  const double2 *dends;
  ChebResult *res;
  double mid[ASSOC_MAX_REGION], inv_half[ASSOC_MAX_REGION];
};

template <int C>
__global__ __launch_bounds__(64) void cheb_search_kernel(AssocArgs g, ChebSearchArgs sa);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define LMM_GRID_INSTANCES(T) \
  T void grid_table_kernel<2, 3, false>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 3, true>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 5, false>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 5, true>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 6, false>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 6, true>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 8, false>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void grid_table_kernel<2, 8, true>(const double *, long, long, int, int, const double *, double *, TableGather); \
  T void table_v2_kernel<2, 3, 4, false, false>(TableV2); \
  T void table_v2_kernel<2, 3, 4, false, true>(TableV2); \
  T void table_v2_kernel<2, 3, 4, true, false>(TableV2); \
  T void table_v2_kernel<2, 3, 4, true, true>(TableV2); \
  T void table_v2_kernel<2, 5, 2, false, false>(TableV2); \
  T void table_v2_kernel<2, 5, 2, false, true>(TableV2); \
  T void table_v2_kernel<2, 5, 2, true, false>(TableV2); \
  T void table_v2_kernel<2, 5, 2, true, true>(TableV2); \
  T void table_v2_kernel<2, 6, 2, false, false>(TableV2); \
  T void table_v2_kernel<2, 6, 2, false, true>(TableV2); \
  T void table_v2_kernel<2, 6, 2, true, false>(TableV2); \
  T void table_v2_kernel<2, 6, 2, true, true>(TableV2); \
  T void table_v2_kernel<2, 8, 2, false, false>(TableV2); \
  T void table_v2_kernel<2, 8, 2, false, true>(TableV2); \
  T void table_v2_kernel<2, 8, 2, true, false>(TableV2); \
  T void table_v2_kernel<2, 8, 2, true, true>(TableV2); \
  T void table_reduce_kernel<false>(const double *, int, long, int, long, const int *, double *); \
  T void table_reduce_kernel<true>(const double *, int, long, int, long, const int *, double *); \
  T void cheb_scan_kernel<1>(AssocArgs, ChebScanArgs); \
  T void cheb_scan_kernel<2>(AssocArgs, ChebScanArgs); \
  T void cheb_scan_kernel<3>(AssocArgs, ChebScanArgs); \
  T void cheb_scan_kernel<4>(AssocArgs, ChebScanArgs); \
  T void cheb_search_kernel<1>(AssocArgs, ChebSearchArgs); \
  T void cheb_search_kernel<2>(AssocArgs, ChebSearchArgs); \
  T void cheb_search_kernel<3>(AssocArgs, ChebSearchArgs); \
  T void cheb_search_kernel<4>(AssocArgs, ChebSearchArgs);
#ifndef GEMMA_HIP_KERNEL_BODIES
LMM_GRID_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

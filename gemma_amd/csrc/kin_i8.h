// What the host side of kin_i8.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in kin_i8.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ingest.h"

namespace gemma_hip {

constexpr int KI8_SEG = 4096;  // individuals i per block of the correction kernel (16 per thread)
constexpr int KI8_LIST = 4096; // SNPs listed per pass (LDS); a block walks the SNP axis in ranges of this many rows

__global__ void kin_i8_transpose_kernel(const int8_t *__restrict__ A, long l, long ldk, long n, int8_t *__restrict__ At,
                                        int8_t *__restrict__ Gt, long ldl, long rows_out);

__global__ void kin_i8_accum_kernel(const int *__restrict__ C, long ldc, long n, double *__restrict__ acc);

struct KinCorrArgs {
  const int8_t *A;   // l x ldk, SNP-major packed (g | m << 4)
  const int8_t *At;  // individual-major packed, ldl bytes per row
  const double *mean; // l
  long l, ldk, ldl, n;
  double *S;     // n x n, row j: S[j][i]
  double *a;     // n
  double *smu2;  // 1
  const int *lists_ok; // device flag of kin_i8_scan_kernel (nullptr: always run)
};

__global__ __launch_bounds__(256) void kin_i8_corr_kernel(KinCorrArgs g);

__global__ __launch_bounds__(256) void kin_i8_pack2_kernel(const int8_t *__restrict__ A, long l, long ldk, int nseg,
                                                           unsigned *__restrict__ A2);

__global__ __launch_bounds__(256) void kin_i8_count_kernel(const int8_t *__restrict__ M, long rows, long len, long ld,
                                                           int *__restrict__ cnt);

// exclusive scans of the two count arrays (one block of 1024 threads), the decision whether the lists fit, sum mu^2
struct KinScanArgs {
  const int *cntS, *cntJ;
  int *offS, *offJ; // l + 1, n + 1
  long l, n;
  long cap;         // entries either list buffer holds
  int *ok;          // out: 1 = lists are valid
  const double *mean;
  double *smu2;     // += sum mu_s^2 when ok
};

__global__ __launch_bounds__(1024) void kin_i8_scan_kernel(KinScanArgs g);

template <bool BYIDV>
__global__ __launch_bounds__(256) void kin_i8_fill_kernel(const int8_t *__restrict__ M, long rows, long len, long ld,
                                                          const int *__restrict__ off, int *__restrict__ list,
                                                          const int *__restrict__ ok, const double *__restrict__ mean,
                                                          long l, double *__restrict__ a, double *__restrict__ cj);

__global__ __launch_bounds__(256) void kin_i8_sub_kernel(const int *__restrict__ offS, const int *__restrict__ listS, long l,
                                                         int nseg, const int *__restrict__ ok, int *__restrict__ sub);

constexpr double KI8_FIX = 17592186044416.0; // 2^44: fixed point of the both-missing term
struct KinCorr2Args {
  const unsigned *A2; // l x ld2 dwords, ld2 = 256 nseg
  long ld2;
  const double *mean;
  long n;
  const int *offJ, *listJ, *offS, *listS, *sub;
  int nseg;
  const double *cj;
  double *S; // n x n, row j: S[j][i]
  const int *ok;
  int dbg_skip_pairs; // timing experiments only (GEMMA_HIP_KIN_DBG=1): the both-missing term left out, results wrong
  int dbg_skip_main;  // (GEMMA_HIP_KIN_DBG=2): the genotype term left out
};

__global__ __launch_bounds__(256) void kin_i8_corr2_kernel(KinCorr2Args g);

__global__ void kin_i8_fold_kernel(double *__restrict__ K, long n, const double *__restrict__ GtG,
                                   const double *__restrict__ S, const double *__restrict__ a,
                                   const double *__restrict__ smu2);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define KIN_I8_INSTANCES(T) \
  T void kin_i8_fill_kernel<false>(const int8_t *, long, long, long, const int *, int *, const int *, const double *, long, double *, double *); \
  T void kin_i8_fill_kernel<true>(const int8_t *, long, long, long, const int *, int *, const int *, const double *, long, double *, double *);
#ifndef GEMMA_HIP_KERNEL_BODIES
KIN_I8_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

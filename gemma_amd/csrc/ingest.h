// What the host side of ingest.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in ingest.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace gemma_hip {

// device helpers the ingest, QC, kinship and int8 kernels share (the int8 headers include only this file of the pair)
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// PLINK 2-bit code -> genotype (GEMMA src/lmm.cpp:1797-1812; src/gemma_io.cpp:1665-1682):
// v = b0 + 2*b1 : 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing
__device__ __forceinline__ double plink_value(unsigned v, bool &missing) {
  missing = (v == 1u);
  return (v == 0u) ? 2.0 : (v == 2u) ? 1.0 : 0.0;
}

struct IngestArgs {
  const void *src;    // f64 (ld doubles per SNP) or bytes (ld bytes per SNP)
  long ld;
  long l;
  const int *idx_map; // PLINK: position in ni_total of analysed individual j (nullptr = identity)
  int n;              // individuals written per SNP
  double *dst;        // l x ldo, SNP-major
  long ldo;
  int k_mode;         // kinship only: 1 centred, 2 standardised
};

template <bool PLINK>
__global__ __launch_bounds__(256) void ingest_lmm_kernel(IngestArgs g);

// GXE ingest (GEMMA src/lmm.cpp:2316-2361 BIMBAM, :2487-2536 PLINK): mean-impute, recode 2 - x when x_mean > 1,
// and also write z = x . env; flip[s] records the recoding (beta changes sign, :2403 / :2584).
struct IngestGxeArgs {
  const void *src;
  long ld, l;
  const int *idx_map;
  int n;
  const double *env; // n
  double *X, *Z;     // l x ldo each
  long ldo;
  int *flip;
};

template <bool PLINK>
__global__ __launch_bounds__(256) void ingest_gxe_kernel(IngestGxeArgs g);

template <bool PLINK>
__global__ __launch_bounds__(256) void ingest_kin_kernel(IngestArgs g);

__global__ void transpose_kernel(const double *in, long rows, long cols, long ld, double *out,
                                 long ldo);

__global__ __launch_bounds__(256) void rowsum_kernel(const double *G, long n, long ld, double *Gw);

__global__ __launch_bounds__(1024) void total_kernel(const double *Gw, long n, double *d);

__global__ __launch_bounds__(256) void center_update_kernel(double *G, long n, long ld,
                                                            const double *Gw, const double *d);

__global__ void loco_kernel(const double *__restrict__ Ka, double nsa, double *__restrict__ Kc, double nsc, long total);

__global__ void zero_small_eval_kernel(double *eval, long n, double *trace);

// AnalyzePlink's stale beta/se when CalcRLWald was skipped (GEMMA src/lmm.cpp:1725,1870):
// a failed SNP (NaN logl_H1, a_mode 1) reports the beta/se of the nearest preceding SNP that
// did run CalcRLWald; carry_in covers the previous batch, carry_out receives the batch's last.
struct SumStatRaw { double v[8]; };

__global__ void plink_carry_kernel(SumStatRaw *out, long l, const double *carry_in,
                                   double *carry_out);

__global__ void subselect_kernel(const double *__restrict__ K, long ni_total, const int *__restrict__ map, long n,
                                 double *__restrict__ G);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define INGEST_INSTANCES(T) \
  T void ingest_lmm_kernel<false>(IngestArgs); \
  T void ingest_lmm_kernel<true>(IngestArgs); \
  T void ingest_gxe_kernel<false>(IngestGxeArgs); \
  T void ingest_gxe_kernel<true>(IngestGxeArgs); \
  T void ingest_kin_kernel<false>(IngestArgs); \
  T void ingest_kin_kernel<true>(IngestArgs);
#ifndef GEMMA_HIP_KERNEL_BODIES
INGEST_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

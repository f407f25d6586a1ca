// What the host side of lmm_pair.hip.h needs: argument structs, constants, kernel declarations.  The device functions and kernel
// bodies are in lmm_pair.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "lmm_assoc.h"
#include "lmm_score_panel.h"

namespace gemma_hip {

constexpr int PR_WAVES = 4; // wavefronts (pairs) per workgroup; the last workgroup is ragged

// a list of (SNP row, phenotype) pairs and what the phenotypes bring along
struct PairArgs {
  const ScoreHit *pairs;     // m entries (gemma_score_hit); only snp and pheno are read
  long m;
  const double *Yt;          // T x n: U^T Y transposed
  const double *l_mle_null;  // T
  const double *logl_mle_H0; // T
  int T;
};

// C covariates in registers; UNR and WPS as the single-phenotype launch of that C has them (launch_assoc)
template <int C, int UNR, int WPS>
__global__ __launch_bounds__(64 * PR_WAVES, WPS) void lmm_pair_kernel(AssocArgs g, PairArgs p);

__global__ __launch_bounds__(64 * PR_WAVES) void lmm_pair_generic_kernel(AssocArgs g, int c, PairArgs p);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define LMM_PAIR_INSTANCES(T) \
  T void lmm_pair_kernel<1, 4, 4>(AssocArgs, PairArgs); \
  T void lmm_pair_kernel<2, 2, 2>(AssocArgs, PairArgs); \
  T void lmm_pair_kernel<3, 2, 1>(AssocArgs, PairArgs); \
  T void lmm_pair_kernel<4, 2, 1>(AssocArgs, PairArgs);
#ifndef GEMMA_HIP_KERNEL_BODIES
LMM_PAIR_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

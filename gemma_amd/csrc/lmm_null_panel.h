// What the host side of lmm_null_panel.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in lmm_null_panel.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "lmm_assoc.h"
#include "lmm_score_panel.h"

namespace gemma_hip {

constexpr int NP_WAVES = 4;     // wavefronts (phenotypes) per workgroup of the FixedC and GenericC forms; the last workgroup is ragged
constexpr int NP_CMAX = SP_CMAX; // covariates of the optional beta / se(beta) output

template <int CP>
__global__ __launch_bounds__(64 * NP_WAVES) void lmm_null_panel_kernel(AssocArgs g, const double *__restrict__ Yt, int T,
                                                                      NullOut *__restrict__ out);

__global__ __launch_bounds__(64 * NP_WAVES) void lmm_null_panel_generic_kernel(AssocArgs g, int cp, const double *__restrict__ Yt,
                                                                              int T, NullOut *__restrict__ out);

__global__ __launch_bounds__(64) void lmm_null_panel_wide_kernel(AssocArgs g, int cp, const double *__restrict__ Yt, int T,
                                                                 NullOut *__restrict__ out);
struct NullFit8 {
  double l_mle_null, logl_mle_H0, l_remle_null, logl_remle_H0, pve, pve_se, vg_remle, ve_remle;
};

__global__ __launch_bounds__(256) void null_panel_derive_kernel(const NullOut *__restrict__ in, int T, double trace_G, double df,
                                                               NullFit8 *__restrict__ fit);

__global__ __launch_bounds__(64 * NP_WAVES) void null_panel_beta_kernel(int n, int c, int T, const double *__restrict__ eval,
                                                                       const double *__restrict__ UtWt, const double *__restrict__ Yt,
                                                                       const NullOut *__restrict__ fit, double *__restrict__ beta,
                                                                       double *__restrict__ se_beta);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define LMM_NULL_PANEL_INSTANCES(T) \
  T void lmm_null_panel_kernel<0>(AssocArgs, const double *, int, NullOut *); \
  T void lmm_null_panel_kernel<1>(AssocArgs, const double *, int, NullOut *); \
  T void lmm_null_panel_kernel<2>(AssocArgs, const double *, int, NullOut *); \
  T void lmm_null_panel_kernel<3>(AssocArgs, const double *, int, NullOut *); \
  T void lmm_null_panel_kernel<4>(AssocArgs, const double *, int, NullOut *);
#ifndef GEMMA_HIP_KERNEL_BODIES
LMM_NULL_PANEL_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

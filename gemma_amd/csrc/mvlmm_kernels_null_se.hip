// The fixed null-fit instances with the variance epilogue (MvNullSe: VVg, VVe, VB of gemma_hip_mvlmm_null_se): the shapes of
// mvlmm_null_kernel in mvlmm_kernels.hip / mvlmm_kernels_wide.hip, as kernels of their own so that those stay what they are.
#include "mvlmm_kernels.hip.h"
#include "mvlmm_pair.h"

using namespace gemma_hip;

namespace gemma_hip {

template <int D, int C> __global__ __launch_bounds__(64) void mvlmm_null_se_kernel(MvNullArgs a, double *se_out) {
  __shared__ double scratch[MvNrScratch<D, C>::DOUBLES];
  MvNullSe se;
  se.p = se_out;
  mv_null_fit<D, C, MvWaveLanes>(a, scratch, se);
}

} // namespace gemma_hip

#define MV_FOR_D(F, C) F(1, C) F(2, C) F(3, C) F(4, C) F(5, C)
#define MV_FOR_D3(F, C) F(1, C) F(2, C) F(3, C)

// c = covariates of the null model (>= 1); se: 2 x mv_null_se_doubles(d, c).  Returns 0, a hipError_t, or -1 for a (d, c) without a
// fixed kernel -- the same table as gemma_hip_mvlmm_null_launch_.
extern "C" int gemma_hip_mvlmm_null_se_launch_(const MvNullArgs *a, int d, int c, double *se, hipStream_t s) {
#define MV_CASE(DD, CC)                                                                        \
  if (d == DD && c == CC) {                                                                    \
    hipLaunchKernelGGL((mvlmm_null_se_kernel<DD, CC>), dim3(1), dim3(64), 0, s, *a, se);       \
    return (int)hipGetLastError();                                                             \
  }
  MV_FOR_D(MV_CASE, 1)
  MV_FOR_D(MV_CASE, 2)
  MV_FOR_D(MV_CASE, 3)
  MV_FOR_D3(MV_CASE, 4)
  MV_FOR_D3(MV_CASE, 5)
  MV_FOR_D3(MV_CASE, 6)
#undef MV_CASE
  return -1;
}

// The two-trait null fits of a whole panel (gemma_hip_mvlmm_null_pairs, abi_mvlmm_pairs.inc.h): for every pair (i, j) of traits what
// gemma_hip_mvlmm_null computes for d = 2 on columns i and j -- mv_null_fit<2, C> from MphInitial's diagonal start -- with the
// variance epilogue (MvNullSe), one wavefront per pair.  The pair's two rows of U^T Y are gathered into a slab of their own first, so
// MvArgs keeps its layout and the fit body reads them as it reads any d x n block.
#include <algorithm>

#include "mvlmm_kernels.hip.h"
#include "mvlmm_pair.h"

using namespace gemma_hip;

namespace gemma_hip {

// Yp[q][0][k] = Yt[i_q][k], Yp[q][1][k] = Yt[j_q][k]; grid.y walks the pairs
__global__ __launch_bounds__(256) void mvpair_gather_kernel(const double *__restrict__ Yt, long n, const int *__restrict__ pairs, long m,
                                                            double *__restrict__ Yp) {
  for (long q = blockIdx.y; q < m; q += gridDim.y) {
    const long i = pairs[2 * q], j = pairs[2 * q + 1];
    for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) {
      Yp[(2 * q) * n + k] = Yt[i * n + k];
      Yp[(2 * q + 1) * n + k] = Yt[j * n + k];
    }
  }
}

// one pair per wavefront, WAVES per workgroup; the waves never synchronise with each other
template <int C, int WAVES> __global__ __launch_bounds__(64 * WAVES) void mvlmm_pair_null_kernel(MvPairArgs p) {
  __shared__ double scratch[WAVES][MvNrScratch<2, C>::DOUBLES];
  const int wv = (int)(threadIdx.x >> 6);
  const long q = (long)blockIdx.x * WAVES + wv;
  if (q >= p.m) return;
  mv_pair_fit<C, MvWaveLanes>(p, q, scratch[wv]);
}

// raw -> gemma_mvpair_fit (+ B, VB); one thread per pair
__global__ __launch_bounds__(256) void mvpair_finish_kernel(MvPairArgs p, MvPairFit *__restrict__ fit, double *__restrict__ B,
                                                            double *__restrict__ VB) {
  const long q = (long)blockIdx.x * 256 + threadIdx.x;
  if (q < p.m) mv_pair_finish(p, q, fit, B, VB);
}

} // namespace gemma_hip

extern "C" int gemma_hip_mvpair_gather_launch_(const double *Yt, long n, const int *pairs, long m, double *Yp, hipStream_t s) {
  const dim3 grid((unsigned)std::min<long>((n + 255) / 256, 1024), (unsigned)std::min<long>(m, 65535));
  hipLaunchKernelGGL(mvpair_gather_kernel, grid, dim3(256), 0, s, Yt, n, pairs, m, Yp);
  return (int)hipGetLastError();
}

extern "C" int gemma_hip_mvpair_launch_(const MvPairArgs *p, int waves, hipStream_t s) {
#define MV_CASE(CC)                                                                                                          \
  if (p->c == CC) {                                                                                                          \
    if (waves == 1)                                                                                                          \
      hipLaunchKernelGGL((mvlmm_pair_null_kernel<CC, 1>), dim3((unsigned)p->m), dim3(64), 0, s, *p);                         \
    else                                                                                                                     \
      hipLaunchKernelGGL((mvlmm_pair_null_kernel<CC, 4>), dim3((unsigned)((p->m + 3) / 4)), dim3(256), 0, s, *p);            \
    return (int)hipGetLastError();                                                                                           \
  }
  MV_CASE(1) MV_CASE(2) MV_CASE(3) MV_CASE(4) MV_CASE(5) MV_CASE(6)
#undef MV_CASE
  return (int)hipErrorInvalidValue;
}

extern "C" int gemma_hip_mvpair_finish_launch_(const MvPairArgs *p, MvPairFit *fit, double *B, double *VB, hipStream_t s) {
  hipLaunchKernelGGL(mvpair_finish_kernel, dim3((unsigned)((p->m + 255) / 256)), dim3(256), 0, s, *p, fit, B, VB);
  return (int)hipGetLastError();
}

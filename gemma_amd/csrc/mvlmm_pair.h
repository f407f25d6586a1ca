// What the host side of the two-trait pair panel and of the null block's standard errors (abi_mvlmm_pairs.inc.h, abi_mvlmm.inc.h)
// needs: the structs of mvlmm_pair.hip.h and the launchers of the kernel units.
#pragma once
#include <hip/hip_runtime.h>

#include "mvlmm_pair.hip.h"

// mvlmm_kernels_pair.hip.  Each returns 0 or a hipError_t.  waves: wavefronts (= pairs) per workgroup, 4 or (any other value) 1.
extern "C" int gemma_hip_mvpair_gather_launch_(const double *Yt, long n, const int *pairs, long m, double *Yp, hipStream_t s);
extern "C" int gemma_hip_mvpair_launch_(const gemma_hip::MvPairArgs *p, int waves, hipStream_t s);
extern "C" int gemma_hip_mvpair_finish_launch_(const gemma_hip::MvPairArgs *p, gemma_hip::MvPairFit *fit, double *B, double *VB, hipStream_t s);
// the null fits with the MvNullSe epilogue: the fixed instances (mvlmm_kernels_null_se.hip; -1: no fixed kernel for (d, c)) and the
// run-time one (mvlmm_kernels_rt.hip).  se: 2 x mv_null_se_doubles(d, c) doubles on the device.
extern "C" int gemma_hip_mvlmm_null_se_launch_(const gemma_hip::MvNullArgs *a, int d, int c, double *se, hipStream_t s);
extern "C" int gemma_hip_mvlmm_null_se_launch_rt_(const gemma_hip::MvNullArgs *a, double *se, hipStream_t s);

// Memory-bound passes of GEMMA's variance-component fit (-vc 1 / -vc 2; VC::CalcVChe src/vc.cpp:1503-1724, UpdateParam /
// LogRL_dev1 / LogRL_dev12 src/vc.cpp:168-380).  Each reads its n x n operands once:
//  (a) vc_assemble_kernel: H = sum_l s_l K_l + s_e I (also the in-place ScaleMatrix, src/mathfunc.cpp:271-286: one K, s = 1 / d);
//  (b) vc_matvec_kernel:   out = M [v_1 .. v_m] for m <= 16 vectors (Kry / K Kry of HE; P y, K Py, P [K Py] of REML);
//  (c) vc_trace_kernel:    tr(A_p B_p) = sum A_p o B_p for every pair p of a set of symmetric matrices (S_ij of HE, tr(P K_i) of REML).
// The centring P_W K P_W (CenterMatrix(G, W), src/mathfunc.cpp:205-247) and the P correction are rank-2c / rank-c updates on the
// fp64 MFMA GEMM (vc_tu.hip).  No floating-point atomics: a wavefront reduces by a fixed butterfly, a workgroup by a fixed tree,
// and the host adds the workgroups' partial sums in workgroup order, so a fit is bit-identical from run to run.
#pragma once
#include <hip/hip_runtime.h>

namespace gemma_hip {

constexpr int VC_MAX_K = 8;       // kinships of one fit
constexpr int VC_MAX_MAT = VC_MAX_K + 1;
constexpr int VC_MAX_PAIRS = 45;  // all pairs i <= j of 9 matrices
constexpr int VC_MAX_VEC = 16;    // vectors of one mat-vec pass
constexpr int VC_TRACE_BLOCKS = 1024;
constexpr int VC_THREADS = 256;

struct VcMats {
  const double *m[VC_MAX_MAT];
  double s[VC_MAX_MAT];
  int count;
};

// the operands of pair p (a matrix met in several pairs is read from HBM once, its repeats come from the caches)
struct VcPairs {
  const double *a[VC_MAX_PAIRS], *b[VC_MAX_PAIRS];
  long lda[VC_MAX_PAIRS], ldb[VC_MAX_PAIRS];
  int count;
};

// out (n x n, ldo) = sum_l s_l K_l + s_e I ; out may be K_0 (in place)
__global__ __launch_bounds__(VC_THREADS) void vc_assemble_kernel(VcMats k, long n, long ld, double s_e, double *out, long ldo) {
  for (long i = blockIdx.x; i < n; i += gridDim.x) {
    for (long j = threadIdx.x; j < n; j += VC_THREADS) {
      double v = (i == j) ? s_e : 0.0;
#pragma unroll
      for (int l = 0; l < VC_MAX_MAT; ++l)
        if (l < k.count) v += k.s[l] * k.m[l][i * ld + j];
      out[i * ldo + j] = v;
    }
  }
}

// out[i * m + v] = sum_k M[i, k] X[k * m + v]: one wavefront per row, lanes across the row, a fixed butterfly at the end
__global__ __launch_bounds__(VC_THREADS) void vc_matvec_kernel(const double *M, long n, long ld, const double *X, int m, double *out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long i = (long)blockIdx.x * (VC_THREADS / 64) + wave;
  if (i >= n) return;
  double acc[VC_MAX_VEC];
#pragma unroll
  for (int v = 0; v < VC_MAX_VEC; ++v) acc[v] = 0.0;
  const double *row = M + i * ld;
  for (long k = lane; k < n; k += 64) {
    const double a = row[k];
#pragma unroll
    for (int v = 0; v < VC_MAX_VEC; ++v)
      if (v < m) acc[v] += a * X[k * m + v];
  }
#pragma unroll
  for (int v = 0; v < VC_MAX_VEC; ++v) {
    if (v < m) {
      double x = acc[v];
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
      acc[v] = x;
    }
  }
  if (lane == 0)
    for (int v = 0; v < m; ++v) out[i * m + v] = acc[v];
}

// partial[block * pairs.count + p] = this workgroup's share of sum_{i,j} A_p[i, j] B_p[i, j] (rows block, block + grid, ...)
__global__ __launch_bounds__(VC_THREADS) void vc_trace_kernel(VcPairs pairs, long n, double *partial) {
  __shared__ double red[VC_THREADS];
  double acc[VC_MAX_PAIRS];
#pragma unroll
  for (int p = 0; p < VC_MAX_PAIRS; ++p) acc[p] = 0.0;
  for (long i = blockIdx.x; i < n; i += gridDim.x) {
    for (long j = threadIdx.x; j < n; j += VC_THREADS) {
#pragma unroll
      for (int p = 0; p < VC_MAX_PAIRS; ++p)
        if (p < pairs.count) acc[p] += pairs.a[p][i * pairs.lda[p] + j] * pairs.b[p][i * pairs.ldb[p] + j];
    }
  }
#pragma unroll
  for (int p = 0; p < VC_MAX_PAIRS; ++p) {
    if (p >= pairs.count) break;
    red[threadIdx.x] = acc[p];
    __syncthreads();
    for (int w = VC_THREADS / 2; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(long)blockIdx.x * pairs.count + p] = red[0];
    __syncthreads();
  }
}

} // namespace gemma_hip

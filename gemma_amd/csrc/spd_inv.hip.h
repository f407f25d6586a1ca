// Inverse of a symmetric positive-definite matrix on gfx950, with its log determinant: the n x n LU inverse of
// H = sum_i sigma_i^2 K_i + sigma_e^2 I that every REML evaluation of GEMMA's variance-component fit takes
// (fast_inverse in UpdateParam, src/vc.cpp:168-258; src/fastblas.cpp fast_inverse = LUDecomp + LUInvert).
//
// Row-major, upper form (A = U^T U, U = L^T: the same factor as a lower Cholesky, stored in the upper triangle, so that the
// trailing update is the kinship's upper-tile SYRK of the fp64 MFMA GEMM):
//  1. blocked Cholesky, NB = 128: spd_diag_kernel factors the 128 x 128 diagonal block resident in LDS (132 KiB of the CU's
//     160 KiB) and inverts its triangle; the panel U_k,r = U_kk^-T A_k,r is one GEMM with that inverse; the trailing update
//     A_rr -= U_k,r^T U_k,r is launch_dgemm's SYRK on the upper tiles (K = 128);                                    n^3 / 3 flop
//  2. V = U^-1 by recursive halving: V12 = -V11 (U12 V22), two GEMMs per split, the 128 x 128 leaves from step 1;   ~2 n^3 / 3
//  3. A^-1 = V V^T by recursive halving on the upper triangle (C11 += V12 V12^T, C12 = V12 V22^T), then the lower triangle
//     mirrored from the upper one;                                                                                    ~n^3 / 3
// The first non-positive (or NaN) pivot stops the factorisation: the host reads the pivot flag after every diagonal block and
// launches nothing further.  log det A = 2 sum log U_jj, summed per block on the device and over blocks on the host in block order
// (every reduction has a fixed order: the inverse is bit-identical from run to run).
// Step 1 also stands alone (spd_chol_blocks), followed by two blocked triangular solves for one right-hand side
// (spd_factor_solve_device, at the end of this file): what the Kronecker system of the kinship-only prediction takes (prdt_mv.hip.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "dgemm.h"

namespace gemma_hip {

constexpr int SPD_NB = 128;
constexpr int SPD_LDS_LD = SPD_NB + 1; // 128 x 129 doubles = 132 096 bytes of LDS
constexpr int SPD_THREADS = 256;

// One workgroup: factor the b x b diagonal block at (k0, k0) of A (its upper triangle is read; b <= 128), write U_kk to A's upper
// triangle and V_kk = U_kk^-1 (upper, zeros below) to V at (k0, k0); logdet_part[k0 / NB] = 2 sum log U_jj.  On a pivot that is not
// > 0, *info = k0 + j + 1 and nothing is written.  vc0: the column of V the block starts at (k0 in the n x n V of the inverse; 0
// where V keeps the diagonal blocks alone, one under the other, as the factor-only form does).
static __global__ __launch_bounds__(SPD_THREADS) void spd_diag_kernel(double *A, long lda, double *V, long ldv, long k0, long vc0, int b,
                                                                       double *logdet_part, int *info) {
  __shared__ double S[SPD_NB * SPD_LDS_LD];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < b * b; idx += SPD_THREADS) {
    const int r = idx / b, c = idx - r * b;
    if (c >= r) S[r * SPD_LDS_LD + c] = A[(k0 + r) * lda + k0 + c];
  }
  // right-looking, one pivot at a time: row j scaled by 1 / sqrt(pivot), rows > j updated by the outer product of row j
  for (int j = 0; j < b; ++j) {
    __syncthreads();
    const double piv = S[j * SPD_LDS_LD + j];
    if (!(piv > 0.0) || !isfinite(piv)) { // uniform: every thread read the same LDS word after the barrier
      if (tid == 0) *info = (int)(k0 + j + 1);
      return;
    }
    const double d = sqrt(piv), rd = 1.0 / d;
    __syncthreads();
    for (int c = j + tid; c < b; c += SPD_THREADS) S[j * SPD_LDS_LD + c] = (c == j) ? d : S[j * SPD_LDS_LD + c] * rd;
    __syncthreads();
    const int m = b - j - 1;
    for (int idx = tid; idx < m * m; idx += SPD_THREADS) {
      const int r = j + 1 + idx / m, c = j + 1 + idx % m;
      if (c >= r) S[r * SPD_LDS_LD + c] -= S[j * SPD_LDS_LD + r] * S[j * SPD_LDS_LD + c];
    }
  }
  __syncthreads();
  if (tid == 0) {
    double ld = 0.0;
    for (int j = 0; j < b; ++j) ld += log(S[j * SPD_LDS_LD + j]);
    logdet_part[k0 / SPD_NB] = 2.0 * ld;
  }
  // V = U^-1, column c by thread c (back substitution); V_ic (i < c) is kept in the free strict lower triangle at S[c][i], which
  // only thread c writes and reads
  if (tid < b) {
    const int c = tid;
    const double vcc = 1.0 / S[c * SPD_LDS_LD + c];
    for (int i = c - 1; i >= 0; --i) {
      double s = S[i * SPD_LDS_LD + c] * vcc;
      for (int k = i + 1; k < c; ++k) s += S[i * SPD_LDS_LD + k] * S[c * SPD_LDS_LD + k];
      S[c * SPD_LDS_LD + i] = -s / S[i * SPD_LDS_LD + i];
    }
  }
  __syncthreads();
  for (int idx = tid; idx < b * b; idx += SPD_THREADS) {
    const int r = idx / b, c = idx - r * b;
    double v = 0.0;
    if (c > r) v = S[c * SPD_LDS_LD + r];
    else if (c == r) v = 1.0 / S[r * SPD_LDS_LD + r];
    V[(k0 + r) * ldv + vc0 + c] = v;
    if (c >= r) A[(k0 + r) * lda + k0 + c] = S[r * SPD_LDS_LD + c];
  }
}

// Workspace of one inversion of order n: V (n x ld), the panel (NB x ld), the split scratch of step 2 (ceil(n/2) x ld), the pivot
// flag and the per-block log determinants; kept between calls of the same or a smaller order.
struct SpdWork {
  double *V = nullptr, *P = nullptr, *T = nullptr, *ldp = nullptr;
  int *info = nullptr;
  long n = 0, ld = 0;
  size_t bytes = 0;
  int reserve(long n_, std::string &msg) {
    const long ld_ = (n_ + 1) & ~1L; // even: 16-byte aligned rows for the GEMM's fast path
    if (V && n_ <= n && ld_ <= ld) return 0;
    release();
    const long nblk = (n_ + SPD_NB - 1) / SPD_NB, half = ((nblk + 1) / 2) * SPD_NB;
    const size_t bv = (size_t)n_ * ld_ * 8, bp = (size_t)SPD_NB * ld_ * 8, bt = (size_t)half * ld_ * 8;
    if (hipMalloc((void **)&V, bv) != hipSuccess || hipMalloc((void **)&P, bp) != hipSuccess ||
        hipMalloc((void **)&T, bt) != hipSuccess || hipMalloc((void **)&ldp, nblk * 8) != hipSuccess ||
        hipMalloc((void **)&info, 8) != hipSuccess) {
      (void)hipGetLastError();
      release();
      msg = "spd_inverse: cannot allocate the workspace of order " + std::to_string(n_);
      return 3; // GEMMA_HIP_ENOMEM
    }
    n = n_;
    ld = ld_;
    bytes = bv + bp + bt + nblk * 8 + 8;
    return 0;
  }
  void release() {
    if (V) (void)hipFree(V);
    if (P) (void)hipFree(P);
    if (T) (void)hipFree(T);
    if (ldp) (void)hipFree(ldp);
    if (info) (void)hipFree(info);
    V = P = T = ldp = nullptr;
    info = nullptr;
    n = ld = 0;
    bytes = 0;
  }
};

// step 2 on the block range [a, c) (a a multiple of NB): V[a:c, a:c] = U[a:c, a:c]^-1 given the diagonal blocks of V
static inline hipError_t spd_trtri_rec(const double *U, long lda, double *V, long ldv, double *T, long a, long c, hipStream_t s) {
  const long nb = (c - a + SPD_NB - 1) / SPD_NB;
  if (nb <= 1) return hipSuccess;
  const long mid = a + (nb / 2) * SPD_NB, h1 = mid - a, h2 = c - mid;
  hipError_t e;
  if ((e = spd_trtri_rec(U, lda, V, ldv, T, a, mid, s)) != hipSuccess) return e;
  if ((e = spd_trtri_rec(U, lda, V, ldv, T, mid, c, s)) != hipSuccess) return e;
  // T = U12 V22 (h1 x h2); V12 = -V11 T.  V's blocks below the diagonal are zero, so the dense products are exact.
  if ((e = launch_dgemm('N', 'N', h1, h2, h2, 1.0, U + a * lda + mid, lda, V + mid * ldv + mid, ldv, 0.0, T, ldv, false, false, s)) !=
      hipSuccess)
    return e;
  return launch_dgemm('N', 'N', h1, h2, h1, -1.0, V + a * ldv + a, ldv, T, ldv, 0.0, V + a * ldv + mid, ldv, false, false, s);
}

// step 3 on the block range [a, c): the upper triangle of C[a:c, a:c] = V[a:c, a:c] V[a:c, a:c]^T (V upper), recursively:
// C11 = V11 V11^T + V12 V12^T (upper-tile SYRK), C12 = V12 V22^T, C22 = V22 V22^T -- n^3 / 3 flop where the dense product takes n^3
static inline hipError_t spd_lauum_rec(const double *V, long ldv, double *C, long ldc, long a, long c, hipStream_t s) {
  const long nb = (c - a + SPD_NB - 1) / SPD_NB;
  hipError_t e;
  if (nb <= 1)
    return launch_dgemm('N', 'T', c - a, c - a, c - a, 1.0, V + a * ldv + a, ldv, V + a * ldv + a, ldv, 0.0, C + a * ldc + a, ldc,
                        false, false, s);
  const long mid = a + (nb / 2) * SPD_NB, h1 = mid - a, h2 = c - mid;
  if ((e = spd_lauum_rec(V, ldv, C, ldc, a, mid, s)) != hipSuccess) return e;
  if ((e = spd_lauum_rec(V, ldv, C, ldc, mid, c, s)) != hipSuccess) return e;
  if ((e = launch_dgemm('N', 'T', h1, h1, h2, 1.0, V + a * ldv + mid, ldv, V + a * ldv + mid, ldv, 1.0, C + a * ldc + a, ldc, true,
                        false, s)) != hipSuccess)
    return e;
  return launch_dgemm('N', 'T', h1, h2, h2, 1.0, V + a * ldv + mid, ldv, V + mid * ldv + mid, ldv, 0.0, C + a * ldc + mid, ldc, false,
                      false, s);
}

// Step 1 alone: the blocked Cholesky A = U^T U in A's upper triangle.  V (ld ldv) receives the inverted diagonal triangles: at
// (k0, k0) of an n x n matrix, or with v_diag_only at (k0, 0) of an n x NB one (ldv = NB).  P: the panel, NB rows of ld ldp.
// Returns 0 with e = the first HIP error (hipSuccess: the factor is complete), or 7 with *bad_pivot and msg ("<who>: ...").
static inline int spd_chol_blocks(double *A, long n, long lda, double *V, long ldv, bool v_diag_only, double *P, long ldp, double *ldpart,
                                  int *info_d, long *bad_pivot, const char *who, hipStream_t s, std::string &msg, hipError_t &e) {
  e = hipMemsetAsync(info_d, 0, sizeof(int), s);
  for (long k0 = 0; k0 < n && e == hipSuccess; k0 += SPD_NB) {
    const int b = (int)std::min<long>(SPD_NB, n - k0);
    const long vc0 = v_diag_only ? 0 : k0;
    hipLaunchKernelGGL(spd_diag_kernel, dim3(1), dim3(SPD_THREADS), 0, s, A, lda, V, ldv, k0, vc0, b, ldpart, info_d);
    int info = 0;
    if ((e = hipGetLastError()) != hipSuccess) break;
    if ((e = hipMemcpyAsync(&info, info_d, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess) break;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) break;
    if (info) {
      if (bad_pivot) *bad_pivot = info - 1;
      msg = std::string(who) + ": the matrix is not positive definite (pivot " + std::to_string(info - 1) + " of " + std::to_string(n) +
            " is not > 0)";
      return 7;
    }
    const long m = n - k0 - b;
    if (m == 0) break;
    double *Akr = A + k0 * lda + k0 + b;
    // panel: P = V_kk^T A_k,r  (b x m), then back into A's block row
    if ((e = launch_dgemm('T', 'N', b, m, b, 1.0, V + k0 * ldv + vc0, ldv, Akr, lda, 0.0, P, ldp, false, false, s)) != hipSuccess) break;
    if ((e = hipMemcpy2DAsync(Akr, lda * 8, P, ldp * 8, m * 8, b, hipMemcpyDeviceToDevice, s)) != hipSuccess) break;
    // trailing: A_rr -= P^T P on the upper tiles
    e = launch_dgemm('T', 'N', m, m, b, -1.0, P, ldp, P, ldp, 1.0, A + (k0 + b) * lda + k0 + b, lda, true, false, s);
  }
  return 0;
}

// A (n x n, ld lda even, 16-byte aligned, device; upper triangle read) -> A^-1 (full), *logdet.  Returns 0, or 7
// (GEMMA_HIP_ENOTPD) with *bad_pivot = the 0-based index of the first non-positive pivot, or 4 (ERUNTIME) with msg.
static inline int spd_inverse_device(double *A, long n, long lda, double *logdet, long *bad_pivot, SpdWork &w, hipStream_t s,
                                     std::string &msg) {
  int rc = w.reserve(n, msg);
  if (rc) return rc;
  const long ldv = w.ld, nblk = (n + SPD_NB - 1) / SPD_NB;
  hipError_t e = hipMemsetAsync(w.V, 0, (size_t)n * ldv * 8, s);
  if (e == hipSuccess && (rc = spd_chol_blocks(A, n, lda, w.V, ldv, false, w.P, ldv, w.ldp, w.info, bad_pivot, "spd_inverse", s, msg, e)))
    return rc;
  if (e == hipSuccess) e = spd_trtri_rec(A, lda, w.V, ldv, w.T, 0, n, s);
  if (e == hipSuccess) e = spd_lauum_rec(w.V, ldv, A, lda, 0, n, s);
  if (e == hipSuccess) { // the upper triangle mirrored into the lower one
    hipLaunchKernelGGL(symm_fill_scale_kernel, dim3((unsigned)((n + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, A, n, lda,
                       1.0);
    e = hipGetLastError();
  }
  std::vector<double> part(nblk);
  if (e == hipSuccess) e = hipMemcpyAsync(part.data(), w.ldp, nblk * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    msg = std::string("spd_inverse: ") + hipGetErrorString(e);
    return 4;
  }
  double ld = 0.0;
  for (long k = 0; k < nblk; ++k) ld += part[k];
  if (logdet) *logdet = ld;
  return 0;
}

// ------------------------------------------------------------------------------------------------ factor + solve
// A x = r for ONE right-hand side without the inverse: step 1 above (n^3 / 3 flop), then U^T w = r and U x = w block by block
// (2 n^2 flop, each a pass over the factor's upper triangle).  spd_diag_kernel leaves the inverted 128 x 128 diagonal triangles, so a
// diagonal step is a triangular matrix-vector product (spd_trmv_kernel); the off-diagonal steps are matrix-vector products of a
// 128-row block row of U with kernels of their own: the fp64 MFMA GEMM at n = 1 would fill one column of its 128-wide tiles.
// Every sum has a fixed order: the solution is bit-identical from run to run.

// x_k <- V_kk^T x_k (trans) or V_kk x_k: V_kk b x b upper with zeros below, ld SPD_NB.  One workgroup.
static __global__ __launch_bounds__(SPD_THREADS) void spd_trmv_kernel(const double *Vkk, int b, int trans, double *x) {
  __shared__ double t[SPD_NB];
  const int tid = threadIdx.x;
  if (tid < b) t[tid] = x[tid];
  __syncthreads();
  if (trans) { // column c by thread c: the loads of one r are contiguous over the threads
    if (tid < b) {
      double s = 0.0;
      for (int r = 0; r <= tid; ++r) s += Vkk[r * SPD_NB + tid] * t[r];
      x[tid] = s;
    }
  } else { // row r by a wavefront, the lanes along the row
    const int lane = tid & 63;
    for (int r = tid >> 6; r < b; r += SPD_THREADS / 64) {
      double s = 0.0;
      for (int c = r + lane; c < b; c += 64) s += Vkk[r * SPD_NB + c] * t[c];
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) x[r] = s;
    }
  }
}

// forward, right-looking: x[c] -= sum_r U[k0 + r][c] w[r] for the columns c >= k0 + b, w = x[k0 .. k0 + b).  One thread per column.
static __global__ __launch_bounds__(SPD_THREADS) void spd_fwd_update_kernel(const double *U, long lda, long n, long k0, int b, double *x) {
  __shared__ double w[SPD_NB];
  if ((int)threadIdx.x < b) w[threadIdx.x] = x[k0 + threadIdx.x];
  __syncthreads();
  const long c = k0 + b + (long)blockIdx.x * SPD_THREADS + threadIdx.x;
  if (c >= n) return;
  const double *u = U + k0 * lda + c;
  double s = 0.0;
  for (int r = 0; r < b; ++r) s += u[(long)r * lda] * w[r];
  x[c] -= s;
}

// backward, left-looking: x[k0 + r] -= sum_{c >= k0 + b} U[k0 + r][c] x[c].  One workgroup per row r of the block.
static __global__ __launch_bounds__(SPD_THREADS) void spd_bwd_update_kernel(const double *U, long lda, long n, long k0, int b, double *x) {
  __shared__ double red[SPD_THREADS / 64];
  const long r = k0 + blockIdx.x;
  const double *u = U + r * lda;
  double s = 0.0;
  for (long c = k0 + b + threadIdx.x; c < n; c += SPD_THREADS) s += u[c] * x[c];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) x[r] -= ((red[0] + red[1]) + red[2]) + red[3];
}

// Workspace of one factorisation of order n: the inverted diagonal triangles (n x NB), the panel (NB x ld), the pivot flag and the
// per-block log determinants -- (2 NB + 1) n doubles, where the inverse keeps 1.5 n^2.
struct SpdFactorWork {
  double *Vd = nullptr, *P = nullptr, *ldp = nullptr;
  int *info = nullptr;
  long n = 0, ld = 0;
  int reserve(long n_, std::string &msg) {
    const long ld_ = (n_ + 1) & ~1L;
    if (Vd && n_ <= n) return 0;
    release();
    const long nblk = (n_ + SPD_NB - 1) / SPD_NB;
    if (hipMalloc((void **)&Vd, (size_t)nblk * SPD_NB * SPD_NB * 8) != hipSuccess ||
        hipMalloc((void **)&P, (size_t)SPD_NB * ld_ * 8) != hipSuccess || hipMalloc((void **)&ldp, nblk * 8) != hipSuccess ||
        hipMalloc((void **)&info, 8) != hipSuccess) {
      (void)hipGetLastError();
      release();
      msg = "spd_factor: cannot allocate the workspace of order " + std::to_string(n_);
      return 3; // GEMMA_HIP_ENOMEM
    }
    n = n_;
    ld = ld_;
    return 0;
  }
  void release() {
    if (Vd) (void)hipFree(Vd);
    if (P) (void)hipFree(P);
    if (ldp) (void)hipFree(ldp);
    if (info) (void)hipFree(info);
    Vd = P = ldp = nullptr;
    info = nullptr;
    n = ld = 0;
  }
};

// A (n x n, lda, device; upper triangle read) -> its factor U in the upper triangle (what lies below the diagonal of the diagonal
// tiles is scratch), x (n, device): the right-hand side in, the solution out.  Returns as spd_inverse_device does.
static inline int spd_factor_solve_device(double *A, long n, long lda, double *x, double *logdet, long *bad_pivot, SpdFactorWork &w,
                                          const char *who, hipStream_t s, std::string &msg) {
  int rc = w.reserve(n, msg);
  if (rc) return rc;
  const long nblk = (n + SPD_NB - 1) / SPD_NB;
  hipError_t e;
  if ((rc = spd_chol_blocks(A, n, lda, w.Vd, SPD_NB, true, w.P, w.ld, w.ldp, w.info, bad_pivot, who, s, msg, e))) return rc;
  for (long k0 = 0; k0 < n && e == hipSuccess; k0 += SPD_NB) { // U^T w = r
    const int b = (int)std::min<long>(SPD_NB, n - k0);
    hipLaunchKernelGGL(spd_trmv_kernel, dim3(1), dim3(SPD_THREADS), 0, s, w.Vd + k0 * SPD_NB, b, 1, x + k0);
    const long m = n - k0 - b;
    if (m > 0)
      hipLaunchKernelGGL(spd_fwd_update_kernel, dim3((unsigned)((m + SPD_THREADS - 1) / SPD_THREADS)), dim3(SPD_THREADS), 0, s, A, lda, n,
                         k0, b, x);
    e = hipGetLastError();
  }
  for (long k = nblk - 1; k >= 0 && e == hipSuccess; --k) { // U x = w
    const long k0 = k * SPD_NB;
    const int b = (int)std::min<long>(SPD_NB, n - k0);
    if (n - k0 - b > 0) hipLaunchKernelGGL(spd_bwd_update_kernel, dim3((unsigned)b), dim3(SPD_THREADS), 0, s, A, lda, n, k0, b, x);
    hipLaunchKernelGGL(spd_trmv_kernel, dim3(1), dim3(SPD_THREADS), 0, s, w.Vd + k0 * SPD_NB, b, 0, x + k0);
    e = hipGetLastError();
  }
  std::vector<double> part(nblk);
  if (e == hipSuccess) e = hipMemcpyAsync(part.data(), w.ldp, nblk * 8, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    msg = std::string(who) + ": " + hipGetErrorString(e);
    return 4;
  }
  double ld = 0.0;
  for (long k = 0; k < nblk; ++k) ld += part[k];
  if (logdet) *logdet = ld;
  return 0;
}

} // namespace gemma_hip

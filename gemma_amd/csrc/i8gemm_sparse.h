// What the host side of i8gemm_sparse.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in i8gemm_sparse.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "i8gemm.h"

namespace gemma_hip {

typedef int i32x8 __attribute__((ext_vector_type(8)));
constexpr int SP_STAGE = I8P_STAGE + 4096; // operands + the mask words of 128 rows (32 bytes each)

struct SparseMeta {
  const uint4 *m4;   // [row][tile][h]: {idx pair 0, bits pair 0, idx pair 1, bits pair 1} of K-steps 2 p + h
  int *row_surplus;  // per row: number of calls the sparse operand drops (0 for almost every row)
  long ntiles;
};

__global__ __launch_bounds__(256) void sparse_meta_kernel(const int8_t *__restrict__ A, long lpad, long ldk, uint4 *__restrict__ m4,
                                                          int *__restrict__ row_surplus);

static inline int sparse_meta_build(const int8_t *A, long lpad, long ldk, SparseMeta *sm) {
  const long nk = ldk / I8_BK, total = lpad * nk * 2;
  uint4 *m4 = nullptr;
  int *rs = nullptr;
  if (hipMalloc(reinterpret_cast<void **>(&m4), (size_t)total * sizeof(uint4)) != hipSuccess ||
      hipMalloc(reinterpret_cast<void **>(&rs), (size_t)lpad * sizeof(int)) != hipSuccess)
    return 1;
  (void)hipMemset(rs, 0, (size_t)lpad * sizeof(int));
  hipLaunchKernelGGL(sparse_meta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, 0, A, lpad, ldk, m4, rs);
  sm->m4 = m4;
  sm->row_surplus = rs;
  sm->ntiles = nk;
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

// Where the surplus kernels read a row's missing pattern: bit q of pat(s, gq) = call q of group gq (individuals 4 gq .. 4 gq + 3)
// of row s is missing.  SurplusBytes: the packed byte matrix (byte = g | m << 4).  SurplusPlink: the 2-bit PLINK rows themselves
// (code 1 = missing; calls n .. are none), for blocks whose records came from plink_records_kernel and have no byte matrix.
struct SurplusBytes {
  const int8_t *A;
  long ldk;
  __device__ __forceinline__ unsigned pat(long s, long gq) const {
    const unsigned word = *reinterpret_cast<const unsigned *>(A + s * ldk + 4 * gq);
    const unsigned m = (word >> 4) & 0x01010101u;
    return (m | (m >> 7) | (m >> 14) | (m >> 21)) & 0xFu;
  }
};
struct SurplusPlink {
  const unsigned char *src;
  long ld, n;
  __device__ __forceinline__ unsigned pat(long s, long gq) const {
    const long left = n - 4 * gq;
    if (left <= 0) return 0u;
    const unsigned b = src[s * ld + gq];
    const unsigned m = b & ~(b >> 1) & 0x55u; // code 01 at bits 2 q
    const unsigned p = (m & 1u) | ((m >> 1) & 2u) | ((m >> 2) & 4u) | ((m >> 3) & 8u);
    return left >= 4 ? p : p & ((1u << left) - 1u);
  }
};

template <class Src>
__global__ __launch_bounds__(256) void i8_surplus_fix_kernel(Src src, long ldk,
                                                             const int *__restrict__ row_surplus,
                                                             const double *__restrict__ mean, const double *__restrict__ U,
                                                             long ldu, long n, long l, double *__restrict__ UtX, long ldx,
                                                             int skip_upto);

// The dropped calls of a row as a short list, so that the digit combine can add them in the same pass (a pass of its own over
// the fp64 rows costs 4.7 ms per 20 000-SNP block at 5 % missingness, where every row has two or three of them): one wavefront
// per row with row_surplus > 0 scans the row's groups of four in order and writes the first SUR_MAX dropped individuals to
// sur_list[row][..] (group order: deterministic), the count to sur_cnt[row]; a row with more (a SNP missing for most
// individuals) keeps cnt = -1 and is left to i8_surplus_fix_kernel.
static_assert(SUR_MAX >= 2, "SUR_MAX (i8gemm.hip.h) is the list stride of this kernel, of i8_combine_kernel and of the host's buffers");

template <class Src>
__global__ __launch_bounds__(256) void i8_surplus_list_kernel(Src src, long ldk, const int *__restrict__ row_surplus,
                                                             long l, int *__restrict__ sur_cnt, int *__restrict__ sur_list);

__global__ __launch_bounds__(256) void i8_surplus_short_kernel(const int *__restrict__ sur_cnt, const int *__restrict__ sur_list,
                                                               const double *__restrict__ mean, const double *__restrict__ U,
                                                               long ldu, long n, long l, double *__restrict__ UtX, long ldx);

__global__ __launch_bounds__(512, 2) void i8gemm_sparse_kernel(I8PackArgs g, SparseMeta sm);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define I8GEMM_SPARSE_INSTANCES(T) \
  T void i8_surplus_fix_kernel<SurplusBytes>(SurplusBytes, long, const int *, const double *, const double *, long, long, long, double *, long, int); \
  T void i8_surplus_fix_kernel<SurplusPlink>(SurplusPlink, long, const int *, const double *, const double *, long, long, long, double *, long, int); \
  T void i8_surplus_list_kernel<SurplusBytes>(SurplusBytes, long, const int *, long, int *, int *); \
  T void i8_surplus_list_kernel<SurplusPlink>(SurplusPlink, long, const int *, long, int *, int *);
#ifndef GEMMA_HIP_KERNEL_BODIES
I8GEMM_SPARSE_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

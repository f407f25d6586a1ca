// The fp64 MFMA GEMM as the other units see it: the launchers, the side stream, the tile constants.  The kernels are in
// dgemm_mfma.hip.h and exist once, in dgemm_tu.hip -- as do the side stream and the caches of the GEMMA_HIP_GEMM_* switches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace gemma_hip {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void *gemma_gptr_t;
typedef __attribute__((address_space(3))) void *gemma_lptr_t;
#define GEMMA_SB() __builtin_amdgcn_sched_barrier(0)

constexpr int GEMM_BM = 128, GEMM_BN = 128, GEMM_BK = 16;
constexpr int GEMM_LD_KM = 144; // [k][m] image: row stride in doubles
constexpr int GEMM_LD_MK = 18;  // [m][k] image: row stride in doubles
constexpr int GEMM_TILE_DOUBLES = 2304; // 16*144 == 128*18
constexpr int GEMM_THREADS = 256;

// Optional side stream for the ragged edge strips: they are tiny launches (<= 2 x 157 blocks at n = 20000)
// that would otherwise run alone after the main grid; on a second stream they fill the main grid's tail.
// One per process: gemma_hip_init creates it, gemma_hip_shutdown destroys it (eigh2.hip.h borrows the stream and the events).
struct GemmAux {
  hipStream_t stream = nullptr;
  hipEvent_t ready = nullptr, done = nullptr;
};
extern GemmAux g_gemm_aux;
void gemm_aux_init();
void gemm_aux_destroy();

// ta/tb in {'N','T'} with the cblas row-major meaning; mirror (with syrk_upper, M == N): the lower triangle is written too, as the
// transpose of the upper tiles (GemmArgs::mirror)
hipError_t launch_dgemm(char ta, char tb, long M, long N, long K, double alpha, const double *A, long lda, const double *B, long ldb,
                        double beta, double *C, long ldc, bool syrk_upper, bool square_a, hipStream_t s, bool mirror = false);

// How K is cut for launch_dgemm_ksliced: K0 = the part that is whole K-tiles, `per` = length of a slice (a multiple of the K-tile),
// return = number of slices: every slice is non-empty ((ns - 1) per < K0 <= ns per) and -- when more than one -- at least four K-tiles
// long except possibly the last.  1 means "do not slice".  (tests/cpp/raster_slices_check.hip runs this for every K <= 40 000.)
static inline int gemm_kslice_plan(long K, int want, long *K0, long *per) {
  *K0 = (K / GEMM_BK) * GEMM_BK;
  *per = *K0;
  int ns = want < 1 ? 1 : want;
  while (ns > 1 && *K0 / ns < 4 * GEMM_BK) --ns;
  if (ns <= 1 || *K0 == 0) return 1;
  const long kt = *K0 / GEMM_BK, pt = (kt + ns - 1) / ns; // K-tiles in all, per slice
  ns = (int)((kt + pt - 1) / pt);
  *per = pt * GEMM_BK;
  return ns;
}

// C_ks (ks = 0 .. *nslices - 1, at C + ks * cslice) = alpha op(A) op(B) over the K range of slice ks; see dgemm_tu.hip
hipError_t launch_dgemm_ksliced(char ta, char tb, long M, long N, long K, double alpha, const double *A, long lda, const double *B,
                                long ldb, double *C, long ldc, long cslice, int want, int *nslices, hipStream_t s);

// mirror the strict upper triangle into the lower one and scale everything (grid: n / 32 x n / 32 tiles, block 32 x 8)
__global__ void symm_fill_scale_kernel(double *K, long n, long ld, double scale);

} // namespace gemma_hip

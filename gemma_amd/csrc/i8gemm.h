// What the host side of i8gemm.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in i8gemm.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include "dgemm.h"
#include "ingest.h"

namespace gemma_hip {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int I8_BM = 256, I8_BN = 256, I8_BK = 128;
constexpr int I8_DIGITS = 7;      // most digits a build handles (buffers are sized for it)
constexpr int SUR_MAX = 16;       // calls per row the sparse mask operand may drop before the row goes to the fp64 fix-up: the stride of
                                  // the dropped-call lists, shared by the list kernel (i8gemm_sparse.hip.h), the combine below and the host
constexpr int I8_SCALE_BITS = 54;  // with 7 digits; D digits scale to 8 D - 2 bits (|V| <= 2^(8D-2) < 128 * 256^(D-1))
// Digits actually used (host: i8_digits_for): 7 round U at 2^-56 of each column's maximum.  From n = 16384 up 6 digits are used: U is
// then rounded at 2^-48 of the column maximum, which perturbs a dot product by cmax |x|_2 / (0.99 * 2^47 * sqrt(12)) -- measured against
// long-double products 1.66e-16 rms in units of sum_k |x_k||u_k| (the fp64 MFMA GEMM: 3.6e-17), 4.6 x the GEMM's, for 6/7 of the
// matrix-pipe cycles; GEMMA_HIP_I8_FORM=7g6m (seven digits for the genotype product, six for the mask product) is below the GEMM's
// (tests/test_gpu_at_size.py::test_six_digit_rounding_of_U_is_what_the_model_says).  i8_scale_bits: the power-of-two scale of rounds 1-5.
__host__ __device__ inline int i8_scale_bits(int digits) { return 8 * digits - 2; }

// ---------------------------------------------------------------------------------------------------------------
// ONE packed left factor per SNP row, byte = g | (m << 4).  A wave reads an A fragment from LDS once and
// masks it into the genotype operand (a & 0x03) and the missing-mask operand ((a >> 4) & 0x01) -- the G and M
// products share every global / LDS byte of both operands, so LDS traffic per MFMA drops by a third and the left
// factor is read once.  Two digits of U are fused per output plane where 256 * C_{d+1} + C_d still fits int32
// (n <= 32640): the K loop runs for the upper digit, the accumulators are shifted left by 8, and it runs again for
// the lower digit -- 4 int32 planes leave the kernel instead of 7.
//   tile 128 SNP rows x 256 columns x 128 K bytes; 8 wavefronts (2 x 4), wave tile 64 x 64 for G and for M
//   (2 x 2 x 2 blocks of 32 x 32 = 128 int32 accumulators); three LDS stages of 48 KiB (A 16 KiB + B 32 KiB), LDS-DMA
//   two K-tiles ahead with a counted vmcnt and a raw s_barrier; pinned issue order: one ds_read_b128 / LDS-DMA piece /
//   pair of v_and behind each MFMA, fragments one K-step ahead, the barrier after MFMA 25 of 32 so that the next
//   tile's first fragments are already there when this tile ends.
struct I8PackArgs {
  const int8_t *A;   // lpad x ldk packed bytes
  const int8_t *Bt;  // digit d: N x ldk
  int *C;            // plane q: (2 lpad) x ldc; rows [0, lpad) = G products, [lpad, 2 lpad) = M products
  long ldk, ldc;
  long strideB, strideC;
  long m_row0;       // lpad
  int tiles_m, tiles_n;
  int nk;
  int gm;
  int fuse;          // 1: two digits per output plane (needs n * 2 * 128 * 257 < 2^31): 7 digits -> planes {0}, {2,1},
                     // {4,3}, {6,5}; 6 digits -> {1,0}, {3,2}, {5,4};  0: one plane per digit
  int digits;        // 6 or 7
  const int *tile_map = nullptr; // (tile_m, tile_n) per linear tile index when only some tiles are wanted (the symmetric
                                 // product of kin_i8.hip.h: tiles that meet the upper triangle); the grid has that many blocks
};
constexpr int I8P_BM = 128;
constexpr int I8P_STAGE = 49152;

template <bool WITH_M, bool RAW = false>
__global__ __launch_bounds__(512, 2) void i8gemm_packed_kernel_t(I8PackArgs g);

__global__ __launch_bounds__(256) void u_colmax_kernel(const double *__restrict__ U, long n, long ld,
                                                       unsigned long long *__restrict__ colmax_bits);

__global__ void u_scale_kernel(const unsigned long long *__restrict__ colmax_bits, long n, int digits, int exact_max,
                               double *__restrict__ q, double *__restrict__ qinv);

__global__ __launch_bounds__(256) void u_digits_kernel(const double *__restrict__ U, long n, long ld,
                                                       const double *__restrict__ q, int8_t *__restrict__ Bt, long ldk,
                                                       long strideB, int digits);

// ---------------------------------------------------------------------------------------------------------------
// PLINK rows -> packed left factor rows (byte = g | m << 4) and mean_s
struct IngestI8Args {
  const unsigned char *src;
  long ld, l;
  const int *idx_map;
  int n;
  int8_t *A;  // l x ldk, byte = g | (m << 4)
  long ldk;
  double *mean;
};

__global__ __launch_bounds__(256) void ingest_i8_kernel(IngestI8Args g);

// fp64 SNP-major rows (BIMBAM / the reference's Xlarge after transposition) -> packed left factor, when the row is a
// hard-call row: every value is 0, 1 or 2 except one repeated "other" value.  nan_missing = 1: the other value must be
// NaN (missing; mean_s = sum / count of the calls, as ingest_lmm_kernel); nan_missing = 0: the input is already
// mean-imputed (src/lmm.cpp:1590-1618) and the other value must be ONE finite number v (mean_s = v, bit for bit).
// Any row that is not of that form clears *all_hard (the batch then takes the fp64 GEMM).
struct PackF64Args {
  const double *src; // l x ld
  long ld, l;
  int n;
  int nan_missing;
  int8_t *A;
  long ldk;
  double *mean;
  int *all_hard; // [0] every row is a hard-call row; [1] every row is a fixed-point dosage row with 3 decimals (values k / 1000
                 // in [0, 2], plus the missing marker: NaN, or with nan_missing = 0 one repeated other value); [2] ... with 2
                 // decimals (k / 100); [3] set when any row has a missing entry
};

__global__ __launch_bounds__(256) void pack_f64_kernel(PackF64Args g);

// ---------------------------------------------------------------------------------------------------------------
// Fixed-point dosages (BIMBAM mean genotypes: "0.98, 0.04, 1.00", doc/manual.tex:398-404) on the int8 pipe.  With scale S = 100
// or 1000 a dosage is x = 1 + q' / S, q' = round(S x) - S in [-S, S]: ONE signed byte for S = 100, two balanced base-256 bytes
// for S = 1000 (q' = 256 a1 + a0).  With m the 0/1 mask of missing entries (q' = 0 there) and mean_s the SNP's mean,
//     (U^T x_s)[j] = ( sum_k q'_sk U[k][j] ) / S  +  sum_k U[k][j]  +  (mean_s - 1) sum_k m_sk U[k][j]:
// integer left factors again, one dense int8 product per byte plane and digit of U, the column sums of U once per setup
// (from the same digits).  The products run on i8gemm_packed_kernel_t<false, true>, one int32 plane per digit (|sum| <=
// 128 * 128 * n does not leave room to fuse two).
struct PackDosageArgs {
  const double *src; // l x ld
  long ld, l;
  int n;
  int nan_missing, two; // two: S = 1000 (planes a0, a1), else S = 100 (plane a0)
  int8_t *A0, *A1, *Am; // l x ldk each; Am may be null when the batch has no missing entry
  long ldk;
  double *mean;         // nan_missing: mean of the present entries; else the row's off-grid value (or 1.0 when it has none)
};

__global__ __launch_bounds__(256) void pack_dosage_kernel(PackDosageArgs g);

__global__ __launch_bounds__(256) void u_digit_colsum_kernel(const int8_t *__restrict__ Bt, long ldk, long strideB,
                                                             const double *__restrict__ qinv, long n, int digits,
                                                             double *__restrict__ colsum);

__global__ __launch_bounds__(256) void i8_combine_dosage_kernel(const int *__restrict__ C, long ldc, long strideC,
                                                                const double *__restrict__ mean, const double *__restrict__ qinv,
                                                                const double *__restrict__ colsum, long l, long n,
                                                                double *__restrict__ UtX, long ldx, int digits, int two,
                                                                int have_m, double inv_scale_is_S);

__global__ __launch_bounds__(256) void i8_combine_kernel(const int *__restrict__ C, long ldc, long strideC, long m_row0,
                                                         const double *__restrict__ mean, const double *__restrict__ qinv,
                                                         long l, long n, double *__restrict__ UtX, long ldx,
                                                         double m_scale, int fuse, int digits,
                                                         const int *__restrict__ sur_cnt = nullptr,
                                                         const int *__restrict__ sur_list = nullptr,
                                                         const double *__restrict__ U = nullptr, long ldu = 0,
                                                         int m_skip0 = 0 /* 1: plane 0 carries no mask product (7g6m) */,
                                                         const int *__restrict__ anymiss = nullptr /* Sparse2Args::anymiss: 0 = no
                                                         plane of this block carries one (their M rows were not written) */);

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define I8GEMM_INSTANCES(T) \
  T void i8gemm_packed_kernel_t<false, false>(I8PackArgs); \
  T void i8gemm_packed_kernel_t<false, true>(I8PackArgs); \
  T void i8gemm_packed_kernel_t<true, false>(I8PackArgs);
#ifndef GEMMA_HIP_KERNEL_BODIES
I8GEMM_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

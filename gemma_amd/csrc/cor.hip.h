// Kernels of the windowed SNP correlation (GEMMA -calccor, a_mode 71; VARCOV::AnalyzePlink / AnalyzeBimbam + Calc_Cor,
// src/varcov.cpp:220-446), gfx950.  With c the 0/1 "called" mask, g the genotype (0 where missing) and mu = sum g / sum c, the
// reference's column is x = c (g - mu) (Plink_ReadOneSNP / Bimbam_ReadOneSNP, src/gemma_io.cpp:1069-1184, then the centring of
// src/varcov.cpp:308 / :408), and a record is var_t = x_t.x_t / n, cor_{t,k} = x_t.x_{t+k} / sqrt((x_t.x_t)(x_{t+k}.x_{t+k})).
//
//   hard calls   ingest: SNP-major K-contiguous int8 rows of g and of c (K padding 0 in BOTH planes: a padded individual is "not
//                called"), and per SNP the integers N = sum c, S = sum g, S2 = sum g^2.
//                band: one workgroup per (row tile, column tile) pair of 64 x 64 SNPs from a list; the four products
//                P1 = sum g_a g_b, P2 = sum c_a g_b, P3 = sum g_a c_b, P4 = sum c_a c_b on v_mfma_i32_16x16x64_i8, exact in int32;
//                a pair of tiles without a missing call runs P1 alone (P2 = S_b, P3 = S_a, P4 = n).  The epilogue combines in int64
//                before any rounding and stores straight into the ragged output; no int32 product reaches memory.
//   dosages      ingest: mean, impute, centre, own sum of squares in fp64; the band panels come from the fp64 MFMA GEMM
//                (dgemm_mfma.hip.h) and cor_scatter_kernel divides and stores the ragged rows.
//
// No atomics; every floating-point sum runs in an order fixed by the shapes alone, the integer route has no sum to order.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dev_common.hip.h"

namespace gemma_hip {

constexpr int COR_THREADS = 256;
constexpr int COR_T = 64;                       // SNPs per side of a tile
constexpr int COR_BK = 64;                      // K bytes per step: one v_mfma_i32_16x16x64_i8
constexpr int COR_LDS_ROW = COR_BK + 16;        // 80-byte rows: the 16 rows a quarter-wave reads land in 16 different 16-byte slots
constexpr int COR_PLANE = COR_T * COR_LDS_ROW;  // one operand plane of a K step in LDS; four of them (A g, A c, B g, B c) = 20 KiB
constexpr long COR_I8_NMAX = 1L << 20;          // 4 n^3 < 2^63: the int64 combine is exact up to here

typedef int cor_i32x4 __attribute__((ext_vector_type(4)));

// sum over the 256 threads of a workgroup, the same value in every thread; red: 4 doubles of LDS
__device__ __forceinline__ double cor_bsum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads(); // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ int cor_wave_isum(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------------------------------------------------ hard calls
struct CorIngestI8 {
  const unsigned char *src; // l rows of ld bytes, PLINK 2-bit
  long ld, l, l_out;
  const int *idx; // position among the ni_total individuals of analysed individual j; nullptr: every individual, in order
  int n;
  int8_t *G, *Cm; // l x ldk each
  long ldk;       // a multiple of COR_BK
  int *st;        // 3 per SNP: N, S, S2
  double *var;    // l_out
};

// One wavefront per SNP.  PLINK code v = b0 + 2 b1: 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing (src/gemma_io.cpp:1156-1171).
__global__ __launch_bounds__(COR_THREADS) void cor_ingest_i8_kernel(CorIngestI8 g) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= g.l) return;
  const unsigned char *bs = g.src + s * g.ld;
  int8_t *gr = g.G + s * g.ldk, *cr = g.Cm + s * g.ldk;
  int N = 0, S = 0, S2 = 0;
  if (!g.idx && (reinterpret_cast<uintptr_t>(bs) & 3) == 0) {
    // every individual analysed: a lane turns one 32-bit word = 16 calls into one 16-byte store per plane.  Code c -> genotype byte
    // (0x00010002 >> 8 c) & 0xFF, called byte (0x01010001 >> 8 c) & 0xFF.
    const long nbytes = ((long)g.n + 3) / 4;
    for (long k = lane; k < g.ldk / 16; k += 64) {
      const long i0 = 16 * k;
      unsigned og[4] = {0u, 0u, 0u, 0u}, oc[4] = {0u, 0u, 0u, 0u};
      if (i0 < g.n) {
        const int nvalid = (g.n - i0 < 16) ? (int)(g.n - i0) : 16;
        unsigned w;
        if (i0 / 4 + 4 <= nbytes) {
          w = *reinterpret_cast<const unsigned *>(bs + i0 / 4);
        } else {
          w = 0u;
          for (int b = 0; b < 4; ++b)
            if (i0 / 4 + b < nbytes) w |= (unsigned)bs[i0 / 4 + b] << (8 * b);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const unsigned c = (w >> (2 * q)) & 3u;
          const unsigned bg = (q < nvalid) ? ((0x00010002u >> (8 * c)) & 0xFFu) : 0u; // the padding is "not called"
          const unsigned bc = (q < nvalid) ? ((0x01010001u >> (8 * c)) & 0xFFu) : 0u;
          og[q >> 2] |= bg << (8 * (q & 3));
          oc[q >> 2] |= bc << (8 * (q & 3));
          N += (int)bc;
          S += (int)bg;
          S2 += (int)(bg * bg);
        }
      }
      *reinterpret_cast<uint4 *>(gr + i0) = make_uint4(og[0], og[1], og[2], og[3]);
      *reinterpret_cast<uint4 *>(cr + i0) = make_uint4(oc[0], oc[1], oc[2], oc[3]);
    }
  } else {
    for (int i = lane; i < g.n; i += 64) {
      const int p = g.idx ? g.idx[i] : i;
      const unsigned v = (bs[p >> 2] >> (2 * (p & 3))) & 3u;
      const int called = (v != 1u), gv = (v == 0u) ? 2 : (v == 2u) ? 1 : 0;
      gr[i] = (int8_t)gv;
      cr[i] = (int8_t)called;
      N += called;
      S += gv;
      S2 += gv * gv;
    }
    for (long i = g.n + lane; i < g.ldk; i += 64) { // K padding: genotype 0, not called
      gr[i] = 0;
      cr[i] = 0;
    }
  }
  N = cor_wave_isum(N);
  S = cor_wave_isum(S);
  S2 = cor_wave_isum(S2);
  if (lane == 0) {
    g.st[3 * s] = N;
    g.st[3 * s + 1] = S;
    g.st[3 * s + 2] = S2;
    if (s < g.l_out) { // x.x / n = (S2 - S^2 / N) / n, one division of two exact integers (0 / 0 = NaN without a called genotype)
      const long long D = (long long)N * S2 - (long long)S * S;
      g.var[s] = (double)D / (double)((long long)N * g.n);
    }
  }
}

struct CorBandI8 {
  const int8_t *G, *Cm; // rows padded to whole tiles
  long ldk;
  int nk;               // ldk / COR_BK
  const int *st;        // 3 per SNP, padded rows 0
  const int *tiles;     // 2 per workgroup: row tile, column tile
  const int *n_nb;      // l_out
  const long long *off; // l_out: exclusive prefix sum of n_nb
  long l_out, l_in;
  int n;
  double *cor;
};

// numI = P1 Na Nb - Sa Nb P2 - Sb Na P3 + Sa Sb P4 (the terms wrap, the total fits: |numI| <= sqrt(Da Nb Db Na) <= 4 n^3),
// r = numI / sqrt((Da Nb)(Db Na)) with D = N S2 - S^2
__device__ __forceinline__ double cor_combine(long long P1, long long P2, long long P3, long long P4, int Na, int Sa, int S2a, int Nb,
                                              int Sb, int S2b) {
  typedef unsigned long long U;
  const U num = (U)P1 * (U)Na * (U)Nb - (U)Sa * (U)Nb * (U)P2 - (U)Sb * (U)Na * (U)P3 + (U)Sa * (U)Sb * (U)P4;
  const long long Da = (long long)Na * S2a - (long long)Sa * Sa, Db = (long long)Nb * S2b - (long long)Sb * Sb;
  const double den = sqrt((double)(Da * Nb) * (double)(Db * Na));
  return (double)(long long)num / den;
}

// The K loop of one tile pair.  MASKS: all four products; else P1 alone.  Thread t moves the 16 bytes (row t / 4, chunk t % 4) of
// each plane per K step: global -> registers one step ahead, registers -> LDS between two barriers.  Wave (wm, wn) owns 32 x 32 =
// 2 x 2 blocks of 16 x 16; lane (r16 = lane % 16, q = lane / 16) of a fragment holds K bytes 16 q .. 16 q + 15 of row / column r16.
template <bool MASKS>
__device__ __forceinline__ void cor_band_loop(const CorBandI8 &g, int8_t *lds, long rowA, long rowB, cor_i32x4 (&acc)[4][2][2]) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, r16 = lane & 15, q = lane >> 4;
  const int lrow = t >> 2, lch = t & 3;
  const long ga = (rowA + lrow) * g.ldk + 16 * lch, gb = (rowB + lrow) * g.ldk + 16 * lch;
  const int ldst = lrow * COR_LDS_ROW + 16 * lch;
  // four named values, all of them always defined: an array indexed under `if (MASKS)` went to scratch memory
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  uint4 vag = *reinterpret_cast<const uint4 *>(g.G + ga), vbg = *reinterpret_cast<const uint4 *>(g.G + gb);
  uint4 vac = MASKS ? *reinterpret_cast<const uint4 *>(g.Cm + ga) : zero4, vbc = MASKS ? *reinterpret_cast<const uint4 *>(g.Cm + gb) : zero4;
  for (int kt = 0; kt < g.nk; ++kt) {
    __syncthreads(); // the fragments of the previous step are read
    *reinterpret_cast<uint4 *>(lds + ldst) = vag;
    *reinterpret_cast<uint4 *>(lds + 2 * COR_PLANE + ldst) = vbg;
    if (MASKS) {
      *reinterpret_cast<uint4 *>(lds + COR_PLANE + ldst) = vac;
      *reinterpret_cast<uint4 *>(lds + 3 * COR_PLANE + ldst) = vbc;
    }
    __syncthreads();
    if (kt + 1 < g.nk) { // the next step's pieces travel while this step's matrix instructions run
      const long o = (long)(kt + 1) * COR_BK;
      vag = *reinterpret_cast<const uint4 *>(g.G + ga + o);
      vbg = *reinterpret_cast<const uint4 *>(g.G + gb + o);
      if (MASKS) {
        vac = *reinterpret_cast<const uint4 *>(g.Cm + ga + o);
        vbc = *reinterpret_cast<const uint4 *>(g.Cm + gb + o);
      }
    }
    cor_i32x4 ag[2], ac[2], bg[2], bc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int fa = (wm * 32 + 16 * i + r16) * COR_LDS_ROW + 16 * q, fb = (wn * 32 + 16 * i + r16) * COR_LDS_ROW + 16 * q;
      ag[i] = *reinterpret_cast<const cor_i32x4 *>(lds + fa);
      bg[i] = *reinterpret_cast<const cor_i32x4 *>(lds + 2 * COR_PLANE + fb);
      if (MASKS) {
        ac[i] = *reinterpret_cast<const cor_i32x4 *>(lds + COR_PLANE + fa);
        bc[i] = *reinterpret_cast<const cor_i32x4 *>(lds + 3 * COR_PLANE + fb);
      }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        acc[0][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag[i], bg[j], acc[0][i][j], 0, 0, 0);
        if (MASKS) {
          acc[1][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac[i], bg[j], acc[1][i][j], 0, 0, 0);
          acc[2][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ag[i], bc[j], acc[2][i][j], 0, 0, 0);
          acc[3][i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac[i], bc[j], acc[3][i][j], 0, 0, 0);
        }
      }
  }
}

__global__ __launch_bounds__(COR_THREADS) void cor_band_i8_kernel(CorBandI8 g) {
  __shared__ __attribute__((aligned(16))) int8_t lds[4 * COR_PLANE];
  const int ti = g.tiles[2 * blockIdx.x], tj = g.tiles[2 * blockIdx.x + 1];
  const long rowA = (long)ti * COR_T, rowB = (long)tj * COR_T;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, wm = wave >> 1, wn = wave & 1, r16 = lane & 15, q = lane >> 4;
  // a missing call in either tile?  (N < n; rows past l_in are padding and do not count)
  int miss = 0;
  if (t < 2 * COR_T) {
    const long s = (t < COR_T ? rowA : rowB - COR_T) + t;
    if (s < g.l_in) miss = g.st[3 * s] != g.n;
  }
  const bool masks = __syncthreads_or(miss) != 0; // the same in every thread of the workgroup
  cor_i32x4 acc[4][2][2];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[p][i][j] = (cor_i32x4){0, 0, 0, 0};
  if (masks) cor_band_loop<true>(g, lds, rowA, rowB, acc);
  else cor_band_loop<false>(g, lds, rowA, rowB, acc);
  // accumulator of a block: lane (c16 = r16, q) holds rows 4 q + r, column c16
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long a = rowA + wm * 32 + 16 * i + 4 * q + r;
      if (a >= g.l_out) continue;
      const int nb = g.n_nb[a];
      if (nb == 0) continue;
      const int Na = g.st[3 * a], Sa = g.st[3 * a + 1], S2a = g.st[3 * a + 2];
      const long long base = g.off[a];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const long b = rowB + wn * 32 + 16 * j + r16;
        const long d = b - a;
        if (d < 1 || d > nb) continue; // b <= a + n_nb[a] < l_in: checked on the host
        const int Nb = g.st[3 * b], Sb = g.st[3 * b + 1], S2b = g.st[3 * b + 2];
        const long long P1 = acc[0][i][j][r];
        const long long P2 = masks ? (long long)acc[1][i][j][r] : (long long)Sb;
        const long long P3 = masks ? (long long)acc[2][i][j][r] : (long long)Sa;
        const long long P4 = masks ? (long long)acc[3][i][j][r] : (long long)g.n;
        g.cor[base + d - 1] = cor_combine(P1, P2, P3, P4, Na, Sa, S2a, Nb, Sb, S2b);
      }
    }
}

// --------------------------------------------------------------------------------------------------------------- dosages
struct CorIngestF64 {
  const double *src; // l rows of ld doubles, NaN = missing
  long ld, l, l_out;
  const int *idx; // as CorIngestI8
  int n;
  double *X; // l x ldx: c (g - mu), columns n .. ldx - 1 written as 0
  long ldx;
  double *ss;  // l: x.x of the stored row (NaN without a called genotype; the row is then 0)
  double *var; // l_out
};

// One workgroup per SNP, as mqs_ingest_kernel without the covariate residual.
__global__ __launch_bounds__(COR_THREADS) void cor_ingest_f64_kernel(CorIngestF64 g) {
  __shared__ double red[4];
  const long s = blockIdx.x;
  const int n = g.n, tid = threadIdx.x;
  const double *row = g.src + s * g.ld;
  double *x = g.X + s * g.ldx;
  double tot = 0.0, cnt = 0.0;
  for (int i = tid; i < n; i += COR_THREADS) {
    const double v = row[g.idx ? g.idx[i] : i];
    if (!isnan(v)) { tot += v; cnt += 1.0; }
  }
  tot = cor_bsum(tot, red);
  cnt = cor_bsum(cnt, red);
  if (cnt == 0.0) { // the reference's mean is 0 / 0 and every entry of its column NaN
    for (long i = tid; i < g.ldx; i += COR_THREADS) x[i] = 0.0;
    if (tid == 0) {
      g.ss[s] = NAN;
      if (s < g.l_out) g.var[s] = NAN;
    }
    return;
  }
  const double mean = tot / cnt;
  double ss = 0.0;
  for (int i = tid; i < n; i += COR_THREADS) {
    double v = row[g.idx ? g.idx[i] : i];
    v = isnan(v) ? mean : v;
    v = v + (-1.0 * mean); // gsl_vector_add_constant(geno, -1.0 * geno_mean)
    x[i] = v;
    ss += v * v;
  }
  for (long i = n + tid; i < g.ldx; i += COR_THREADS) x[i] = 0.0;
  ss = cor_bsum(ss, red);
  if (tid == 0) {
    g.ss[s] = ss;
    if (s < g.l_out) g.var[s] = ss / (double)n;
  }
}

// Rows r0 .. r0 + rows - 1 of the band from their panel P (rows x ldp; column j of row a - r0 is x_a . x_{r0 + j}): one workgroup
// per row, r = P / sqrt(ss_a ss_b) into cor[off[a] + k - 1].
__global__ __launch_bounds__(COR_THREADS) void cor_scatter_kernel(const double *P, long ldp, long r0, const double *ss, const int *n_nb,
                                                                  const long long *off, double *cor) {
  const long a = r0 + blockIdx.x;
  const int nb = n_nb[a];
  const double va = ss[a];
  const double *p = P + (long)blockIdx.x * ldp + (a - r0);
  double *out = cor + off[a];
  for (int k = 1 + threadIdx.x; k <= nb; k += COR_THREADS) out[k - 1] = p[k] / sqrt(va * ss[a + k]);
}

} // namespace gemma_hip

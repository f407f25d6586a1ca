// Kernels of the MQS confidence intervals (GEMMA -ci 1 / -ci 2, a_mode 66 / 67; src/vc.cpp:2314-2437, :2568-2688), gfx950.
//
// Over the n analysed individuals a SNP s has mu_s = mean of its called genotypes, var_s = (sum g^2 + mu^2 n_miss) / n - mu^2 and
// x_si = g_si - mu_s (0 where missing).  With its category c_s, z-score z_s and weight w_s the two passes are
//
//   pass 1   Xz [i][c] = sum_{s: c_s = c}     z_s / sqrt(var_s) x_si        (PlinkXwz / BimbamXwz: one daxpy per SNP there)
//            XWz[i][c] = sum_{s: c_s = c} w_s z_s / sqrt(var_s) x_si
//   pass 2   XtXWz[s][j] = (sum_i x_si XWz[i][j]) / sqrt(var_s)             (PlinkXtXwz / BimbamXtXwz: n_vc ddots per SNP there)
//
// Both are skinny products with 16 columns and run on v_mfma_f64_16x16x4_f64 with the 2-bit calls decoded in registers: lane l
// supplies A[row = l & 15][k = l >> 4] and B[k = l >> 4][col = l & 15], and holds D[row = (l >> 4) + 4 r][col = l & 15] in
// accumulator r.  Nobody writes an fp64 copy of a 2-bit block.
//
//   pass 1   M = 16 individuals (one 2-bit word), K = SNPs, N = the n_vc columns of Xz then the n_vc columns of XWz.  A is the
//            SNP's table of what a call code adds, {2 - mu, 0, 1 - mu, -mu} z / sqrt(var); B of SNP s is 1 in column c_s, w_s in
//            column n_vc + c_s and 0 elsewhere.  A wavefront owns CI_TILES words of every row of its SNP partition.
//   pass 2   M = 16 SNPs, K = individuals, N = the columns of XWz padded to 16.  The four wavefronts of a workgroup cut K.
//
// A SNP without a called genotype or with var == 0 among the analysed individuals is skipped: its table is 0 in pass 1, its
// row is 0 in pass 2 (the reference divides by 0 there).  Every sum runs in an order the launch geometry alone fixes (MFMA k
// order -> SNP partitions / wavefronts in index order -> blocks in call order); there are no floating-point atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dev_common.hip.h"

namespace gemma_hip {

constexpr int CI_COLS = 16;       // one MFMA's width: 2 n_vc <= 16
constexpr int CI_TILES = 8;       // pass 1: 2-bit words (16 individuals each) per wavefront
constexpr int CI_PARTS_MAX = 32;  // pass 1: SNP partitions
constexpr int CI_PART_MIN = 64;   // pass 1: at least this many rows per partition
constexpr int CI_GROUP = 16;      // pass 2: words per K step of a wavefront (4 per k quarter)

typedef double ci_f64x4 __attribute__((ext_vector_type(4)));

template <bool ALIGNED>
__device__ __forceinline__ unsigned ci_word(const unsigned char *row, long w, long bytes) {
  if (ALIGNED && 4 * w + 4 <= bytes) return reinterpret_cast<const unsigned *>(row)[w];
  unsigned v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (4 * w + b < bytes) v |= (unsigned)row[4 * w + b] << (8 * b);
  return v;
}

// what code v = b0 + 2 b1 of a call selects from {t0, 0, t2, t3}: 0 -> 2, 1 -> missing, 2 -> 1, 3 -> 0 (src/vc.cpp:2379-2396)
__device__ __forceinline__ double ci_pick(unsigned code, double t0, double t2, double t3) {
  return code == 0u ? t0 : (code == 2u ? t2 : (code == 3u ? t3 : 0.0));
}

// mu, 1 / sqrt(var) (0: skipped) from the sums over the called genotypes of the n analysed individuals
__device__ __forceinline__ double2 ci_moments(double sum, double cnt, double sumsq, int n) {
  if (!(cnt > 0.0)) return make_double2(0.0, 0.0);
  const double mu = sum / cnt;
  const double var = (sumsq + mu * mu * ((double)n - cnt)) / (double)n - mu * mu;
  if (!(var > 0.0)) return make_double2(mu, 0.0);
  return make_double2(mu, 1.0 / sqrt(var));
}

// ------------------------------------------------------------------------------------------------ per-SNP counts
// st[s] = {mu, 1 / sqrt(var)}; one wavefront per row, exact integer sums by popcount (as mv_stats_plink_kernel, with sum g^2).
// amask: bit 2k of word w = individual 16 w + k is analysed.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ci_stats_plink_kernel(const unsigned char *G, long ld, long l, const unsigned *amask, long ni_total,
                                                             long words, int n, double2 *st) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= l) return;
  const unsigned char *row = G + s * ld;
  const long bytes = (ni_total + 3) / 4;
  long long sg = 0, cg = 0, qg = 0; // sum g^2 reaches 4 n: past an int from n = 2^29, and ni_total may be 2^30
  for (long w = lane; w < words; w += 64) {
    const unsigned v = ci_word<ALIGNED>(row, w, bytes);
    const unsigned lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
    const unsigned two = ~lo & ~hi & 0x55555555u, one = hi & ~lo, nm = ~(lo & ~hi) & 0x55555555u;
    const unsigned a = amask[w];
    const int p2 = __popc(two & a), p1 = __popc(one & a);
    sg += 2 * p2 + p1;
    qg += 4 * p2 + p1;
    cg += __popc(nm & a);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sg += __shfl_xor(sg, off, 64);
    cg += __shfl_xor(cg, off, 64);
    qg += __shfl_xor(qg, off, 64);
  }
  if (lane == 0) st[s] = ci_moments((double)sg, (double)cg, (double)qg, n);
}

// fp64 rows (NaN = missing): the same moments, and the centred row over the analysed individuals in their order,
// X[s][j] = g - mu (0 where missing, and in the columns n .. ldx - 1).  One workgroup per SNP.
__global__ __launch_bounds__(256) void ci_ingest_f64_kernel(const double *G, long ld, long l, const int *idx, int n, double *X, long ldx,
                                                            double2 *st) {
  __shared__ double red[3][4];
  const long s = blockIdx.x;
  const int tid = threadIdx.x;
  const double *row = G + s * ld;
  double sg = 0.0, cg = 0.0, qg = 0.0;
  for (int j = tid; j < n; j += 256) {
    const double v = row[idx[j]];
    if (!isnan(v)) { sg += v; cg += 1.0; qg += v * v; }
  }
  sg = wave_sum(sg); cg = wave_sum(cg); qg = wave_sum(qg);
  if ((tid & 63) == 0) { red[0][tid >> 6] = sg; red[1][tid >> 6] = cg; red[2][tid >> 6] = qg; }
  __syncthreads();
  sg = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  cg = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  qg = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
  const double2 m = ci_moments(sg, cg, qg, n);
  if (tid == 0) st[s] = m;
  double *x = X + s * ldx;
  for (long j = tid; j < ldx; j += 256) {
    double v = 0.0;
    if (j < n) {
      const double g = row[idx[j]];
      v = (isnan(g) || m.y == 0.0) ? 0.0 : g - m.x;
    }
    x[j] = v;
  }
}

// ------------------------------------------------------------------------------------------------ pass 1 operands
// tab[s] = {2 - mu, 0, 1 - mu, -mu} z / sqrt(var) (the A operand of a 2-bit SNP), bm[s][16] = the B row of the SNP -- for the fp64
// route scaled by z / sqrt(var), since its A operand is the plain centred row.  A skipped SNP is 0 in both and counted in
// flags[0]; a category outside 0 .. n_vc - 1 sets flags[1] (every writer stores the same value).
template <bool PLINK>
__global__ __launch_bounds__(256) void ci_table_kernel(const double2 *st, const int *cat, const double *z, const double *w, long l, int n_vc,
                                                       double4 *tab, double *bm, int *flags) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= l) return;
  const double2 m = st[s];
  const int c = cat[s];
  const bool bad = c < 0 || c >= n_vc, skip = m.y == 0.0;
  if (bad) flags[1] = 1;
  if (skip) atomicAdd(&flags[0], 1); // an integer count: the order does not matter
  const double a = skip ? 0.0 : z[s] * m.y;
  const double ww = skip ? 0.0 : (w ? w[s] : 1.0);
  if (PLINK) tab[s] = make_double4((2.0 - m.x) * a, 0.0, (1.0 - m.x) * a, (0.0 - m.x) * a);
  const double one = PLINK ? (skip ? 0.0 : 1.0) : a;
#pragma unroll
  for (int k = 0; k < CI_COLS; ++k) bm[s * CI_COLS + k] = (bad || skip) ? 0.0 : (k == c ? one : (k == n_vc + c ? one * ww : 0.0));
}

constexpr long CI_PART_BYTES = 256L << 20; // pass 1: budget of the partial sums

// SNP partitions of a block of l rows over `words` 2-bit words per row: as many as give every partition CI_PART_MIN rows, at most
// CI_PARTS_MAX, and no more than keep the partial sums (partitions x 16 words x 16 doubles) within CI_PART_BYTES -- a function of
// the shapes alone, like every other part of the summation order.
inline int ci_parts(long l, long words) {
  long p = (l + CI_PART_MIN - 1) / CI_PART_MIN;
  const long fit = CI_PART_BYTES / (words * 16 * CI_COLS * 8);
  if (p > CI_PARTS_MAX) p = CI_PARTS_MAX;
  if (p > fit) p = fit;
  return (int)(p < 1 ? 1 : p);
}

// ------------------------------------------------------------------------------------------------ pass 1, 2-bit rows
// grid = (ceil(words / (4 CI_TILES)), partitions), 256 threads.  Lane (i = l & 15, kq = l >> 4) of a K step takes SNP sb + kq:
// its table, its B entry of column i and, per tile, the word whose call i it decodes.  part[(p ldp + individual) 16 + col] for
// every individual of the row (ldp = 16 words); the combine picks the analysed ones.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ci_xwz_plink_kernel(const unsigned char *G, long ld, long l, const unsigned *amask, long ni_total,
                                                           long words, const double4 *tab, const double *bm, int rows_per_part,
                                                           double *part, long ldp) {
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long w0 = ((long)blockIdx.x * 4 + wave) * CI_TILES;
  if (w0 >= words) return;
  const long bytes = (ni_total + 3) / 4;
  unsigned keep[CI_TILES]; // individuals outside the analysed set read as missing
#pragma unroll
  for (int t = 0; t < CI_TILES; ++t) {
    const unsigned am = (w0 + t < words) ? amask[w0 + t] : 0u;
    keep[t] = am | (am << 1);
  }
  ci_f64x4 acc[CI_TILES];
#pragma unroll
  for (int t = 0; t < CI_TILES; ++t) acc[t] = ci_f64x4{0.0, 0.0, 0.0, 0.0};
  const long s0 = (long)blockIdx.y * rows_per_part;
  const long s1 = min(l, s0 + rows_per_part);
  for (long sb = s0; sb < s1; sb += 4) {
    const long s = sb + kq;
    const bool live = s < s1;
    const double4 tb = live ? tab[s] : make_double4(0.0, 0.0, 0.0, 0.0);
    const double b = live ? bm[s * CI_COLS + i] : 0.0;
    const unsigned char *row = G + (live ? s : s0) * ld;
#pragma unroll
    for (int t = 0; t < CI_TILES; ++t) {
      unsigned v = (live && w0 + t < words) ? ci_word<ALIGNED>(row, w0 + t, bytes) : 0u;
      v = (v & keep[t]) | (~keep[t] & 0x55555555u);
      const double a = ci_pick((v >> (2 * i)) & 3u, tb.x, tb.z, tb.w);
      acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
    }
  }
  // accumulator r of the lane: individual kq + 4 r of the tile, column i
#pragma unroll
  for (int t = 0; t < CI_TILES; ++t) {
    if (w0 + t >= words) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) part[((long)blockIdx.y * ldp + 16 * (w0 + t) + kq + 4 * r) * CI_COLS + i] = acc[t][r];
  }
}

// acc[j][col] += sum over the partitions, in index order, of part[p][idx[j]][col]  (acc: n x 16)
__global__ __launch_bounds__(256) void ci_combine_kernel(const double *part, long ldp, int parts, const int *idx, long n, double *acc) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n * CI_COLS) return;
  const long i = idx[t / CI_COLS];
  const int col = (int)(t % CI_COLS);
  double a = 0.0;
  for (int p = 0; p < parts; ++p) a += part[((long)p * ldp + i) * CI_COLS + col];
  acc[t] += a;
}

// ------------------------------------------------------------------------------------------------ pass 2, 2-bit rows
// grid = ceil(l / 16), 256 threads: a workgroup owns 16 SNPs, wavefront v the word groups [ngrp v / 4, ngrp (v + 1) / 4) of
// CI_GROUP words; lane (i, kq) decodes the words 16 g + 4 kq .. + 3 of SNP s0 + i, call by call, against row `individual` of
// Bf (rows of the individuals outside the analysed set, and past ni_total, are 0: Bf has ngrp CI_GROUP 16 rows of 16).
// out[s][j] = sum / sqrt(var), j < n_vc.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void ci_xtxwz_plink_kernel(const unsigned char *G, long ld, long l, long ni_total, long words,
                                                             const double2 *st, const double *Bf, int n_vc, double *out) {
  __shared__ double red[3][256];
  const int lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long s0 = (long)blockIdx.x * 16;
  const long srow = min(s0 + i, l - 1);
  const long bytes = (ni_total + 3) / 4;
  const unsigned char *row = G + srow * ld;
  const double mu = st[srow].x;
  const double t0 = 2.0 - mu, t2 = 1.0 - mu, t3 = 0.0 - mu;
  const long ngrp = (words + CI_GROUP - 1) / CI_GROUP;
  const long g0 = ngrp * wave / 4, g1 = ngrp * (wave + 1) / 4;
  ci_f64x4 acc = ci_f64x4{0.0, 0.0, 0.0, 0.0};
  for (long g = g0; g < g1; ++g) {
    const long wb = g * CI_GROUP + 4 * kq;
    unsigned v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (wb + e < words) ? ci_word<ALIGNED>(row, wb + e, bytes) : 0x55555555u;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double *bp = Bf + (16 * (wb + e)) * CI_COLS + i;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const double a = ci_pick((v[e] >> (2 * t)) & 3u, t0, t2, t3);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bp[t * CI_COLS], acc, 0, 0, 0);
      }
    }
  }
  // the four K slices in index order; accumulator r of the lane: SNP s0 + kq + 4 r, column i
  if (wave > 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wave - 1][r * 64 + lane] = acc[r];
  }
  __syncthreads();
  if (wave == 0 && i < n_vc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long s = s0 + kq + 4 * r;
      if (s < l) {
        const double sum = ((acc[r] + red[0][r * 64 + lane]) + red[1][r * 64 + lane]) + red[2][r * 64 + lane];
        out[s * n_vc + i] = sum * st[s].y;
      }
    }
  }
}

// fp64 route: out[s][j] = P[s][j] / sqrt(var), j < n_vc, from the GEMM's l x 16 product
__global__ __launch_bounds__(256) void ci_scale_rows_kernel(const double *P, const double2 *st, long l, int n_vc, double *out) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= l * n_vc) return;
  const long s = t / n_vc;
  out[t] = P[s * CI_COLS + t % n_vc] * st[s].y;
}

} // namespace gemma_hip

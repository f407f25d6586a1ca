// Matrix-vector products on SNP-major genotype blocks (gfx950): the two passes of genomic prediction.
//
//   X_c^T r   (ridge / BLUP effects, -bslmm 2):  alpha_s = sum_i xc_si r_i,  xc = g - mean over the analysed non-missing calls,
//             a missing call contributes 0 (ReadFile_bed / ReadFile_geno with a UtX argument, GEMMA src/gemma_io.cpp:1956-2084,
//             :1742-1845, followed by the dgemv of BSLMM::RidgeR, src/bslmm.cpp:1208 -- without ever forming U^T X)
//   X~ w      (-predict):  y_t += sum_s w_s x~_st over the test individuals, x~ = g - x_train_mean, a missing test call is
//             x_mean - x_train_mean, a SNP missing in every test individual is skipped (PRDT::AnalyzePlink / AnalyzeBimbam,
//             src/prdt.cpp:310-444, :207-308)
//
// Both read a block once for the per-SNP counts (popcounts on the 2-bit words) and once for the product; a 2-bit block of
// 20 000 x 20 000 calls is 100 MB, the vectors are 160 KB.  Two groups of individuals: A = analysed / training
// (indicator_idv == 1), B = test (indicator_idv == 0; prediction only).
//
// Reduction orders are fixed by the launch geometry alone (lane -> wavefront butterfly -> wavefronts of a workgroup ->
// column chunks / SNP partitions in index order): two runs of a call are bit-identical, there are no floating-point atomics.
//
// 2-bit rows: the thread that owns word w of a row (16 individuals) keeps its 16 entries of r -- or its 16 accumulators of
// y -- in registers over all rows of its tile, so r and y cost no traffic per row and the lanes of a wavefront read
// consecutive words.  fp64 rows: one wavefront per row for X_c^T r (r from L2), one thread per individual for X~ w.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dev_common.hip.h"

namespace gemma_hip {

constexpr int MV_ROWS = 64;       // X_c^T r, 2-bit: SNP rows per workgroup
constexpr int MV_CHUNK = 256;     // X_c^T r, 2-bit: words per workgroup (4096 individuals)
constexpr int MV_PARTS_MAX = 32;  // X~ w: SNP partitions
constexpr int MV_PART_MIN = 64;   // X~ w: at least this many rows per partition

// word w of a 2-bit row of `bytes` bytes; bits past the row's end read as 0 (the group masks never select them)
template <bool ALIGNED>
__device__ __forceinline__ unsigned mv_word(const unsigned char *row, long w, long bytes) {
  if (ALIGNED && 4 * w + 4 <= bytes) return reinterpret_cast<const unsigned *>(row)[w];
  unsigned v = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (4 * w + b < bytes) v |= (unsigned)row[4 * w + b] << (8 * b);
  return v;
}

struct MvGroups {
  const unsigned *amask, *bmask; // 2-bit rows: bit 2k of word w = individual 16 w + k is in the group (bmask may be nullptr)
  const unsigned char *grp;      // fp64 rows: 1 = A, 2 = B, 0 = neither
  long ni_total;                 // individuals per row
  long words;                    // ceil(ni_total / 16)
};

// ------------------------------------------------------------------------------------------------ per-SNP counts
// stats[s] = {sum of the non-missing calls of A, their count, the same for B}; one wavefront per row.
// PLINK code v = b0 + 2 b1: 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing (ingest.hip.h, plink_value): exact integer sums by popcount.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void mv_stats_plink_kernel(const unsigned char *G, long ld, long l, MvGroups g, double4 *stats) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= l) return;
  const unsigned char *row = G + s * ld;
  const long bytes = (g.ni_total + 3) / 4;
  int sa = 0, ca = 0, sb = 0, cb = 0;
  for (long w = lane; w < g.words; w += 64) {
    const unsigned v = mv_word<ALIGNED>(row, w, bytes);
    const unsigned lo = v & 0x55555555u, hi = (v >> 1) & 0x55555555u;
    const unsigned two = ~lo & ~hi & 0x55555555u, one = hi & ~lo, nm = ~(lo & ~hi) & 0x55555555u;
    const unsigned a = g.amask[w];
    sa += 2 * __popc(two & a) + __popc(one & a);
    ca += __popc(nm & a);
    if (g.bmask) {
      const unsigned b = g.bmask[w];
      sb += 2 * __popc(two & b) + __popc(one & b);
      cb += __popc(nm & b);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    sa += __shfl_xor(sa, off, 64);
    ca += __shfl_xor(ca, off, 64);
    sb += __shfl_xor(sb, off, 64);
    cb += __shfl_xor(cb, off, 64);
  }
  if (lane == 0) stats[s] = make_double4((double)sa, (double)ca, (double)sb, (double)cb);
}

__global__ __launch_bounds__(256) void mv_stats_f64_kernel(const double *X, long ld, long l, MvGroups g, double4 *stats) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= l) return;
  const double *row = X + s * ld;
  double sa = 0.0, ca = 0.0, sb = 0.0, cb = 0.0;
  for (long i = lane; i < g.ni_total; i += 64) {
    const int k = g.grp[i];
    if (k == 0) continue;
    const double x = row[i];
    if (isnan(x)) continue;
    if (k == 1) { sa += x; ca += 1.0; }
    else { sb += x; cb += 1.0; }
  }
  sa = wave_sum(sa); ca = wave_sum(ca); sb = wave_sum(sb); cb = wave_sum(cb);
  if (lane == 0) stats[s] = make_double4(sa, ca, sb, cb);
}

// ------------------------------------------------------------------------------------------------ X_c^T r
// 2-bit rows.  grid = (column chunks of MV_CHUNK words, tiles of MV_ROWS rows), 256 threads.  r_full: r scattered to the
// positions of the analysed individuals, 0 elsewhere, padded with zeros to gridDim.x * MV_CHUNK * 16 entries.
// part[chunk * l + s] = the chunk's share of sum_i xc_si r_i.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void mv_xtr_plink_kernel(const unsigned char *G, long ld, long l, MvGroups g, const double *r_full,
                                                           const double4 *stats, double *part) {
  __shared__ double red[MV_ROWS][4];
  __shared__ double tab[MV_ROWS][4]; // per row: what a call adds per unit of r, indexed by its code {2 - mean, 0, 1 - mean, 0 - mean}
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long w = (long)blockIdx.x * MV_CHUNK + threadIdx.x;
  const bool live = w < g.words;
  const long bytes = (g.ni_total + 3) / 4;
  const unsigned am = live ? g.amask[w] : 0u;
  const unsigned keep = am | (am << 1); // individuals outside the group read as missing
  double rr[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) rr[k] = r_full[16 * w + k];
  const long s0 = (long)blockIdx.y * MV_ROWS;
  const int rows = (int)min((long)MV_ROWS, l - s0);
  if ((int)threadIdx.x < rows) {
    const double4 st = stats[s0 + threadIdx.x];
    // an all-missing SNP: every entry of the reference's column is 0 (its mean is 0 / 0 and never used)
    const double mean = st.y > 0.0 ? st.x / st.y : 0.0;
    tab[threadIdx.x][0] = 2.0 - mean;
    tab[threadIdx.x][1] = 0.0;
    tab[threadIdx.x][2] = 1.0 - mean;
    tab[threadIdx.x][3] = 0.0 - mean;
  }
  __syncthreads();
#pragma unroll 2
  for (int t = 0; t < rows; ++t) {
    const long s = s0 + t;
    unsigned v = live ? mv_word<ALIGNED>(G + s * ld, w, bytes) : 0u;
    v = (v & keep) | (~keep & 0x55555555u);
    const double *tr = tab[t];
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) acc = fma(tr[(v >> (2 * k)) & 3u], rr[k], acc);
    acc = wave_sum(acc);
    if (lane == 0) red[t][wave] = acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < rows)
    part[(long)blockIdx.x * l + s0 + threadIdx.x] =
        ((red[threadIdx.x][0] + red[threadIdx.x][1]) + red[threadIdx.x][2]) + red[threadIdx.x][3];
}

__global__ __launch_bounds__(256) void mv_xtr_finish_kernel(const double *part, int chunks, long l, double scale, double *alpha) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= l) return;
  double a = 0.0;
  for (int c = 0; c < chunks; ++c) a += part[(long)c * l + s];
  alpha[s] = scale * a;
}

// fp64 rows (NaN = missing): one wavefront per row, the mean first, then the centred dot product (the row comes back from L2)
__global__ __launch_bounds__(256) void mv_xtr_f64_kernel(const double *X, long ld, long l, MvGroups g, const double *r_full, double scale,
                                                         double *alpha) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= l) return;
  const double *row = X + s * ld;
  double tot = 0.0, cnt = 0.0;
  for (long i = lane; i < g.ni_total; i += 64) {
    const double x = row[i];
    if (g.grp[i] == 1 && !isnan(x)) { tot += x; cnt += 1.0; }
  }
  tot = wave_sum(tot);
  cnt = wave_sum(cnt);
  const double mean = tot / cnt;
  double acc = 0.0;
  for (long i = lane; i < g.ni_total; i += 64) {
    const double x = row[i];
    if (g.grp[i] == 1 && !isnan(x)) acc = fma(x - mean, r_full[i], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) alpha[s] = scale * acc;
}

// ------------------------------------------------------------------------------------------------ X~ w
// Per-SNP terms of the prediction.  2-bit rows: tab[s] = the four values a call can add, indexed by its code
// {2 - tm, x_mean - tm, 1 - tm, 0 - tm} * w; fp64 rows: tab[s] = {tm, w, (x_mean - tm) * w, used}.  A SNP without a
// non-missing test call is skipped (all zero, used[s] = 0); one without a non-missing training call has tm = 0 / 0 = NaN,
// as in the reference (src/prdt.cpp:283, :420), and makes every prediction NaN.
template <bool PLINK>
__global__ __launch_bounds__(256) void mv_xw_table_kernel(const double4 *stats, const double *w, long l, double4 *tab, int *used) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  if (s >= l) return;
  const double4 st = stats[s];
  const bool use = st.w > 0.0;
  const double tm = st.x / st.y, xm = st.z / st.w, e = w[s];
  double4 t;
  if (PLINK) t = use ? make_double4((2.0 - tm) * e, (xm - tm) * e, (1.0 - tm) * e, (0.0 - tm) * e) : make_double4(0.0, 0.0, 0.0, 0.0);
  else t = use ? make_double4(tm, e, (xm - tm) * e, 1.0) : make_double4(0.0, 0.0, 0.0, 0.0);
  tab[s] = t;
  used[s] = use ? 1 : 0;
}

inline int mv_parts(long l) {
  long p = (l + MV_PART_MIN - 1) / MV_PART_MIN;
  return (int)(p < 1 ? 1 : (p > MV_PARTS_MAX ? MV_PARTS_MAX : p));
}

// 2-bit rows.  grid = (chunks of 64 words, partitions), 256 threads: the four wavefronts of a workgroup own the same 64 words
// (1024 individuals) and take every fourth row of the partition; 16 accumulators per lane, summed over the wavefronts in
// LDS.  part[p * ldp + i] for individual i (every individual of the row: the combine picks the test ones).
template <bool ALIGNED>
__global__ __launch_bounds__(256) void mv_xw_plink_kernel(const unsigned char *G, long ld, long l, MvGroups g, const double4 *tab,
                                                          int rows_per_part, double *part, long ldp) {
  __shared__ double red[3][16][64];
  __shared__ double4 lt[256]; // the table rows of 256 SNPs at a time
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long w = (long)blockIdx.x * 64 + lane;
  const bool live = w < g.words;
  const long bytes = (g.ni_total + 3) / 4;
  const long s0 = (long)blockIdx.y * rows_per_part;
  const long s1 = min(l, s0 + rows_per_part);
  double acc[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) acc[k] = 0.0;
  for (long tb = s0; tb < s1; tb += 256) {
    const int m = (int)min(256L, s1 - tb);
    if ((int)threadIdx.x < m) lt[threadIdx.x] = tab[tb + threadIdx.x];
    __syncthreads();
#pragma unroll 2
    for (int i = wave; i < m; i += 4) {
      const unsigned v = live ? mv_word<ALIGNED>(G + (tb + i) * ld, w, bytes) : 0u;
      const double *tr = reinterpret_cast<const double *>(&lt[i]);
#pragma unroll
      for (int k = 0; k < 16; ++k) acc[k] += tr[(v >> (2 * k)) & 3u];
    }
    __syncthreads();
  }
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) red[wave - 1][k][lane] = acc[k];
  }
  __syncthreads();
  if (wave == 0 && live) {
    double *out = part + (long)blockIdx.y * ldp + 16 * w;
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (16 * w + k < g.ni_total) out[k] = ((acc[k] + red[0][k][lane]) + red[1][k][lane]) + red[2][k][lane];
  }
}

// fp64 rows: one thread per individual, grid = (ceil(ni_total / 256), partitions)
__global__ __launch_bounds__(256) void mv_xw_f64_kernel(const double *X, long ld, long l, MvGroups g, const double4 *tab, int rows_per_part,
                                                        double *part, long ldp) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= g.ni_total) return;
  const long s0 = (long)blockIdx.y * rows_per_part;
  const long s1 = min(l, s0 + rows_per_part);
  const bool test = g.grp[i] == 2;
  double acc = 0.0;
  if (test) {
#pragma unroll 4
    for (long s = s0; s < s1; ++s) {
      const double x = X[s * ld + i];
      const double4 t = tab[s];
      const double v = isnan(x) ? t.z : (x - t.x) * t.y;
      acc += (t.w != 0.0) ? v : 0.0;
    }
  }
  part[(long)blockIdx.y * ldp + i] = acc;
}

// y[t] += sum over the partitions, in index order, of part[p][pos[t]]
__global__ __launch_bounds__(256) void mv_xw_combine_kernel(const double *part, long ldp, int parts, const int *pos, long n_test, double *y) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n_test) return;
  const long i = pos[t];
  double a = 0.0;
  for (int p = 0; p < parts; ++p) a += part[(long)p * ldp + i];
  y[t] += a;
}

// ------------------------------------------------------------------------------------------------ launchers
inline long mv_chunks(long words) { return (words + MV_CHUNK - 1) / MV_CHUNK; }
// entries of r_full the 2-bit kernel reads
inline long mv_rfull_len(long ni_total) { return mv_chunks((ni_total + 15) / 16) * MV_CHUNK * 16; }
// doubles of workspace: stats (4 l) + the partial sums
inline long mv_xtr_work(long ni_total, long l) { return 4 * l + mv_chunks((ni_total + 15) / 16) * l; }
inline long mv_xw_work(long ni_total, long l) { return 8 * l + (long)mv_parts(l) * (((ni_total + 15) / 16) * 16); }

inline bool mv_aligned(const void *p, long ld) { return ((reinterpret_cast<uintptr_t>(p) & 3) == 0) && ((ld & 3) == 0); }

// alpha[l] = scale * X_c^T r; work: mv_xtr_work doubles
inline hipError_t launch_xtr(bool plink, const void *geno, long l, long ld, const MvGroups &g, const double *r_full, double scale,
                             double *alpha, double *work, hipStream_t s) {
  if (l <= 0) return hipSuccess;
  const unsigned rows4 = (unsigned)((l + 3) / 4);
  if (!plink) {
    mv_xtr_f64_kernel<<<rows4, 256, 0, s>>>(reinterpret_cast<const double *>(geno), ld, l, g, r_full, scale, alpha);
    return hipGetLastError();
  }
  double4 *stats = reinterpret_cast<double4 *>(work);
  double *part = work + 4 * l;
  const unsigned char *G = reinterpret_cast<const unsigned char *>(geno);
  const int chunks = (int)mv_chunks(g.words);
  const dim3 grid((unsigned)chunks, (unsigned)((l + MV_ROWS - 1) / MV_ROWS));
  MvGroups ga = g;
  ga.bmask = nullptr;
  if (mv_aligned(geno, ld)) {
    mv_stats_plink_kernel<true><<<rows4, 256, 0, s>>>(G, ld, l, ga, stats);
    mv_xtr_plink_kernel<true><<<grid, 256, 0, s>>>(G, ld, l, ga, r_full, stats, part);
  } else {
    mv_stats_plink_kernel<false><<<rows4, 256, 0, s>>>(G, ld, l, ga, stats);
    mv_xtr_plink_kernel<false><<<grid, 256, 0, s>>>(G, ld, l, ga, r_full, stats, part);
  }
  mv_xtr_finish_kernel<<<(unsigned)((l + 255) / 256), 256, 0, s>>>(part, chunks, l, scale, alpha);
  return hipGetLastError();
}

// y[n_test] += X~ w over the individuals pos[0 .. n_test); used[l]; work: mv_xw_work doubles
inline hipError_t launch_xw(bool plink, const void *geno, long l, long ld, const MvGroups &g, const double *w, const int *pos, long n_test,
                            double *y, int *used, double *work, hipStream_t s) {
  if (l <= 0) return hipSuccess;
  double4 *stats = reinterpret_cast<double4 *>(work);
  double4 *tab = reinterpret_cast<double4 *>(work + 4 * l);
  double *part = work + 8 * l;
  const long ldp = g.words * 16;
  const int parts = mv_parts(l);
  const int rpp = (int)((l + parts - 1) / parts);
  const unsigned rows4 = (unsigned)((l + 3) / 4), lb = (unsigned)((l + 255) / 256);
  if (plink) {
    const unsigned char *G = reinterpret_cast<const unsigned char *>(geno);
    const dim3 grid((unsigned)((g.words + 63) / 64), (unsigned)parts);
    if (mv_aligned(geno, ld)) {
      mv_stats_plink_kernel<true><<<rows4, 256, 0, s>>>(G, ld, l, g, stats);
      mv_xw_table_kernel<true><<<lb, 256, 0, s>>>(stats, w, l, tab, used);
      mv_xw_plink_kernel<true><<<grid, 256, 0, s>>>(G, ld, l, g, tab, rpp, part, ldp);
    } else {
      mv_stats_plink_kernel<false><<<rows4, 256, 0, s>>>(G, ld, l, g, stats);
      mv_xw_table_kernel<true><<<lb, 256, 0, s>>>(stats, w, l, tab, used);
      mv_xw_plink_kernel<false><<<grid, 256, 0, s>>>(G, ld, l, g, tab, rpp, part, ldp);
    }
  } else {
    const double *X = reinterpret_cast<const double *>(geno);
    const dim3 grid((unsigned)((g.ni_total + 255) / 256), (unsigned)parts);
    mv_stats_f64_kernel<<<rows4, 256, 0, s>>>(X, ld, l, g, stats);
    mv_xw_table_kernel<false><<<lb, 256, 0, s>>>(stats, w, l, tab, used);
    mv_xw_f64_kernel<<<grid, 256, 0, s>>>(X, ld, l, g, tab, rpp, part, ldp);
  }
  if (n_test > 0) mv_xw_combine_kernel<<<(unsigned)((n_test + 255) / 256), 256, 0, s>>>(part, ldp, parts, pos, n_test, y);
  return hipGetLastError();
}

} // namespace gemma_hip

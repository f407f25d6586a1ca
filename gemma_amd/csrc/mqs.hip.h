// Kernels of the MQS summary-statistic variance components (GEMMA -gs and -vc 1 -beta; Zhou 2017), gfx950.
//
//   ingest      PlinkKin / BimbamKinUncentered with weights and categories, src/gemma_io.cpp:2947-3170, :2753-2945: per SNP over the
//               analysed individuals -- mean of the called genotypes, impute, centre, residual on the covariates
//               x <- x - W (W^T W)^-1 W^T x, var = x^T x / n of that residual.  One workgroup per SNP.
//   compaction  the kept SNPs (cat >= 0, var != 0) of category c, scaled by sqrt(w / var), written densely and in order into the
//               panel rows [sum_{c' < c} cnt_c', +cnt_c): a prefix sum per category, integers only.
//   centre/scale  CenterMatrix + ScaleMatrix (src/mathfunc.cpp:147-177, :271-286) on a matrix with a leading dimension.
//   row pass    row sums and the diagonal of one matrix.
//   pair pass   h[t] = sum_k A[t,k] K[t,k], u = A sK, v = K sA for one ordered pair: A and K read once, two doubles per load.
//
// Every floating-point sum runs in an order fixed by the shapes alone (lane stride -> wavefront butterfly -> wavefronts of the
// workgroup in index order); there are no atomics, two runs agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dev_common.hip.h"

namespace gemma_hip {

constexpr int MQS_THREADS = 256;
constexpr int MQS_SCAN_THREADS = 1024;
constexpr int MQS_CMAX = 64;  // covariates, as everywhere in the library
constexpr int MQS_VCMAX = 8;  // categories

// sum over the 256 threads of a workgroup, the same value in every thread; red: 4 doubles of LDS
__device__ __forceinline__ double mqs_bsum(double v, double *red) {
  v = wave_sum(v);
  __syncthreads(); // red may still be read from the previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

struct MqsIngest {
  const void *src; // GEMMA_GENO_PLINK_2BIT: ld bytes per SNP; GEMMA_GENO_F64_SNP_MAJOR: ld doubles per SNP, NaN = missing
  long ld, l;
  const int *idx;   // position among the ni_total individuals of analysed individual j
  int n, c;         // analysed individuals, covariates
  const double *Wt; // c x ldx: W transposed
  const double *Wi; // c x c: (W^T W)^-1
  double *X;        // l x ldx: the residuals, SNP-major; columns n .. ldx - 1 are written as 0
  long ldx;
  double *var;      // l
};

// PLINK 2-bit code v = b0 + 2 b1: 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing (src/gemma_io.cpp:3043-3060)
template <bool PLINK>
__device__ __forceinline__ double mqs_call(const MqsIngest &g, long s, int i, bool &miss) {
  const int p = g.idx[i];
  if (PLINK) {
    const unsigned char *row = reinterpret_cast<const unsigned char *>(g.src) + s * g.ld;
    const unsigned v = (row[p >> 2] >> (2 * (p & 3))) & 3u;
    miss = (v == 1u);
    return (v == 0u) ? 2.0 : (v == 2u) ? 1.0 : 0.0;
  }
  const double v = (reinterpret_cast<const double *>(g.src) + s * g.ld)[p];
  miss = isnan(v);
  return v;
}

template <bool PLINK>
__global__ __launch_bounds__(MQS_THREADS) void mqs_ingest_kernel(MqsIngest g) {
  __shared__ double red[4];
  __shared__ double wtx[MQS_CMAX], b[MQS_CMAX], part[4][8];
  const long s = blockIdx.x;
  const int n = g.n, c = g.c, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *x = g.X + s * g.ldx;
  double tot = 0.0, cnt = 0.0;
  for (int i = tid; i < n; i += MQS_THREADS) {
    bool miss;
    const double v = mqs_call<PLINK>(g, s, i, miss);
    if (!miss) { tot += v; cnt += 1.0; }
  }
  tot = mqs_bsum(tot, red);
  cnt = mqs_bsum(cnt, red);
  if (cnt == 0.0) { // no called genotype among the analysed individuals: the SNP is dropped (var = 0)
    for (long i = tid; i < g.ldx; i += MQS_THREADS) x[i] = 0.0;
    if (tid == 0) g.var[s] = 0.0;
    return;
  }
  const double mean = tot / cnt;
  for (int i = tid; i < n; i += MQS_THREADS) {
    bool miss;
    double v = mqs_call<PLINK>(g, s, i, miss);
    v = miss ? mean : v;
    x[i] = v + (-1.0 * mean);
  }
  for (long i = n + tid; i < g.ldx; i += MQS_THREADS) x[i] = 0.0;
  // W^T x, eight covariates at a time (each thread reads back only what it wrote itself)
  for (int a0 = 0; a0 < c; a0 += 8) {
    double acc[8];
#pragma unroll
    for (int a = 0; a < 8; ++a) acc[a] = 0.0;
    for (int i = tid; i < n; i += MQS_THREADS) {
      const double xi = x[i];
#pragma unroll
      for (int a = 0; a < 8; ++a)
        if (a0 + a < c) acc[a] += g.Wt[(long)(a0 + a) * g.ldx + i] * xi;
    }
#pragma unroll
    for (int a = 0; a < 8; ++a) acc[a] = wave_sum(acc[a]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < 8; ++a) part[wave][a] = acc[a];
    }
    __syncthreads();
    if (tid < 8 && a0 + tid < c) wtx[a0 + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  }
  __syncthreads();
  if (tid < c) {
    double r = 0.0;
    for (int e = 0; e < c; ++e) r += g.Wi[tid * c + e] * wtx[e];
    b[tid] = r;
  }
  __syncthreads();
  // the residual and ITS sum of squares: a monomorphic SNP is exactly 0 here, as in the reference
  double ss = 0.0;
  for (int i = tid; i < n; i += MQS_THREADS) {
    double r = 0.0;
    for (int a = 0; a < c; ++a) r += g.Wt[(long)a * g.ldx + i] * b[a];
    const double v = x[i] - r;
    x[i] = v;
    ss += v * v;
  }
  ss = mqs_bsum(ss, red);
  if (tid == 0) g.var[s] = ss / (double)n;
}

// One workgroup per category: pos[s] = how many kept SNPs of category cat[s] precede s in the block; cnt[c] = their number.
// flag[0] = 1 when a category index is >= n_vc (every writer stores the same value).
__global__ __launch_bounds__(MQS_SCAN_THREADS) void mqs_scan_kernel(const int *cat, const double *var, long l, int n_vc, int *pos,
                                                                    int *cnt, int *flag) {
  __shared__ int sc[MQS_SCAN_THREADS];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long per = (l + MQS_SCAN_THREADS - 1) / MQS_SCAN_THREADS;
  const long lo = min(l, tid * per), hi = min(l, lo + per);
  int mine = 0;
  for (long s = lo; s < hi; ++s) {
    const int k = cat[s];
    if (k >= n_vc && c == 0) flag[0] = 1;
    if (k == c && var[s] > 0.0) ++mine;
  }
  sc[tid] = mine;
  __syncthreads();
  for (int off = 1; off < MQS_SCAN_THREADS; off <<= 1) { // inclusive scan
    const int add = tid >= off ? sc[tid - off] : 0;
    __syncthreads();
    sc[tid] += add;
    __syncthreads();
  }
  int run = sc[tid] - mine;
  for (long s = lo; s < hi; ++s)
    if (cat[s] == c && var[s] > 0.0) pos[s] = run++;
  if (tid == MQS_SCAN_THREADS - 1) cnt[c] = sc[tid];
}

// One workgroup per SNP: the kept ones go to their panel row, scaled by sqrt(w / var) (src/gemma_io.cpp:3089-3095)
__global__ __launch_bounds__(MQS_THREADS) void mqs_compact_kernel(const double *X, long ldx, long l, const int *cat, const double *var,
                                                                  const double *weight, int n_vc, const int *pos, const int *cnt,
                                                                  double *P) {
  const long s = blockIdx.x;
  const int k = cat[s];
  const double vr = var[s];
  if (k < 0 || k >= n_vc || !(vr > 0.0)) return;
  long row = pos[s];
  for (int e = 0; e < k; ++e) row += cnt[e];
  const double d = (weight ? weight[s] : 1.0) / vr;
  const double sc = sqrt(d);
  const double2 *src = reinterpret_cast<const double2 *>(X + s * ldx);
  double2 *dst = reinterpret_cast<double2 *>(P + row * ldx);
  for (long i = threadIdx.x; i < ldx / 2; i += MQS_THREADS) { // ldx is even, both bases are 16-byte aligned
    double2 v = src[i];
    v.x *= sc;
    v.y *= sc;
    dst[i] = v;
  }
}

// upper triangle / div, mirrored (the end of PlinkKin, src/gemma_io.cpp:3143-3154: `d /= ns`, a division as there)
__global__ void mqs_symm_scale_kernel(double *K, long n, long ld, double div) {
  __shared__ double tile[32][33];
  const int bx = blockIdx.x, by = blockIdx.y;
  if (bx < by) return;
  const int tx = threadIdx.x, ty = threadIdx.y; // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const long i = (long)by * 32 + r, j = (long)bx * 32 + tx;
    double v = 0.0;
    if (i < n && j < n) {
      v = K[i * ld + j] / div;
      if (j >= i) K[i * ld + j] = v;
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const long j = (long)bx * 32 + r, i = (long)by * 32 + tx;
    if (i < n && j < n && j > i) K[j * ld + i] = tile[tx][r];
  }
}

// rs[r] = sum_j M[r][j], dg[r] = M[r][r]; one wavefront per row
__global__ __launch_bounds__(MQS_THREADS) void mqs_rowstat_kernel(const double *M, long n, long ld, double *rs, double *dg) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const double *row = M + r * ld;
  double s = 0.0;
  for (long j = lane; j < n; j += 64) s += row[j];
  s = wave_sum(s);
  if (lane == 0) {
    rs[r] = s;
    dg[r] = row[r];
  }
}

// out[0] = sum(v) (one workgroup)
__global__ __launch_bounds__(1024) void mqs_total_kernel(const double *v, long n, double *out) {
  __shared__ double part[16];
  double s = 0.0;
  for (long i = threadIdx.x; i < n; i += 1024) s += v[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w];
    out[0] = t;
  }
}

// CenterMatrix: G[i][j] += -(Gw[i] + Gw[j]) / n + d / n^2 on the upper triangle, mirrored (src/mathfunc.cpp:160-171)
__global__ __launch_bounds__(256) void mqs_center_kernel(double *G, long n, long ld, const double *Gw, const double *d) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double alpha = -1.0 / (double)n;
  const double beta = (*d) / ((double)n * (double)n);
  for (long i = blockIdx.y; i <= j; i += gridDim.y) {
    double v = G[i * ld + j];
    v += alpha * Gw[i] + alpha * Gw[j];
    v += beta;
    G[i * ld + j] = v;
    if (j != i) G[j * ld + i] = v;
  }
}

// ScaleMatrix: G *= 1 / (tr / n) unless the mean diagonal is 0; tr[0] = the trace
__global__ __launch_bounds__(256) void mqs_scale_kernel(double *G, long n, long ld, const double *tr) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const double d = tr[0] / (double)n;
  if (d == 0.0) return;
  for (long i = blockIdx.y; i < n; i += gridDim.y) G[i * ld + j] *= 1.0 / d;
}

// One wavefront per row t of the ordered pair (A, K):  huv[t] = sum_k A[t,k] K[t,k],  huv[n + t] = sum_k A[t,k] sK[k],
// huv[2 n + t] = sum_k K[t,k] sA[k].  VEC: ld even and 16-byte aligned bases, two doubles per load.
template <bool VEC>
__global__ __launch_bounds__(MQS_THREADS) void mqs_pair_kernel(const double *A, const double *K, long n, long ld, const double *sA,
                                                               const double *sK, double *huv) {
  const int lane = threadIdx.x & 63;
  const long t = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= n) return;
  const double *a = A + t * ld, *k = K + t * ld;
  double h = 0.0, u = 0.0, v = 0.0;
  if (VEC) {
    const long n2 = n / 2;
    const double2 *a2 = reinterpret_cast<const double2 *>(a), *k2 = reinterpret_cast<const double2 *>(k);
    const double2 *sa2 = reinterpret_cast<const double2 *>(sA), *sk2 = reinterpret_cast<const double2 *>(sK);
    for (long j = lane; j < n2; j += 64) {
      const double2 av = a2[j], kv = k2[j], sa = sa2[j], sk = sk2[j];
      h += av.x * kv.x;
      u += av.x * sk.x;
      v += kv.x * sa.x;
      h += av.y * kv.y;
      u += av.y * sk.y;
      v += kv.y * sa.y;
    }
    if ((n & 1) && lane == 0) {
      h += a[n - 1] * k[n - 1];
      u += a[n - 1] * sK[n - 1];
      v += k[n - 1] * sA[n - 1];
    }
  } else {
    for (long j = lane; j < n; j += 64) {
      h += a[j] * k[j];
      u += a[j] * sK[j];
      v += k[j] * sA[j];
    }
  }
  h = wave_sum(h);
  u = wave_sum(u);
  v = wave_sum(v);
  if (lane == 0) {
    huv[t] = h;
    huv[n + t] = u;
    huv[2 * n + t] = v;
  }
}

} // namespace gemma_hip

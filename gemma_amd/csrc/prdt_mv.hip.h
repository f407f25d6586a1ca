// Kinship-only prediction for several phenotypes (GEMMA -predict 1 with -k and -n a b c, a_mode 43): the Kronecker system of
//   src/gemma.cpp:1821-1871 (H_full = G (x) Vg + I (x) Ve) and PRDT::MvnormPrdt, src/prdt.cpp:448-553
// without H_full and H_mo.  Entries are ordered i * d + a (individual-major, as KroneckerSym and MvnormPrdt order them).  With Gc the
// centred kinship, o the observed (i, a) pairs in that order and r = (Y - W B^T)[o]:
//   H_oo[(i,a),(j,b)] = Gc_ij Vg_ab + delta_ij Ve_ab      assembled here from Gc and the index lists (upper triangle)
//   z = H_oo^-1 r                                          Cholesky factor + two triangular solves (spd_inv.hip.h)
//   Z (ni x d) = z scattered, zero at the unobserved entries
//   y_miss_ia = (W B^T)_ia + (Gc Z Vg + Z Ve)_ia           on the unobserved entries: the reference's H_mo z, of which the I (x) Ve
//                                                          term couples a missing entry to the observed traits of the same individual
// The observed individuals are counted by rank: ou[p] = the rank of entry p's individual among the individuals with an observed
// trait, ui[rank] = that individual.  The ranks of consecutive entries are equal or consecutive (the individuals themselves are not,
// where an individual has no observed trait), so a 64 x 64 tile of H_oo needs at most a 64 x 64 sub-tile of Gc.
#pragma once
#include <hip/hip_runtime.h>

namespace gemma_hip {

constexpr int PMV_TILE = 64;  // rows and columns of H_oo per workgroup
constexpr int PMV_DMAX = 8;   // GEMMA_MV_DMAX
constexpr int PMV_CMAX = 12;  // GEMMA_MV_CMAX

struct PmvSmall { // Vg, Ve (d x d, ld d) and B (d x c, ld c) as kernel arguments
  double Vg[PMV_DMAX * PMV_DMAX], Ve[PMV_DMAX * PMV_DMAX], B[PMV_DMAX * PMV_CMAX];
  int d, c;
};

// The upper triangle of H_oo (N x N, lda): one workgroup per 64 x 64 tile on or above the diagonal.  The Gc sub-tile of the tile's
// individuals is loaded once into LDS (up to d-fold reuse: d consecutive entries share an individual); every thread then writes up to
// 16 entries of one column, so a wavefront's stores are contiguous.  Only entries with row <= column are written; no atomics;
// 64-bit element offsets (N * lda passes 2^31 from N = 46 341).
static __global__ __launch_bounds__(256) void prdt_mv_assemble_kernel(const double *Gc, long ldg, const int *ou, const int *oa, const int *ui,
                                                                     long N, PmvSmall sm, double *H, long lda) {
  if (blockIdx.x < blockIdx.y) return; // below the diagonal
  __shared__ double T[PMV_TILE][PMV_TILE + 1];
  __shared__ double vg[PMV_DMAX * PMV_DMAX], ve[PMV_DMAX * PMV_DMAX];
  const int tid = threadIdx.x;
  const long p0 = (long)blockIdx.y * PMV_TILE, q0 = (long)blockIdx.x * PMV_TILE;
  const long p1 = min(p0 + PMV_TILE, N) - 1, q1 = min(q0 + PMV_TILE, N) - 1; // last row / column of the tile
  const int ru0 = ou[p0], cu0 = ou[q0];
  const int nr = ou[p1] - ru0 + 1, nc = ou[q1] - cu0 + 1; // <= 64 each: ranks rise by at most one per entry
  if (tid < sm.d * sm.d) {
    vg[tid] = sm.Vg[tid];
    ve[tid] = sm.Ve[tid];
  }
  for (int idx = tid; idx < nr * PMV_TILE; idx += 256) {
    const int rr = idx / PMV_TILE, cc = idx - rr * PMV_TILE;
    if (cc < nc) T[rr][cc] = Gc[(long)ui[ru0 + rr] * ldg + ui[cu0 + cc]];
  }
  __syncthreads();
  const long q = q0 + (tid & 63);
  if (q > q1) return;
  const int uq = ou[q], b = oa[q];
  for (int k = tid >> 6; k < PMV_TILE; k += 4) {
    const long p = p0 + k;
    if (p > p1 || p > q) break; // p rises with k
    const int up = ou[p], a = oa[p];
    double h = T[up - ru0][uq - cu0] * vg[a * sm.d + b];
    if (up == uq) h += ve[a * sm.d + b];
    H[p * lda + q] = h;
  }
}

// r[p] = Y_ia - (W B^T)_ia at the observed entries (i, a) = (oi[p], oa[p])
static __global__ void prdt_mv_resid_kernel(const double *Y, const double *W, const int *oi, const int *oa, long N, PmvSmall sm, double *r) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  const long i = oi[p];
  const int a = oa[p];
  double f = 0.0;
  for (int k = 0; k < sm.c; ++k) f += W[i * sm.c + k] * sm.B[a * sm.c + k];
  r[p] = Y[i * sm.d + a] - f;
}

// Z (ni x d, zeroed before): Z_ia = z[p]
static __global__ void prdt_mv_scatter_kernel(const double *z, const int *oi, const int *oa, long N, int d, double *Z) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= N) return;
  Z[(long)oi[p] * d + oa[p]] = z[p];
}

// y_miss[m] = (W B^T)_ia + sum_b (Gc Z)_ib Vg_ba + Z_ib Ve_ba at the unobserved entries (i, a) = (mi[m], ma[m])
static __global__ void prdt_mv_epilogue_kernel(const double *GZ, const double *Z, const double *W, const int *mi, const int *ma, long M,
                                               PmvSmall sm, double *y_miss) {
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const long i = mi[m];
  const int a = ma[m], d = sm.d;
  double f = 0.0;
  for (int k = 0; k < sm.c; ++k) f += W[i * sm.c + k] * sm.B[a * sm.c + k];
  double g = 0.0;
  for (int b = 0; b < d; ++b) g += GZ[i * d + b] * sm.Vg[b * d + a] + Z[i * d + b] * sm.Ve[b * d + a];
  y_miss[m] = f + g;
}

// out (n x n, dense) = G[pos[a]][pos[b]]: the kinship of the individuals with every trait, as ReadFile_kin selects it
static __global__ void prdt_mv_sub_kernel(const double *G, long ldg, const int *pos, long n, double *out) {
  const long b = (long)blockIdx.x * 256 + threadIdx.x;
  const long a = blockIdx.y;
  if (b >= n) return;
  out[a * n + b] = G[(long)pos[a] * ldg + pos[b]];
}

} // namespace gemma_hip

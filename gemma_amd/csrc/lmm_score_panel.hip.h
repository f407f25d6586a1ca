// Score-test panel: (beta, se, p_score) of `-lmm 3` for T phenotypes x l SNPs straight from one U^T x (gemma_hip_lmm_score_panel_*).
//
// CalcRLScore (GEMMA src/lmm.cpp:1170-1211) evaluates CalcPab (:311-350) at the phenotype's null lambda -- no search per SNP.
// CalcPab eliminates the covariates one after the other in the inner product weighted by h_i = 1 / (lambda delta_i + 1); that is
// the full projection, so with S_ww = UtW^T diag(h) UtW = L L^T, v = S_ww^-1 UtW^T (h . y), r = y - UtW v, w~_a = column a of
// UtW L^-T and P_yy = sum h y^2 - (UtW^T (h . y)) . v:
//     P_xy = sum_i h_i x_i r_i,     P_xx = sum_i h_i x_i^2 - sum_a (sum_i h_i x_i w~_ai)^2
// and beta, se, p_score follow per (SNP, phenotype) pair without a recursion.  All pairs of a block are ONE skinny product of
// [X.X | X] (l x n) against a weight matrix of c + 2 columns ("kinds") per phenotype: h (against x^2), h . r and h . w~_a (against x).
//
// Weight matrix, in the B-operand order of v_mfma_f64_16x16x4_f64 (as grid_weights_kernel of lmm_grid.hip.h):
//     Rp[chunk][group][kind][kq][col][j],   i = 16 chunk + 4 kq + j,   phenotype t = 16 group + col,
// i.e. a 16-wide column block holds 16 phenotypes of ONE kind: lane (col, kq) of a wave holds, in every one of the c + 2
// accumulator blocks of a (row group, phenotype group) pair, the same (SNP, phenotype) positions -- the epilogue is per lane.
// Zero beyond n and beyond T.
//
// Two output forms of the one product: the records form (T x l records of beta, se, p_score) and the hits form (the pairs with
// p_score <= p_max in a caller-sized list, and the best pair of every phenotype) -- see SP_PXX_FLOOR / SP_FCRIT_MARGIN below.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <climits>
#include "dgemm.h"
#include "lmm_assoc.hip.h"
#define GEMMA_HIP_KERNEL_BODIES // a unit that includes this file instantiates what it launches: lmm_score_panel.h leaves out its extern templates
#include "lmm_score_panel.h"

namespace gemma_hip {

// One workgroup per phenotype: the Gram matrix at its lambda, its Cholesky factor, v and P_yy, then the phenotype's c + 2 weight
// columns.  bad: the smallest phenotype index whose Gram matrix is not positive definite (INT_MAX: none) -- its columns stay zero.
// UtWt: c x n, Yt: T x n.
__global__ __launch_bounds__(256) void score_setup_kernel(ScoreGeom g, const double *__restrict__ eval,
                                                         const double *__restrict__ UtWt, const double *__restrict__ Yt,
                                                         const double *__restrict__ lam, double *__restrict__ Rp,
                                                         double *__restrict__ Pyy, int *__restrict__ bad) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int c = g.c, n = g.n;
  const double l = lam[t];
  const double *y = Yt + (long)t * n;
  __shared__ double S[SP_CMAX][SP_CMAX + 1]; // the Gram matrix, then L in its lower triangle
  __shared__ double bv[SP_CMAX];             // UtW^T (h . y), then v
  __shared__ double dv[SP_CMAX];             // the refinement of v
  __shared__ double syy;
  __shared__ int ok;
  // the (c + 1)(c + 2) / 2 weighted sums, one wave per sum (fixed order: lanes stride over i, then the butterfly)
  const int np = c * (c + 1) / 2, nsum = np + c + 1;
  for (int p = wave; p < nsum; p += 4) {
    int a = 0, b = 0;
    const double *ua = y, *ub = y;
    if (p < np) {
      int q = p;
      while (q > a) { q -= a + 1; ++a; }
      b = q;
      ua = UtWt + (long)a * n;
      ub = UtWt + (long)b * n;
    } else if (p < np + c) {
      a = p - np;
      ua = UtWt + (long)a * n;
    }
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += ua[i] * ub[i] / (l * eval[i] + 1.0);
    s = wave_sum(s);
    if (lane == 0) {
      if (p < np) { S[a][b] = s; S[b][a] = s; }
      else if (p < np + c) bv[a] = s;
      else syy = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int good = 1;
    for (int j = 0; j < c && good; ++j) {
      const double sjj = S[j][j];
      double d = sjj;
      for (int k = 0; k < j; ++k) d -= S[j][k] * S[j][k];
      if (!(d > SP_PIVOT_MIN * sjj) || !(d <= DBL_MAX)) { good = 0; break; }
      const double ljj = sqrt(d);
      S[j][j] = ljj;
      for (int i = j + 1; i < c; ++i) {
        double e = S[i][j];
        for (int k = 0; k < j; ++k) e -= S[i][k] * S[j][k];
        S[i][j] = e / ljj;
      }
    }
    if (good) {
      double q = 0.0; // |L^-1 b|^2 = b . S^-1 b
      for (int a = 0; a < c; ++a) {
        double z = bv[a];
        for (int k = 0; k < a; ++k) z -= S[a][k] * bv[k];
        z /= S[a][a];
        bv[a] = z;
        q += z * z;
      }
      for (int a = c - 1; a >= 0; --a) {
        double z = bv[a];
        for (int k = a + 1; k < c; ++k) z -= S[k][a] * bv[k];
        bv[a] = z / S[a][a];
      }
      Pyy[t] = syy - q;
    } else {
      Pyy[t] = NAN;
      atomicMin(bad, t);
    }
    ok = good;
  }
  __syncthreads();
  if (!ok) return;
  // One step of iterative refinement on v.  r0 = y - UtW v carries the rounding of v, W (v* - v), which is NOT orthogonal to the
  // covariates: at lambda = 1e5 the weight of the direction with delta = 0 is 1 beside 1e-5 for the rest, x and the intercept are
  // large there, and h x r0 of that one direction puts 1e-14 into a P_xy of 1e-8 for a SNP with |z| of 1e-4.  dv = S_ww^-1 UtW^T (h . r0)
  // is that rounding, and r = r0 - UtW dv (v and dv kept apart: v + dv would round again) is orthogonal to the covariates to fp64.
  for (int a = wave; a < c; a += 4) {
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {
      double r0 = y[i];
      for (int b = 0; b < c; ++b) r0 -= UtWt[(long)b * n + i] * bv[b];
      s += UtWt[(long)a * n + i] * r0 / (l * eval[i] + 1.0);
    }
    s = wave_sum(s);
    if (lane == 0) dv[a] = s;
  }
  __syncthreads();
  if (tid == 0) {
    for (int a = 0; a < c; ++a) {
      double z = dv[a];
      for (int k = 0; k < a; ++k) z -= S[a][k] * dv[k];
      dv[a] = z / S[a][a];
    }
    for (int a = c - 1; a >= 0; --a) {
      double z = dv[a];
      for (int k = a + 1; k < c; ++k) z -= S[k][a] * dv[k];
      dv[a] = z / S[a][a];
    }
  }
  __syncthreads();
  double *rt = Rp + ((long)(t >> 4) * g.nk) * 256 + (t & 15) * 4;
  const long chunk_stride = (long)g.ng * g.nk * 256;
  for (int i = tid; i < n; i += 256) {
    const double h = 1.0 / (l * eval[i] + 1.0);
    double r = y[i], rd = 0.0;
    double w[SP_CMAX];
#pragma unroll
    for (int a = 0; a < SP_CMAX; ++a) {
      w[a] = 0.0;
      if (a < c) {
        const double wa = UtWt[(long)a * n + i];
        r -= wa * bv[a];
        rd += wa * dv[a];
        double z = wa;
#pragma unroll
        for (int k = 0; k < a; ++k) z -= S[a][k] * w[k];
        w[a] = z / S[a][a];
      }
    }
    double *re = rt + (long)(i >> 4) * chunk_stride + ((i >> 2) & 3) * 64 + (i & 3);
    re[0] = h;
    re[256] = h * (r - rd);
#pragma unroll
    for (int a = 0; a < SP_CMAX; ++a)
      if (a < c) re[(2 + a) * 256] = h * w[a];
  }
}

// The epilogue arithmetic of CalcRLScore, shared by the records form, the hits form and score_best_kernel: the same operations
// in the same order, so a hit and a best carry the bits of the record of their pair.
__device__ __forceinline__ double score_F(double nd, double P_xx, double P_xy, double P_yy) {
  return nd * P_xy * P_xy / (P_yy * P_xx);
}
__device__ __forceinline__ ScoreRec score_stats(double nd, double df, double lnbeta_half_df, double P_xx, double P_xy, double P_yy) {
  ScoreRec o;
  o.beta = P_xy / P_xx;
  const double Px_yy = P_yy - P_xy * P_xy / P_xx;
  const double tau = df / Px_yy;
  o.se = safe_sqrt_dev(1.0 / (tau * P_xx));
  o.p_score = fdist_Q1_dev(score_F(nd, P_xx, P_xy, P_yy), df, lnbeta_half_df);
  return o;
}
// (F, row) of b before (F, row) of a: larger F, the smaller row among equals
__device__ __forceinline__ bool score_better(double Fb, long long rb, double Fa, long long ra) {
  return Fb > Fa || (Fb == Fa && rb < ra);
}

// One thread: the pre-filter's threshold of (p_max, df), see SP_FCRIT_MARGIN.
__global__ void score_fcrit_kernel(double p_max, double df, double lnbeta_half_df, double *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (!(p_max < SP_FCRIT_PMAX)) {
    *out = -INFINITY;
    return;
  }
  const double pe = p_max > SP_FCRIT_PMIN ? p_max : SP_FCRIT_PMIN;
  double lo = 0.0, hi = 1.0; // Q^(0) = 1 > pe
  for (;;) {
    const double q = fdist_Q1_dev(hi, df, lnbeta_half_df);
    if (q > pe && hi < 1e300) { lo = hi; hi *= 2.0; }
    else break;
  }
  for (int it = 0; it < 64; ++it) {
    const double mid = 0.5 * (lo + hi);
    const double q = fdist_Q1_dev(mid, df, lnbeta_half_df);
    if (q > pe) lo = mid;
    else if (q <= pe) hi = mid;
    else break;
  }
  *out = lo * (1.0 - SP_FCRIT_MARGIN);
}

// One K pass of a wave: NK kinds (FIRST: kind 0 is h against x^2 -- the fragment squared in registers --, kind 1 h . r; the rest
// and every kind of a later pass: h . w~_a) for SP_RG row groups x SP_PG phenotype groups.  rp[q]: the lane's operand of chunk 0,
// phenotype group q, first kind of the pass.  pxx / pxy: the running P_xx and P_xy of the lane's positions.
// HITS (first pass): sx takes sum h x^2 of the positions as floats (SP_PXX_FLOOR).
template <int NK, bool FIRST, bool AL, bool HITS = false>
__device__ __forceinline__ void score_pass(const ScoreArgs &a, const double *const (&xr)[SP_RG], const double *const (&rp)[SP_PG],
                                           int kq, double (&pxx)[SP_NPOS], double (&pxy)[SP_NPOS], float *sx = nullptr) {
  f64x4 acc[SP_RG][SP_PG][NK];
#pragma unroll
  for (int g = 0; g < SP_RG; ++g)
#pragma unroll
    for (int q = 0; q < SP_PG; ++q)
#pragma unroll
      for (int k = 0; k < NK; ++k) acc[g][q][k] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int n = a.g.n;
  const long cs = (long)a.g.ng * a.g.nk * 256;
  const int nfull = n / 16;
  double rb[SP_PG][NK][4], xv[SP_RG][4];
#define SP_LOAD_R(CH)                                                                       \
  do {                                                                                      \
    _Pragma("unroll") for (int q = 0; q < SP_PG; ++q) {                                     \
      _Pragma("unroll") for (int k = 0; k < NK; ++k) {                                      \
        const double *p_ = rp[q] + (long)(CH) * cs + k * 256;                               \
        const f64x2 lo = *reinterpret_cast<const f64x2 *>(p_);                              \
        const f64x2 hi = *reinterpret_cast<const f64x2 *>(p_ + 2);                          \
        rb[q][k][0] = lo.x; rb[q][k][1] = lo.y; rb[q][k][2] = hi.x; rb[q][k][3] = hi.y;     \
      }                                                                                     \
    }                                                                                       \
  } while (0)
#define SP_MFMA()                                                                           \
  do {                                                                                      \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) {                                         \
      _Pragma("unroll") for (int g = 0; g < SP_RG; ++g) {                                   \
        const double xs = xv[g][j] * xv[g][j];                                              \
        _Pragma("unroll") for (int q = 0; q < SP_PG; ++q) {                                 \
          _Pragma("unroll") for (int k = 0; k < NK; ++k)                                    \
            acc[g][q][k] = __builtin_amdgcn_mfma_f64_16x16x4f64((FIRST && k == 0) ? xs : xv[g][j], rb[q][k][j], acc[g][q][k], 0, 0, 0); \
        }                                                                                   \
      }                                                                                     \
    }                                                                                       \
  } while (0)
  for (int ch = 0; ch < nfull; ++ch) {
    SP_LOAD_R(ch);
#pragma unroll
    for (int g = 0; g < SP_RG; ++g) {
      const double *x_ = xr[g] + (long)ch * 16;
      if (AL) {
        const f64x2 lo = *reinterpret_cast<const f64x2 *>(x_);
        const f64x2 hi = *reinterpret_cast<const f64x2 *>(x_ + 2);
        xv[g][0] = lo.x; xv[g][1] = lo.y; xv[g][2] = hi.x; xv[g][3] = hi.y;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) xv[g][j] = x_[j];
      }
    }
    SP_MFMA();
  }
  if (a.g.nc > nfull) { // the partial chunk of a ragged n: the weights are zero beyond n, the row is not read there
    const int ch = nfull;
    const long k0 = (long)ch * 16 + 4 * kq;
    SP_LOAD_R(ch);
#pragma unroll
    for (int g = 0; g < SP_RG; ++g)
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[g][j] = (k0 + j < n) ? xr[g][(long)ch * 16 + j] : 0.0;
    SP_MFMA();
  }
#undef SP_LOAD_R
#undef SP_MFMA
  // accumulator r of a lane: row kq + 4 r of the row group, column (lane & 15) of the phenotype group
#pragma unroll
  for (int g = 0; g < SP_RG; ++g)
#pragma unroll
    for (int q = 0; q < SP_PG; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int e = (g * SP_PG + q) * 4 + r;
        if (FIRST) {
          pxx[e] = acc[g][q][0][r];
          pxy[e] = acc[g][q][1][r];
          if (HITS) sx[e] = (float)acc[g][q][0][r];
        }
#pragma unroll
        for (int k = FIRST ? 2 : 0; k < NK; ++k) pxx[e] -= acc[g][q][k][r] * acc[g][q][k][r];
      }
}

// grid: ceil(ng / (2 SP_PG)) phenotype tiles (fastest: the workgroups that share SNP rows run together) x ceil(l / (32 SP_RG)) SNP
// tiles, linear in blockIdx.x; 4 waves = 2 (rows) x 2 (phenotype groups).  c + 2 <= SP_KP kinds: one pass over K; more: further
// passes of up to SP_KP kinds h . w~_a each, P_xx and P_xy kept in registers.
// HITS: the same K passes, then instead of the T x l records the pairs with p_score <= p_max appended to a.hits (one slot claim
// per wave and step: ballot, one atomicAdd of the wave's count, the lanes' ranks in the ballot) and the wave's best pair of each
// of its phenotypes written to its own cell of a.cells (no atomics: score_best_kernel reduces the cells in a fixed order).  The
// F tail runs only where F passes the pre-filter.
template <bool AL, bool HITS>
__global__ __launch_bounds__(256, 2) void score_panel_kernel(ScoreArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = lane & 15, kq = lane >> 4;
  const int npt = (a.g.ng + 2 * SP_PG - 1) / (2 * SP_PG);
  const int pt = (int)(blockIdx.x % (unsigned)npt);
  const long st = (long)(blockIdx.x / (unsigned)npt);
  const long s0 = (st * 2 + (wave & 1)) * (SP_RG * 16);
  const int g0 = (pt * 2 + (wave >> 1)) * SP_PG;
  if (s0 >= a.l || g0 >= a.g.ng) return;
  const double *xr[SP_RG];
#pragma unroll
  for (int g = 0; g < SP_RG; ++g) {
    long row = s0 + g * 16 + i;
    if (row >= a.l) row = a.l - 1;
    xr[g] = a.UtX + row * a.ld + 4 * kq;
  }
  int grp[SP_PG];
  const double *rp[SP_PG];
#pragma unroll
  for (int q = 0; q < SP_PG; ++q) {
    grp[q] = g0 + q < a.g.ng ? g0 + q : a.g.ng - 1; // a group past the end: computed on the last one, not stored
    rp[q] = a.Rp + (long)grp[q] * a.g.nk * 256 + lane * 4;
  }
  double pxx[SP_NPOS], pxy[SP_NPOS];
  float sx[SP_NPOS]; // the hits form only (never written or read by the records form)
  const int nk = a.g.nk;
  if (nk == 3) score_pass<3, true, AL, HITS>(a, xr, rp, kq, pxx, pxy, sx);
  else score_pass<4, true, AL, HITS>(a, xr, rp, kq, pxx, pxy, sx);
  for (int k0 = SP_KP; k0 < nk; k0 += SP_KP) {
    const double *rq[SP_PG];
#pragma unroll
    for (int q = 0; q < SP_PG; ++q) rq[q] = rp[q] + k0 * 256;
    const int left = nk - k0;
    if (left >= 4) score_pass<4, false, AL>(a, xr, rq, kq, pxx, pxy);
    else if (left == 3) score_pass<3, false, AL>(a, xr, rq, kq, pxx, pxy);
    else if (left == 2) score_pass<2, false, AL>(a, xr, rq, kq, pxx, pxy);
    else score_pass<1, false, AL>(a, xr, rq, kq, pxx, pxy);
  }
  // CalcRLScore from (P_xx, P_xy, P_yy), one position at a time (the F tail is long: not unrolled SP_NPOS times)
  const double nd = (double)a.g.n, df = (double)(a.g.n - a.g.c - 1);
  if (!HITS) {
#pragma unroll 1
    for (int e = 0; e < SP_NPOS; ++e) {
      double P_xx = 0.0, P_xy = 0.0;
#pragma unroll
      for (int k = 0; k < SP_NPOS; ++k)
        if (k == e) { P_xx = pxx[k]; P_xy = pxy[k]; }
      const int g = e / (SP_PG * 4), q = (e >> 2) % SP_PG, r = e & 3;
      const long row = s0 + g * 16 + kq + 4 * r;
      const int t = (g0 + q) * 16 + i;
      if (row >= a.l || t >= a.g.T) continue;
      a.out[(long)t * a.l + row] = score_stats(nd, df, a.lnbeta_half_df, P_xx, P_xy, a.Pyy[t]);
    }
    return;
  }
  const double f_thr = *a.f_thr;
  double bF[SP_PG], bxx[SP_PG], bxy[SP_PG];
  long long brow[SP_PG];
#pragma unroll
  for (int q = 0; q < SP_PG; ++q) { bF[q] = -INFINITY; bxx[q] = 0.0; bxy[q] = 0.0; brow[q] = -1; }
#pragma unroll 1
  for (int e = 0; e < SP_NPOS; ++e) { // e is wave-uniform: every lane reaches the ballot
    double P_xx = 0.0, P_xy = 0.0;
    float shx2 = 0.0f;
#pragma unroll
    for (int k = 0; k < SP_NPOS; ++k)
      if (k == e) { P_xx = pxx[k]; P_xy = pxy[k]; shx2 = sx[k]; }
    const int g = e / (SP_PG * 4), q = (e >> 2) % SP_PG, r = e & 3;
    const long row = s0 + g * 16 + kq + 4 * r;
    const int t = (g0 + q) * 16 + i;
    const bool inside = row < a.l && t < a.g.T;
    const double P_yy = inside ? a.Pyy[t] : NAN;
    const double F = score_F(nd, P_xx, P_xy, P_yy);
    const bool sound = inside && P_xx >= SP_PXX_FLOOR * (double)shx2; // false on NaN
    if (sound && F <= DBL_MAX) { // finite (NaN compares false)
#pragma unroll
      for (int qq = 0; qq < SP_PG; ++qq)
        if (qq == q && (brow[qq] < 0 || score_better(F, row, bF[qq], brow[qq]))) { bF[qq] = F; bxx[qq] = P_xx; bxy[qq] = P_xy; brow[qq] = row; }
    }
    bool hit = false;
    ScoreRec o;
    if (sound && F >= f_thr) {
      o = score_stats(nd, df, a.lnbeta_half_df, P_xx, P_xy, P_yy);
      hit = o.p_score <= a.p_max;
    }
    const unsigned long long m = __ballot(hit);
    if (m != 0) {
      unsigned long long base = 0;
      const int leader = __ffsll((long long)m) - 1;
      if (lane == leader) base = atomicAdd(a.n_hits, (unsigned long long)__popcll(m));
      base = __shfl(base, leader);
      const unsigned long long slot = base + (unsigned long long)__popcll(m & ((1ULL << lane) - 1ULL));
      if (hit && slot < a.cap) {
        ScoreHit h;
        h.snp = (unsigned int)row; h.pheno = (unsigned int)t;
        h.beta = o.beta; h.se = o.se; h.p_score = o.p_score;
        a.hits[slot] = h;
      }
    }
  }
  if (a.cells == nullptr) return;
  // the lanes (i, kq = 0 .. 3) hold the four row quarters of phenotype column i
#pragma unroll
  for (int q = 0; q < SP_PG; ++q) {
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
      const double oF = __shfl_xor(bF[q], off), oxx = __shfl_xor(bxx[q], off), oxy = __shfl_xor(bxy[q], off);
      const long long orow = __shfl_xor(brow[q], off);
      if (orow >= 0 && (brow[q] < 0 || score_better(oF, orow, bF[q], brow[q]))) { bF[q] = oF; bxx[q] = oxx; bxy[q] = oxy; brow[q] = orow; }
    }
    const int t = (g0 + q) * 16 + i;
    if (kq == 0 && t < a.g.T) {
      ScoreCell c;
      c.F = bF[q]; c.P_xx = bxx[q]; c.P_xy = bxy[q]; c.row = brow[q];
      a.cells[(s0 / 32) * (long)a.g.T + t] = c;
    }
  }
}

// One thread per phenotype: the best of its cells over the row tiles in ascending order (a later tile wins only with a larger F:
// ties stay with the smallest row), then the statistics of that one pair.  No pair: snp -1, NaN.
__global__ __launch_bounds__(256) void score_best_kernel(ScoreGeom g, long ntile, const ScoreCell *__restrict__ cells,
                                                        const double *__restrict__ Pyy, double lnbeta_half_df,
                                                        ScoreBest *__restrict__ best) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= g.T) return;
  ScoreCell b;
  b.F = -INFINITY; b.P_xx = 0.0; b.P_xy = 0.0; b.row = -1;
  for (long k = 0; k < ntile; ++k) {
    const ScoreCell c = cells[k * (long)g.T + t];
    if (c.row >= 0 && (b.row < 0 || score_better(c.F, c.row, b.F, b.row))) b = c;
  }
  ScoreBest o;
  o.beta = NAN; o.se = NAN; o.p_score = NAN; o.snp = -1;
  if (b.row >= 0) {
    const ScoreRec r = score_stats((double)g.n, (double)(g.n - g.c - 1), lnbeta_half_df, b.P_xx, b.P_xy, Pyy[t]);
    o.beta = r.beta; o.se = r.se; o.p_score = r.p_score; o.snp = b.row;
  }
  best[t] = o;
}

} // namespace gemma_hip

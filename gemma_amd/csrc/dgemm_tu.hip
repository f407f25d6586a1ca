// The fp64 MFMA GEMM, once for the whole library: its kernels (dgemm_mfma.hip.h), the launch plan, the side stream and the
// GEMMA_HIP_GEMM_* switches (each read once per process).  Every other unit includes dgemm.h.
#include "dgemm_mfma.hip.h"

namespace gemma_hip {

// Wavefronts per 128x128 block: 4 (2x2 waves of 64x64, 2 waves/SIMD at 2 blocks/CU; default) or 8 (2x4 waves
// of 64x32, 4 waves/SIMD; GEMMA_HIP_GEMM_WAVES=8).  Measured at M=N=K=20000 (profiles/r01_gemm_variants.txt):
// the 8-wave form is 1.7 % faster (238.8 vs 242.6 ms) but its blocks drift apart inside an XCD and the L2 hit
// rate drops from 82 % to 17 % (fabric traffic x4); the 4-wave form keeps the co-scheduled tiles in step.
static inline int gemm_waves() {
  static int nw = 0;
  if (nw == 0) {
    const char *e = getenv("GEMMA_HIP_GEMM_WAVES");
    nw = (e && e[0] == '8') ? 8 : 4;
  }
  return nw;
}

// GEMMA_HIP_GEMM_PIPE=0/1/2: interior kernel = register-staged / + software-pipelined fragments / direct-to-LDS with
// pinned interleaved issue (default; 243 -> 238 -> 219 ms at M = N = K = 20000)
static inline int gemm_pipe() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("GEMMA_HIP_GEMM_PIPE");
    v = e ? atoi(e) : 2;
  }
  return v;
}

static inline bool gemm_clamp() { // GEMMA_HIP_GEMM_CLAMP=0: ragged strips through the bounds-checked kernel
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("GEMMA_HIP_GEMM_CLAMP");
    v = (e && e[0] == '0') ? 0 : 1;
  }
  return v == 1;
}

template <bool A_KM, bool B_KN, bool FULL>
static inline hipError_t launch_dgemm_grid(const GemmArgs &g, hipStream_t s) {
  int nblocks;
  if (g.syrk_upper)
    nblocks = g.tiles_m * (g.tiles_m + 1) / 2;
  else
    nblocks = g.tiles_m * g.tiles_n;
  if (nblocks <= 0) return hipSuccess;
  if (FULL && gemm_pipe() == 2 && !g.square_a)
    hipLaunchKernelGGL((dgemm_mfma_glds_kernel<A_KM, B_KN>), dim3(nblocks, g.kslices), dim3(256), 0, s, g);
  else if (FULL && gemm_pipe())
    hipLaunchKernelGGL((dgemm_mfma_pipe_kernel<A_KM, B_KN>), dim3(nblocks, g.kslices), dim3(256), 0, s, g);
  else if (gemm_waves() == 8)
    hipLaunchKernelGGL((dgemm_mfma_kernel<A_KM, B_KN, 8, FULL>), dim3(nblocks, g.kslices), dim3(512), 0, s, g);
  else
    hipLaunchKernelGGL((dgemm_mfma_kernel<A_KM, B_KN, 4, FULL>), dim3(nblocks, g.kslices), dim3(256), 0, s, g);
  return hipGetLastError();
}

// the side stream of the ragged edge strips (dgemm.h)
GemmAux g_gemm_aux;
void gemm_aux_init() {
  if (g_gemm_aux.stream) return;
  const char *e = getenv("GEMMA_HIP_GEMM_SIDE_STREAM"); // "0": keep everything on the caller's stream
  if (e && e[0] == '0') return;
  if (hipStreamCreateWithFlags(&g_gemm_aux.stream, hipStreamNonBlocking) != hipSuccess ||
      hipEventCreateWithFlags(&g_gemm_aux.ready, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&g_gemm_aux.done, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    g_gemm_aux = GemmAux();
  }
}
void gemm_aux_destroy() {
  if (g_gemm_aux.stream) {
    (void)hipStreamDestroy(g_gemm_aux.stream);
    (void)hipEventDestroy(g_gemm_aux.ready);
    (void)hipEventDestroy(g_gemm_aux.done);
  }
  g_gemm_aux = GemmAux();
}

template <bool A_KM, bool B_KN>
static inline hipError_t launch_dgemm_t(GemmArgs g, hipStream_t s) {
  const int Tm = (int)((g.M + GEMM_BM - 1) / GEMM_BM), Tn = (int)((g.N + GEMM_BN - 1) / GEMM_BN);
  const int Fm = (int)(g.M / GEMM_BM), Fn = (int)(g.N / GEMM_BN); // complete tiles per dimension
  const bool aligned = ((reinterpret_cast<uintptr_t>(g.A) & 15) == 0) && ((g.lda & 1) == 0) &&
                       ((reinterpret_cast<uintptr_t>(g.B) & 15) == 0) && ((g.ldb & 1) == 0);
  hipError_t e;
  // K tail: the first floor(K / 16) * 16 of K through the fast kernels, the remaining < 16 accumulated on top by the
  // bounds-checked one (the eigensolver's divide & conquer merges have arbitrary K)
  if (aligned && g.K > 4 * GEMM_BK && (g.K % GEMM_BK) != 0 && Fm > 0 && Fn > 0 && !g.square_a) {
    const long K0 = (g.K / GEMM_BK) * GEMM_BK, K1 = g.K - K0;
    GemmArgs g0 = g;
    g0.K = K0;
    if ((e = launch_dgemm_t<A_KM, B_KN>(g0, s)) != hipSuccess) return e;
    GemmArgs g1 = g;
    g1.K = K1;
    g1.A = A_KM ? g.A + K0 * g.lda : g.A + K0;
    g1.B = B_KN ? g.B + K0 * g.ldb : g.B + K0;
    g1.beta = 1.0;
    g1.clamp = 0;
    g1.tiles_m = Tm; g1.tiles_n = Tn; g1.tm0 = 0; g1.tn0 = 0;
    if (g.syrk_upper) g1.tiles_n = Tm;
    return launch_dgemm_grid<A_KM, B_KN, false>(g1, s);
  }
  const bool fast = aligned && (g.K % GEMM_BK == 0) && g.K > 0 && Fm > 0 && Fn > 0;
  if (!fast) { // everything through the bounds-checked instantiation
    g.tiles_m = Tm; g.tiles_n = Tn; g.tm0 = 0; g.tn0 = 0;
    return launch_dgemm_grid<A_KM, B_KN, false>(g, s);
  }
  const int syrk = g.syrk_upper;
  g.clamp = 0;
  // beta == 0: ragged last tile rows / columns are shifted back inside the matrix and ride in the same launch
  // (bit-identical rewrites of the overlap); the [k][m] operand of a shifted tile must stay 16-byte aligned
  if (gemm_pipe() >= 2 && !syrk && !g.square_a && g.beta == 0.0 && (Tm > Fm || Tn > Fn) && gemm_clamp() &&
      (!A_KM || (g.M & 1) == 0) && (!B_KN || (g.N & 1) == 0)) {
    g.clamp = 1;
    g.tiles_m = Tm; g.tiles_n = Tn; g.tm0 = 0; g.tn0 = 0;
    return launch_dgemm_grid<A_KM, B_KN, true>(g, s);
  }
  const bool strips = (Tn > Fn) || (Tm > Fm && !syrk);
  const bool side = strips && g_gemm_aux.stream != nullptr && Fm * Fn >= 512;
  hipStream_t es = side ? g_gemm_aux.stream : s; // stream of the edge strips
  if (side) {
    if ((e = hipEventRecord(g_gemm_aux.ready, s)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(es, g_gemm_aux.ready, 0)) != hipSuccess) return e;
  }
  GemmArgs ge = g;
  ge.syrk_upper = 0;
  if (side) { // strips first on the side stream, the big grid on the caller's stream
    if (Tn > Fn) { // ragged right strip: all tile rows (SYRK: tm <= Tn-1 is every row)
      ge.tiles_m = Tm; ge.tiles_n = 1; ge.tm0 = 0; ge.tn0 = Fn;
      if ((e = launch_dgemm_grid<A_KM, B_KN, false>(ge, es)) != hipSuccess) return e;
    }
    if (Tm > Fm && !syrk) { // ragged bottom strip (complete columns only; the corner went with the right strip)
      ge.tiles_m = 1; ge.tiles_n = Fn; ge.tm0 = Fm; ge.tn0 = 0;
      if ((e = launch_dgemm_grid<A_KM, B_KN, false>(ge, es)) != hipSuccess) return e;
    }
  }
  // complete tiles: predicate-free kernel (SYRK: the upper triangle of the Fm x Fm complete tiles)
  g.tiles_m = Fm; g.tiles_n = Fn; g.tm0 = 0; g.tn0 = 0;
  e = launch_dgemm_grid<A_KM, B_KN, true>(g, s);
  if (e != hipSuccess) return e;
  if (side) {
    if ((e = hipEventRecord(g_gemm_aux.done, es)) != hipSuccess) return e;
    return hipStreamWaitEvent(s, g_gemm_aux.done, 0);
  }
  if (Tn > Fn) {
    ge.tiles_m = Tm; ge.tiles_n = 1; ge.tm0 = 0; ge.tn0 = Fn;
    if ((e = launch_dgemm_grid<A_KM, B_KN, false>(ge, s)) != hipSuccess) return e;
  }
  if (Tm > Fm && !syrk) {
    ge.tiles_m = 1; ge.tiles_n = Fn; ge.tm0 = Fm; ge.tn0 = 0;
    if ((e = launch_dgemm_grid<A_KM, B_KN, false>(ge, s)) != hipSuccess) return e;
  }
  return hipSuccess;
}

// ta/tb in {'N','T'} with the cblas row-major meaning; mirror (with syrk_upper, M == N): the lower triangle is written too, as the
// transpose of the upper tiles (GemmArgs::mirror)
hipError_t launch_dgemm(char ta, char tb, long M, long N, long K, double alpha,
                                      const double *A, long lda, const double *B, long ldb,
                                      double beta, double *C, long ldc, bool syrk_upper,
                                      bool square_a, hipStream_t s, bool mirror) {
  GemmArgs g;
  g.mirror = (mirror && (syrk_upper ? M == N : M <= N)) ? 1 : 0; // without syrk_upper: a row strip of such an update (tiles (0, j) of C: the
                                                                 // eigensolver's look-ahead); every tile off the diagonal is also written transposed
  g.A = A; g.B = B; g.C = C;
  g.M = M; g.N = N; g.K = K;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.alpha = alpha; g.beta = beta;
  g.tiles_m = g.tiles_n = 0;
  g.tm0 = g.tn0 = 0;
  g.syrk_upper = syrk_upper ? 1 : 0;
  g.clamp = 0;
  g.square_a = square_a ? 1 : 0;
  {
    static int abl = -1;
    if (abl < 0) {
      const char *e = getenv("GEMMA_HIP_GEMM_ABLATE");
      abl = e ? atoi(e) : 0;
    }
    g.ablate = abl;
    static int gm = -1;
    if (gm < 0) {
      const char *e = getenv("GEMMA_HIP_GEMM_GM");
      gm = e ? atoi(e) : 0;
    }
    g.gm = gm;
  }
  const bool tA = (ta == 'T' || ta == 't'), tB = (tb == 'T' || tb == 't');
  // op(A) = A^T  <=> A stored [k][m]  (KM image);  op(B) = B <=> B stored [k][n] (KN image)
  if (tA && !tB) return launch_dgemm_t<true, true>(g, s);
  if (tA && tB) return launch_dgemm_t<true, false>(g, s);
  if (!tA && !tB) return launch_dgemm_t<false, true>(g, s);
  return launch_dgemm_t<false, false>(g, s);
}

// C_ks (ks = 0 .. *nslices - 1, at C + ks * cslice) = alpha op(A) op(B) over the K range of slice ks, ONE launch per kernel
// variant (interior tiles / edge strips) with the slice in blockIdx.y; the caller adds the slices.  want = slices asked for; the
// number used (returned in *nslices) keeps every slice at least four K-tiles long.  A K that is not a multiple of the K-tile
// leaves its last < 16 columns to one extra bounds-checked launch that accumulates into slice 0.
hipError_t launch_dgemm_ksliced(char ta, char tb, long M, long N, long K, double alpha, const double *A, long lda,
                                              const double *B, long ldb, double *C, long ldc, long cslice, int want,
                                              int *nslices, hipStream_t s) {
  const bool tA = (ta == 'T' || ta == 't'), tB = (tb == 'T' || tb == 't');
  long K0, per;
  const int ns = gemm_kslice_plan(K, want, &K0, &per);
  const long K1 = K - K0;
  *nslices = ns;
  if (ns <= 1) return launch_dgemm(ta, tb, M, N, K, alpha, A, lda, B, ldb, 0.0, C, ldc, false, false, s);
  GemmArgs g;
  g.A = A; g.B = B; g.C = C;
  g.M = M; g.N = N; g.K = K0;
  g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.alpha = alpha; g.beta = 0.0;
  g.tiles_m = g.tiles_n = 0;
  g.tm0 = g.tn0 = 0;
  g.syrk_upper = 0; g.clamp = 0; g.square_a = 0; g.ablate = 0; g.gm = 0;
  g.kslices = ns; g.kslice = per; g.cslice = cslice;
  hipError_t e;
  // op(A) = A^T  <=> A stored [k][m]  (KM image);  op(B) = B <=> B stored [k][n] (KN image)
  if (tA && !tB) e = launch_dgemm_t<true, true>(g, s);
  else if (tA && tB) e = launch_dgemm_t<true, false>(g, s);
  else if (!tA && !tB) e = launch_dgemm_t<false, true>(g, s);
  else e = launch_dgemm_t<false, false>(g, s);
  if (e != hipSuccess || K1 == 0) return e;
  const double *A1 = tA ? A + K0 * lda : A + K0, *B1 = tB ? B + K0 : B + K0 * ldb;
  return launch_dgemm(ta, tb, M, N, K1, alpha, A1, lda, B1, ldb, 1.0, C, ldc, false, false, s);
}

} // namespace gemma_hip

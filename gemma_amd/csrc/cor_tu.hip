// Windowed SNP correlation (GEMMA -calccor, a_mode 71) as its own translation unit (see cor_tu.h): the kernels of cor.hip.h, this
// unit's instance of the fp64 MFMA GEMM for the dosage route, and the host side of one block of
//   VARCOV::AnalyzePlink / AnalyzeBimbam   src/varcov.cpp:249-446  (the sliding buffer of centred columns)
//   Calc_Cor                               src/varcov.cpp:220-238  (two ddots of length n per neighbour)
// as a banded Gram matrix: the list of (row tile, column tile) pairs that meet the band, from n_nb[] alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gemma_hip.h"
#include "tu_common.h"
#include "dgemm.h"
#include "cor.hip.h"
#include "cor_tu.h"

namespace gemma_hip {

namespace {

constexpr long COR_PANEL_ROWS = 512; // output SNPs per fp64 band panel: x_{r0 .. r0 + 511} against x_{r0 .. their furthest neighbour}

struct CorState {
  bool active = false, all = true;
  long n = 0, ni_total = 0;
  DevBuf idx;                   // ints
  DevBuf stage;                 // host blocks land here
  DevBuf G, Cm, st;             // hard calls: int8 planes, 3 ints per SNP
  DevBuf X, ss, panel;          // dosages: doubles
  DevBuf nb, off, tiles;        // ints, long longs, 2 ints per tile pair
  DevBuf var, cor;              // the outputs of a host block
  std::vector<int> h_nb, h_tiles; // kept here: asynchronous uploads read them after the call has returned
  std::vector<long long> h_off;
  hipStream_t last = nullptr;
  bool have_last = false;
} g_cor;

void free_block_buffers() {
  g_cor.stage.release();
  g_cor.G.release(); g_cor.Cm.release(); g_cor.st.release();
  g_cor.X.release(); g_cor.ss.release(); g_cor.panel.release();
  g_cor.nb.release(); g_cor.off.release(); g_cor.tiles.release();
  g_cor.var.release(); g_cor.cor.release();
}

struct Want { // what a block needs of one buffer; the buffers grow together, after one wait for the work that may still read them
  DevBuf *b;
  size_t bytes;
};

int grow(std::vector<Want> &w, std::string &msg) {
  bool any = false;
  for (const Want &x : w) any = any || x.bytes > x.b->cap;
  if (!any) return GEMMA_HIP_OK;
  TU_CHK(hipDeviceSynchronize());
  for (const Want &x : w) {
    const int rc = x.b->reserve(x.bytes, "cor", msg);
    if (rc) {
      free_block_buffers();
      return rc;
    }
  }
  return GEMMA_HIP_OK;
}

} // namespace

void cor_release_x() {
  free_block_buffers();
  g_cor.idx.release();
  g_cor.active = false;
  g_cor.have_last = false;
  g_cor.n = g_cor.ni_total = 0;
}

void cor_tu_shutdown() {
  cor_release_x();
}

bool cor_active_x() { return g_cor.active; }
long cor_ni_total_x() { return g_cor.ni_total; }

int cor_begin_x(long ni_total, const int *indicator, std::string &msg) {
  std::vector<int> idx;
  for (long i = 0; i < ni_total; ++i)
    if (!indicator || indicator[i] != 0) idx.push_back((int)i);
  const long n = (long)idx.size();
  if (n < 1) {
    msg = "cor_begin: no analysed individual among " + std::to_string(ni_total);
    return GEMMA_HIP_EINVAL;
  }
  TU_CHK(hipDeviceSynchronize());
  g_cor.active = false;
  int rc;
  if ((rc = g_cor.idx.reserve((size_t)n * sizeof(int), "cor", msg))) return rc;
  TU_CHK(hipMemcpy(g_cor.idx.p, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
  g_cor.n = n;
  g_cor.ni_total = ni_total;
  g_cor.all = (n == ni_total);
  g_cor.have_last = false;
  g_cor.active = true;
  return GEMMA_HIP_OK;
}

int cor_block_x(int geno_kind, const void *geno, long l_in, long ld_src, long l_out, const int *n_nb, double *var, double *cor,
                bool device, hipStream_t s, std::string &msg) {
  const long n = g_cor.n;
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  int rc;
  if (g_cor.have_last) TU_CHK(hipStreamSynchronize(g_cor.last)); // the host lists and the buffers of the previous block are free
  g_cor.have_last = false;
  if (plink && n > COR_I8_NMAX) {
    msg = "cor_block: " + std::to_string(n) + " analysed individuals; the exact integer route takes up to " + std::to_string(COR_I8_NMAX);
    return GEMMA_HIP_EINVAL;
  }
  // the windows, on the host: they decide the shape of everything below
  std::vector<int> &h_nb = g_cor.h_nb;
  h_nb.resize((size_t)l_out);
  if (device) {
    TU_CHK(hipMemcpyAsync(h_nb.data(), n_nb, (size_t)l_out * sizeof(int), hipMemcpyDeviceToHost, s));
    TU_CHK(hipStreamSynchronize(s));
  } else {
    std::memcpy(h_nb.data(), n_nb, (size_t)l_out * sizeof(int));
  }
  std::vector<long long> &h_off = g_cor.h_off;
  h_off.resize((size_t)l_out);
  long long total = 0;
  for (long t = 0; t < l_out; ++t) {
    if (h_nb[t] < 0 || t + (long)h_nb[t] >= l_in) {
      msg = "cor_block: n_nb[" + std::to_string(t) + "] = " + std::to_string(h_nb[t]) + " with l_in = " + std::to_string(l_in) +
            " (the window of an output SNP ends inside the block)";
      return GEMMA_HIP_EINVAL;
    }
    h_off[t] = total;
    total += h_nb[t];
  }
  if (total > 0 && !cor) {
    msg = "cor_block: cor is NULL for " + std::to_string(total) + " correlations";
    return GEMMA_HIP_EINVAL;
  }

  const long tiles_in = (l_in + COR_T - 1) / COR_T, rows_p = tiles_in * COR_T;
  const long ldk = (n + COR_BK - 1) / COR_BK * COR_BK, ldx = (n + 1) & ~1L;
  std::vector<int> &h_tiles = g_cor.h_tiles;
  h_tiles.clear();
  long panel_ld = 2;
  if (plink) {
    for (long ti = 0; ti * COR_T < l_out; ++ti) {
      long reach = -1;
      for (long a = ti * COR_T; a < std::min(l_out, (ti + 1) * COR_T); ++a)
        if (h_nb[a] > 0) reach = std::max(reach, a + h_nb[a]);
      for (long tj = ti; reach >= 0 && tj <= reach / COR_T; ++tj) {
        h_tiles.push_back((int)ti);
        h_tiles.push_back((int)tj);
      }
    }
  } else {
    for (long r0 = 0; r0 < l_out; r0 += COR_PANEL_ROWS) {
      long reach = r0;
      for (long a = r0; a < std::min(l_out, r0 + COR_PANEL_ROWS); ++a) reach = std::max(reach, a + h_nb[a]);
      panel_ld = std::max(panel_ld, (reach - r0 + 2) & ~1L); // reach - r0 + 1 columns, an even leading dimension
    }
  }

  std::vector<Want> w;
  w.push_back({&g_cor.nb, (size_t)l_out * sizeof(int)});
  w.push_back({&g_cor.off, (size_t)l_out * sizeof(long long)});
  const size_t row = plink ? (size_t)((g_cor.ni_total + 3) / 4) : (size_t)g_cor.ni_total * 8;
  if (!device) {
    w.push_back({&g_cor.stage, (size_t)l_in * row});
    w.push_back({&g_cor.var, (size_t)l_out * 8});
    w.push_back({&g_cor.cor, (size_t)total * 8});
  }
  if (plink) {
    w.push_back({&g_cor.G, (size_t)rows_p * ldk});
    w.push_back({&g_cor.Cm, (size_t)rows_p * ldk});
    w.push_back({&g_cor.st, (size_t)rows_p * 3 * sizeof(int)});
    w.push_back({&g_cor.tiles, h_tiles.size() * sizeof(int)});
  } else {
    w.push_back({&g_cor.X, (size_t)l_in * ldx * 8});
    w.push_back({&g_cor.ss, (size_t)l_in * 8});
    w.push_back({&g_cor.panel, (size_t)COR_PANEL_ROWS * panel_ld * 8});
  }
  if ((rc = grow(w, msg))) return rc;

  const void *src = geno;
  const int *nb_d = n_nb;
  double *var_d = var, *cor_d = cor;
  if (!device) {
    const size_t pitch = (size_t)ld_src * (plink ? 1 : 8);
    if ((rc = stage_rows(g_cor.stage, geno, (size_t)l_in, row, pitch, plink ? 1 : 8, s, "cor_block", msg, src, ld_src))) return rc;
    TU_CHK(hipMemcpyAsync(g_cor.nb.p, h_nb.data(), (size_t)l_out * sizeof(int), hipMemcpyHostToDevice, s));
    nb_d = g_cor.nb.as<int>();
    var_d = g_cor.var.as<double>();
    cor_d = g_cor.cor.as<double>();
  }
  g_cor.last = s;
  g_cor.have_last = true;
  TU_CHK(hipMemcpyAsync(g_cor.off.p, h_off.data(), (size_t)l_out * sizeof(long long), hipMemcpyHostToDevice, s));
  const long long *off_d = g_cor.off.as<long long>();
  const int *idx_d = g_cor.all ? nullptr : g_cor.idx.as<int>();

  if (plink) {
    int8_t *G = g_cor.G.as<int8_t>(), *Cm = g_cor.Cm.as<int8_t>();
    int *st = g_cor.st.as<int>();
    if (rows_p > l_in) { // the rows that complete the last tile: genotype 0, not called, N = S = S2 = 0
      TU_CHK(hipMemsetAsync(G + (size_t)l_in * ldk, 0, (size_t)(rows_p - l_in) * ldk, s));
      TU_CHK(hipMemsetAsync(Cm + (size_t)l_in * ldk, 0, (size_t)(rows_p - l_in) * ldk, s));
      TU_CHK(hipMemsetAsync(st + 3 * l_in, 0, (size_t)(rows_p - l_in) * 3 * sizeof(int), s));
    }
    CorIngestI8 a;
    a.src = reinterpret_cast<const unsigned char *>(src);
    a.ld = ld_src;
    a.l = l_in;
    a.l_out = l_out;
    a.idx = idx_d;
    a.n = (int)n;
    a.G = G;
    a.Cm = Cm;
    a.ldk = ldk;
    a.st = st;
    a.var = var_d;
    hipLaunchKernelGGL(cor_ingest_i8_kernel, dim3((unsigned)((l_in + 3) / 4)), dim3(COR_THREADS), 0, s, a);
    TU_CHK(hipGetLastError());
    const long npairs = (long)h_tiles.size() / 2;
    if (npairs > 0) {
      TU_CHK(hipMemcpyAsync(g_cor.tiles.p, h_tiles.data(), h_tiles.size() * sizeof(int), hipMemcpyHostToDevice, s));
      CorBandI8 b;
      b.G = G;
      b.Cm = Cm;
      b.ldk = ldk;
      b.nk = (int)(ldk / COR_BK);
      b.st = st;
      b.tiles = g_cor.tiles.as<int>();
      b.n_nb = nb_d;
      b.off = off_d;
      b.l_out = l_out;
      b.l_in = l_in;
      b.n = (int)n;
      b.cor = cor_d;
      hipLaunchKernelGGL(cor_band_i8_kernel, dim3((unsigned)npairs), dim3(COR_THREADS), 0, s, b);
      TU_CHK(hipGetLastError());
    }
  } else {
    double *X = g_cor.X.as<double>(), *ss = g_cor.ss.as<double>(), *P = g_cor.panel.as<double>();
    CorIngestF64 a;
    a.src = reinterpret_cast<const double *>(src);
    a.ld = ld_src;
    a.l = l_in;
    a.l_out = l_out;
    a.idx = idx_d;
    a.n = (int)n;
    a.X = X;
    a.ldx = ldx;
    a.ss = ss;
    a.var = var_d;
    hipLaunchKernelGGL(cor_ingest_f64_kernel, dim3((unsigned)l_in), dim3(COR_THREADS), 0, s, a);
    TU_CHK(hipGetLastError());
    for (long r0 = 0; r0 < l_out; r0 += COR_PANEL_ROWS) {
      const long rows = std::min(COR_PANEL_ROWS, l_out - r0);
      long reach = -1;
      for (long t = r0; t < r0 + rows; ++t)
        if (h_nb[t] > 0) reach = std::max(reach, t + h_nb[t]);
      if (reach < 0) continue; // no window in these rows
      const long cols = reach - r0 + 1;
      // P = X_{r0 ..} X_{r0 .. reach}^T: K contiguous on both sides
      TU_CHK(launch_dgemm('N', 'T', rows, cols, n, 1.0, X + (size_t)r0 * ldx, ldx, X + (size_t)r0 * ldx, ldx, 0.0, P, panel_ld, false,
                          false, s));
      hipLaunchKernelGGL(cor_scatter_kernel, dim3((unsigned)rows), dim3(COR_THREADS), 0, s, P, panel_ld, r0, ss, nb_d, off_d, cor_d);
      TU_CHK(hipGetLastError());
    }
  }
  if (!device) {
    TU_CHK(hipMemcpyAsync(var, var_d, (size_t)l_out * 8, hipMemcpyDeviceToHost, s));
    if (total > 0) TU_CHK(hipMemcpyAsync(cor, cor_d, (size_t)total * 8, hipMemcpyDeviceToHost, s));
    TU_CHK(hipStreamSynchronize(s));
  }
  return GEMMA_HIP_OK;
}

} // namespace gemma_hip

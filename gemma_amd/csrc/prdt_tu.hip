// Genomic prediction (GEMMA -bslmm 2 and -predict 1 / 2) as its own translation unit (see prdt_tu.h): the two genotype
// matrix-vector passes (geno_mv.hip.h), their state, and the small dense algebra of
//   BSLMM::RidgeR   src/bslmm.cpp:1194-1221
//   PRDT::AddBV     src/prdt.cpp:133-205 with the weighted CenterMatrix(G, w), src/mathfunc.cpp:181-201
//   the tail of the -predict block, src/gemma.cpp:1711-1722
// on the fp64 MFMA GEMM and the eigensolver.
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
#include "eigh_tu.h"
#include "geno_mv.hip.h"
#include "spd_inv.hip.h"
#include "prdt_mv.hip.h"
#include "prdt_tu.h"

namespace gemma_hip {

namespace {

// the groups of individuals of a block's rows, on the device in both forms the kernels read
struct Groups {
  long ni_total = 0, words = 0, n_a = 0, n_b = 0;
  std::vector<int> pos_a, pos_b; // positions of the A / B individuals in ni_total
  DevBuf amask, bmask, grp, posb;
  int set(const int *ind, long ni, std::string &msg) { // ind == nullptr: everybody is in A
    ni_total = ni;
    words = (ni + 15) / 16;
    std::vector<unsigned> am(words, 0u), bm(words, 0u);
    std::vector<unsigned char> g(ni);
    pos_a.clear();
    pos_b.clear();
    for (long i = 0; i < ni; ++i) {
      const bool a = !ind || ind[i] != 0;
      (a ? am : bm)[i / 16] |= 1u << (2 * (i % 16));
      g[i] = a ? 1 : 2;
      (a ? pos_a : pos_b).push_back((int)i);
    }
    n_a = (long)pos_a.size();
    n_b = (long)pos_b.size();
    int rc;
    if ((rc = amask.reserve(words * 4, "prdt", msg)) || (rc = bmask.reserve(words * 4, "prdt", msg)) || (rc = grp.reserve(ni, "prdt", msg)) ||
        (rc = posb.reserve(std::max<long>(n_b, 1) * 4, "prdt", msg)))
      return rc;
    TU_CHK(hipMemcpy(amask.p, am.data(), words * 4, hipMemcpyHostToDevice));
    TU_CHK(hipMemcpy(bmask.p, bm.data(), words * 4, hipMemcpyHostToDevice));
    TU_CHK(hipMemcpy(grp.p, g.data(), ni, hipMemcpyHostToDevice));
    if (n_b) TU_CHK(hipMemcpy(posb.p, pos_b.data(), n_b * 4, hipMemcpyHostToDevice));
    return GEMMA_HIP_OK;
  }
  MvGroups dev() {
    MvGroups m;
    m.amask = amask.as<unsigned>();
    m.bmask = bmask.as<unsigned>();
    m.grp = grp.as<unsigned char>();
    m.ni_total = ni_total;
    m.words = words;
    return m;
  }
  void release() {
    amask.release(); bmask.release(); grp.release(); posb.release();
    pos_a.clear(); pos_b.clear();
    ni_total = words = n_a = n_b = 0;
  }
};

struct RidgeState {
  bool ready = false, have_groups = false;
  long n = 0;
  double scale = 1.0;
  std::vector<double> r; // host copy: scattered again when the indicator changes
  Groups grp;
  DevBuf r_full, work, stage_in, stage_out, dense;
} g_rg;

struct PrdtState {
  bool active = false;
  hipStream_t last = nullptr; // the stream of the last prdt_add
  Groups grp;
  DevBuf y, work, stage_in, stage_w, used, dense;
} g_pd;


// r_full of the current groups (zeros at the other individuals and in the padding)
int ridge_scatter(std::string &msg) {
  const long len = mv_rfull_len(g_rg.grp.ni_total);
  std::vector<double> full(len, 0.0);
  for (long j = 0; j < g_rg.n; ++j) full[g_rg.grp.pos_a[j]] = g_rg.r[j];
  int rc = g_rg.r_full.reserve(len * 8, "prdt", msg);
  if (rc) return rc;
  TU_CHK(hipMemcpy(g_rg.r_full.p, full.data(), len * 8, hipMemcpyHostToDevice));
  return GEMMA_HIP_OK;
}

int ridge_install(long n, double scale, std::string &msg) { // g_rg.r is set: everybody analysed until set_indicator says otherwise
  g_rg.n = n;
  g_rg.scale = scale;
  int rc = g_rg.grp.set(nullptr, n, msg);
  if (rc) return rc;
  g_rg.have_groups = true;
  if ((rc = ridge_scatter(msg))) return rc;
  g_rg.ready = true;
  return GEMMA_HIP_OK;
}

// B[i] = {b_i, (lambda eval_i) b_i} with b = Uty / (lambda eval + 1), the two right-hand sides of RidgeR
__global__ void ridge_rhs_kernel(const double *eval, const double *Uty, long n, double lambda, double *B) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double h = lambda * eval[i] + 1.0;
  const double b = Uty[i] / h;
  B[2 * i] = b;
  B[2 * i + 1] = (h - 1.0) * b;
}

// Goo / Gfo of AddBV from G centred with the 0 / 1 weights of the training individuals (CenterMatrix(G, w): G - (Gw w' + w Gw') /
// w'w + (w'Gw) / (w'w)^2 w w' on the upper triangle, mirrored).  gw[i] = row i of G summed over the training columns.
__global__ __launch_bounds__(256) void bv_rowsum_kernel(const double *G, long ldg, long ni, const int *pos_a, long n_a, double *gw) {
  const int lane = threadIdx.x & 63;
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= ni) return;
  double a = 0.0;
  for (long j = lane; j < n_a; j += 64) a += G[i * ldg + pos_a[j]];
  a = wave_sum(a);
  if (lane == 0) gw[i] = a;
}

__global__ __launch_bounds__(256) void bv_wgw_kernel(const double *gw, const int *pos_a, long n_a, double *d) { // one workgroup
  __shared__ double red[4];
  double a = 0.0;
  for (long j = threadIdx.x; j < n_a; j += 256) a += gw[pos_a[j]];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) *d = ((red[0] + red[1]) + red[2]) + red[3];
}

// out (rows x n_a, ldo): row k = individual rowpos[k]; train_rows: the rows are training individuals (Goo) or not (Gfo)
__global__ __launch_bounds__(256) void bv_gather_kernel(const double *G, long ldg, const int *rowpos, long rows, bool train_rows,
                                                        const int *pos_a, long n_a, const double *gw, const double *d, double *out,
                                                        long ldo) {
  const long j = (long)blockIdx.x * 256 + threadIdx.x;
  const long k = blockIdx.y;
  if (j >= n_a || k >= rows) return;
  const long i = rowpos[k], c = pos_a[j];
  const double wtw = (double)n_a;
  const double g = i <= c ? G[i * ldg + c] : G[c * ldg + i]; // the reference updates the upper triangle and mirrors it
  const double v = train_rows ? g - (gw[i] + gw[c]) / wtw + *d / (wtw * wtw) : g - gw[i] / wtw;
  out[k * ldo + j] = v;
}

// Utu_i /= eval_i where eval_i >= 1e-10 (smaller eigenvalues are zeroed and their component is kept as it is: src/prdt.cpp:176-191)
__global__ void bv_pinv_kernel(const double *eval, long n, double *utu) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double e = eval[i] < 1e-10 ? 0.0 : eval[i];
  if (e != 0.0) utu[i] = utu[i] / e;
}

__global__ void prdt_tail_kernel(double *y, long n, double mean, int probit) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double v = y[i] + mean;
  if (probit) v = 0.5 * erfc(-v * 0.70710678118654752440); // gsl_cdf_gaussian_P(v, 1)
  y[i] = v;
}

unsigned nb(long n) { return (unsigned)((n + 255) / 256); }

} // namespace

// ------------------------------------------------------------------------------------------------ ridge
bool ridge_ready_x() { return g_rg.ready; }
size_t ridge_n_x() { return (size_t)g_rg.n; }
size_t ridge_ni_total_x() { return (size_t)g_rg.grp.ni_total; }

void ridge_finish_x() {
  g_rg.ready = g_rg.have_groups = false;
  g_rg.grp.release();
  g_rg.r.clear();
  g_rg.r_full.release(); g_rg.work.release(); g_rg.stage_in.release(); g_rg.stage_out.release(); g_rg.dense.release();
}

int ridge_set_r_x(long n, const double *r, double scale, std::string &msg) {
  g_rg.ready = false;
  g_rg.r.assign(r, r + n);
  return ridge_install(n, scale, msg);
}

int ridge_setup_x(long n, const double *U, long ldu, const double *eval, bool ue_device, const double *Uty, bool uty_device, double lambda,
                  long ns_test, double *bv_out, hipStream_t s, std::string &msg) {
  g_rg.ready = false;
  // dense: [U copy n x ldc | eval n | Uty n | B n x 2 | C n x 2]
  const long ldc = ue_device ? 0 : ((n + 1) & ~1L);
  int rc = g_rg.dense.reserve((size_t)(n * ldc + 6 * n) * 8, "prdt", msg);
  if (rc) return rc;
  double *base = g_rg.dense.as<double>();
  double *Uc = base, *ev = base + n * ldc, *uy = ev + n, *B = uy + n, *Cm = B + 2 * n;
  const double *Ud = U, *evd = eval, *uyd = Uty;
  long ld = ldu;
  if (!ue_device) {
    TU_CHK(hipMemcpy2DAsync(Uc, ldc * 8, U, ldu * 8, n * 8, n, hipMemcpyHostToDevice, s));
    TU_CHK(hipMemcpyAsync(ev, eval, n * 8, hipMemcpyHostToDevice, s));
    Ud = Uc; evd = ev; ld = ldc;
  }
  if (!uty_device) {
    TU_CHK(hipMemcpyAsync(uy, Uty, n * 8, hipMemcpyHostToDevice, s));
    uyd = uy;
  }
  ridge_rhs_kernel<<<nb(n), 256, 0, s>>>(evd, uyd, n, lambda, B);
  TU_CHK(hipGetLastError());
  TU_CHK(launch_dgemm('N', 'N', n, 2, n, 1.0, Ud, ld, B, 2, 0.0, Cm, 2, false, false, s));
  std::vector<double> c2(2 * n);
  TU_CHK(hipMemcpyAsync(c2.data(), Cm, 2 * n * 8, hipMemcpyDeviceToHost, s));
  TU_CHK(hipStreamSynchronize(s));
  g_rg.r.resize(n);
  for (long i = 0; i < n; ++i) g_rg.r[i] = c2[2 * i];
  if (bv_out) {
    std::vector<double> bv(n);
    for (long i = 0; i < n; ++i) bv[i] = c2[2 * i + 1];
    if (uty_device) TU_CHK(hipMemcpy(bv_out, bv.data(), n * 8, hipMemcpyHostToDevice));
    else memcpy(bv_out, bv.data(), n * 8);
  }
  return ridge_install(n, lambda / (double)ns_test, msg);
}

int ridge_set_indicator_x(const int *indicator_idv, long ni_total, std::string &msg) {
  long n_a = 0; // counted before anything changes: a refused indicator leaves the groups and r_full as they were
  for (long i = 0; i < ni_total; ++i) n_a += indicator_idv[i] != 0;
  if (n_a != g_rg.n) {
    msg = "ridge_set_indicator: " + std::to_string(n_a) + " analysed individuals, n = " + std::to_string(g_rg.n);
    return GEMMA_HIP_EINVAL;
  }
  int rc = g_rg.grp.set(indicator_idv, ni_total, msg);
  if (rc == GEMMA_HIP_OK) rc = ridge_scatter(msg);
  if (rc) g_rg.ready = false; // groups and r_full may disagree now: the fit has to be set up again
  return rc;
}

// rows of one launch: the 2-bit product puts ceil(l / MV_ROWS) into the grid's y dimension (at most 65535)
constexpr long MV_MAX_ROWS = 65535L * MV_ROWS;

int ridge_batch_x(int geno_kind, const void *geno, long l, long ld, bool device, double *alpha_out, hipStream_t s, std::string &msg) {
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  const size_t esz = plink ? 1 : 8;
  const long row = plink ? (g_rg.grp.ni_total + 3) / 4 : g_rg.grp.ni_total; // elements of a row that are read
  for (long s0 = 0; s0 < l; s0 += MV_MAX_ROWS) {
    const long m = std::min(MV_MAX_ROWS, l - s0);
    int rc = g_rg.work.reserve((size_t)mv_xtr_work(g_rg.grp.ni_total, m) * 8, "prdt", msg);
    if (rc) return rc;
    const void *gd = static_cast<const char *>(geno) + (size_t)s0 * ld * esz;
    double *ad = alpha_out + s0;
    long ldd = ld;
    if (!device) { // only the `row` leading elements of each host row are touched: the caller's last row may end there
      if ((rc = g_rg.stage_out.reserve((size_t)m * 8, "prdt", msg)) ||
          (rc = stage_rows(g_rg.stage_in, gd, m, row * esz, ld * esz, esz, s, "prdt", msg, gd, ldd)))
        return rc;
      ad = g_rg.stage_out.as<double>();
    }
    TU_CHK(launch_xtr(plink, gd, m, ldd, g_rg.grp.dev(), g_rg.r_full.as<double>(), g_rg.scale, ad, g_rg.work.as<double>(), s));
    if (!device) {
      TU_CHK(hipMemcpyAsync(alpha_out + s0, ad, (size_t)m * 8, hipMemcpyDeviceToHost, s));
      TU_CHK(hipStreamSynchronize(s));
    }
  }
  return GEMMA_HIP_OK;
}

// ------------------------------------------------------------------------------------------------ prediction
bool prdt_active_x() { return g_pd.active; }
size_t prdt_ni_total_x() { return (size_t)g_pd.grp.ni_total; }
size_t prdt_n_train_x() { return (size_t)g_pd.grp.n_a; }

static void prdt_release() {
  g_pd.active = false;
  g_pd.grp.release();
  g_pd.y.release(); g_pd.work.release(); g_pd.stage_in.release(); g_pd.stage_w.release(); g_pd.used.release(); g_pd.dense.release();
}

int prdt_begin_x(const int *indicator_idv, long ni_total, std::string &msg) {
  g_pd.active = false;
  g_pd.last = nullptr;
  int rc = g_pd.grp.set(indicator_idv, ni_total, msg);
  if (rc) return rc;
  if ((rc = g_pd.y.reserve(std::max<long>(g_pd.grp.n_b, 1) * 8, "prdt", msg))) return rc;
  TU_CHK(hipMemset(g_pd.y.p, 0, std::max<long>(g_pd.grp.n_b, 1) * 8));
  g_pd.active = true;
  return GEMMA_HIP_OK;
}

int prdt_add_x(int geno_kind, const void *geno, long l, long ld, bool device, const double *effect, int *used_out, hipStream_t s,
               std::string &msg) {
  const bool plink = geno_kind == GEMMA_GENO_PLINK_2BIT;
  const size_t esz = plink ? 1 : 8;
  int rc = g_pd.work.reserve((size_t)mv_xw_work(g_pd.grp.ni_total, l) * 8, "prdt", msg);
  if (rc) return rc;
  const void *gd = geno;
  const double *wd = effect;
  int *ud = used_out;
  long ldd = ld;
  if (!device) { // only the leading elements of each host row that are read are copied
    const long row = plink ? (g_pd.grp.ni_total + 3) / 4 : g_pd.grp.ni_total;
    if ((rc = g_pd.stage_w.reserve((size_t)l * 8, "prdt", msg)) ||
        (rc = stage_rows(g_pd.stage_in, geno, l, row * esz, ld * esz, esz, s, "prdt", msg, gd, ldd)))
      return rc;
    TU_CHK(hipMemcpyAsync(g_pd.stage_w.p, effect, (size_t)l * 8, hipMemcpyHostToDevice, s));
    wd = g_pd.stage_w.as<double>();
  }
  if (!device || !used_out) {
    if ((rc = g_pd.used.reserve((size_t)l * 4, "prdt", msg))) return rc;
    ud = g_pd.used.as<int>();
  }
  g_pd.last = s; // prdt_end waits for it: the device form is asynchronous on the caller's stream
  TU_CHK(launch_xw(plink, gd, l, ldd, g_pd.grp.dev(), wd, g_pd.grp.posb.as<int>(), g_pd.grp.n_b, g_pd.y.as<double>(), ud,
                  g_pd.work.as<double>(), s));
  if (!device) {
    if (used_out) TU_CHK(hipMemcpyAsync(used_out, ud, (size_t)l * 4, hipMemcpyDeviceToHost, s));
    TU_CHK(hipStreamSynchronize(s));
  }
  return GEMMA_HIP_OK;
}

int prdt_add_bv_x(const double *G, long ni_total, long ldg, bool device, const double *u_hat, hipStream_t s, std::string &msg) {
  Groups &gr = g_pd.grp;
  const long no = gr.n_a, nf = gr.n_b;
  if (no == 0 || nf == 0) return GEMMA_HIP_OK; // nothing to predict from or for
  const long ldo = (no + 1) & ~1L;
  // dense: [G copy | gw ni | d 2 | pos_a (ints) no | Goo no x no | Gfo nf x ldo | U no x no | eval no | u no | utu no | v no]
  const long gcopy = device ? 0 : ni_total * ni_total;
  const long posd = (no + 1) / 2 + 1;
  const size_t doubles = (size_t)gcopy + ni_total + 2 + posd + (size_t)(2 * no + nf) * ldo + 4 * no;
  int rc = g_pd.dense.reserve(doubles * 8, "prdt", msg);
  if (rc) return rc;
  double *p = g_pd.dense.as<double>();
  double *Gc = p; p += gcopy;
  double *gw = p; p += ni_total;
  double *d = p; p += 2;
  int *pos_a = reinterpret_cast<int *>(p); p += posd;
  double *Goo = p; p += no * ldo;
  double *Gfo = p; p += nf * ldo;
  double *U = p; p += no * ldo;
  double *ev = p; p += no;
  double *u = p; p += no;
  double *utu = p; p += no;
  double *v = p;
  const double *Gd = G;
  long ld = ldg;
  if (!device) {
    TU_CHK(hipMemcpy2DAsync(Gc, ni_total * 8, G, ldg * 8, ni_total * 8, ni_total, hipMemcpyHostToDevice, s));
    Gd = Gc;
    ld = ni_total;
  }
  TU_CHK(hipMemcpyAsync(pos_a, gr.pos_a.data(), no * 4, hipMemcpyHostToDevice, s));
  TU_CHK(hipMemcpyAsync(u, u_hat, no * 8, hipMemcpyHostToDevice, s));
  bv_rowsum_kernel<<<(unsigned)((ni_total + 3) / 4), 256, 0, s>>>(Gd, ld, ni_total, pos_a, no, gw);
  bv_wgw_kernel<<<1, 256, 0, s>>>(gw, pos_a, no, d);
  bv_gather_kernel<<<dim3(nb(no), (unsigned)no), 256, 0, s>>>(Gd, ld, pos_a, no, true, pos_a, no, gw, d, Goo, no); // dense: the solver's form
  bv_gather_kernel<<<dim3(nb(no), (unsigned)nf), 256, 0, s>>>(Gd, ld, gr.posb.as<int>(), nf, false, pos_a, no, gw, d, Gfo, ldo);
  TU_CHK(hipGetLastError());
  rc = eigh_device_x(Goo, no, U, ev, s, msg);
  if (rc) return rc;
  // Utu = U' u; Utu /= eval (pseudo-inverse); v = U Utu; y += Gfo v
  TU_CHK(launch_dgemm('T', 'N', no, 1, no, 1.0, U, no, u, 1, 0.0, utu, 1, false, false, s));
  bv_pinv_kernel<<<nb(no), 256, 0, s>>>(ev, no, utu);
  TU_CHK(hipGetLastError());
  TU_CHK(launch_dgemm('N', 'N', no, 1, no, 1.0, U, no, utu, 1, 0.0, v, 1, false, false, s));
  TU_CHK(launch_dgemm('N', 'N', nf, 1, no, 1.0, Gfo, ldo, v, 1, 1.0, g_pd.y.as<double>(), 1, false, false, s));
  TU_CHK(hipStreamSynchronize(s));
  return GEMMA_HIP_OK;
}

int prdt_end_x(double pheno_mean, int probit, double *y_prdt, std::string &msg) {
  const long nf = g_pd.grp.n_b;
  TU_CHK(hipStreamSynchronize(g_pd.last)); // the adds of the device form may still be running on the caller's stream
  g_pd.last = nullptr;
  if (nf > 0) {
    prdt_tail_kernel<<<nb(nf), 256, 0, nullptr>>>(g_pd.y.as<double>(), nf, pheno_mean, probit);
    TU_CHK(hipGetLastError());
    TU_CHK(hipMemcpy(y_prdt, g_pd.y.p, nf * 8, hipMemcpyDeviceToHost));
  }
  prdt_release();
  return GEMMA_HIP_OK;
}

// ------------------------------------------------------------------------------------------------ kinship-only, several phenotypes
namespace {

struct PrdtMvState {
  DevBuf G, H, small; // the centred kinship (ni x ni), H_oo (N x lda), the index lists and the short vectors
  SpdFactorWork spd;
} g_mv;

// the lists of an ni x d indicator, entries in i * d + a order
struct MvLists {
  std::vector<int> oi, oa, ou, ui, mi, ma;
  void set(const int *ind, long ni, long d) {
    for (long i = 0; i < ni; ++i) {
      bool any = false;
      for (long a = 0; a < d; ++a) {
        if (ind[i * d + a] != 0) {
          if (!any) ui.push_back((int)i);
          any = true;
          oi.push_back((int)i);
          oa.push_back((int)a);
          ou.push_back((int)ui.size() - 1);
        } else {
          mi.push_back((int)i);
          ma.push_back((int)a);
        }
      }
    }
  }
};

PmvSmall mv_small(long d, long c, const double *Vg, const double *Ve, const double *B) {
  PmvSmall sm;
  memset(&sm, 0, sizeof sm);
  sm.d = (int)d;
  sm.c = (int)c;
  memcpy(sm.Vg, Vg, d * d * 8);
  memcpy(sm.Ve, Ve, d * d * 8);
  if (B) memcpy(sm.B, B, d * c * 8);
  return sm;
}

int mv_upload_lists(const MvLists &l, int *&oi, int *&oa, int *&ou, int *&ui, int *&mi, int *&ma, char *&next, hipStream_t s,
                    std::string &msg) { // into g_mv.small, already reserved; next: the first 16-byte aligned byte behind them
  const std::vector<int> *v[6] = {&l.oi, &l.oa, &l.ou, &l.ui, &l.mi, &l.ma};
  int **dst[6] = {&oi, &oa, &ou, &ui, &mi, &ma};
  char *p = g_mv.small.as<char>();
  for (int k = 0; k < 6; ++k) {
    *dst[k] = reinterpret_cast<int *>(p);
    if (!v[k]->empty()) TU_CHK(hipMemcpyAsync(p, v[k]->data(), v[k]->size() * 4, hipMemcpyHostToDevice, s));
    p += (v[k]->size() * 4 + 15) & ~(size_t)15;
  }
  next = p;
  return GEMMA_HIP_OK;
}

size_t mv_lists_bytes(const MvLists &l) {
  size_t b = 0;
  for (const std::vector<int> *v : {&l.oi, &l.oa, &l.ou, &l.ui, &l.mi, &l.ma}) b += (v->size() * 4 + 15) & ~(size_t)15;
  return b;
}

void mv_launch_assemble(const double *Gc, long ldg, const int *ou, const int *oa, const int *ui, long N, const PmvSmall &sm, double *H,
                        long lda, hipStream_t s) {
  const unsigned t = (unsigned)((N + PMV_TILE - 1) / PMV_TILE);
  prdt_mv_assemble_kernel<<<dim3(t, t), 256, 0, s>>>(Gc, ldg, ou, oa, ui, N, sm, H, lda);
}

} // namespace

void prdt_mv_release_x() {
  g_mv.G.release(); g_mv.H.release(); g_mv.small.release();
  g_mv.spd.release();
}

int prdt_mv_stage_G_x(const double *G, long ni, long ldg, bool device, double **Gd, hipStream_t s, std::string &msg) {
  int rc = g_mv.G.reserve((size_t)ni * ni * 8, "prdt_kin_mv", msg);
  if (rc) return rc;
  TU_CHK(hipMemcpy2DAsync(g_mv.G.p, ni * 8, G, ldg * 8, ni * 8, ni, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  *Gd = g_mv.G.as<double>();
  return GEMMA_HIP_OK;
}

int prdt_mv_sub_x(const double *Gd, long ldg, const int *pos, long n, double *out_d, hipStream_t s, std::string &msg) {
  int rc = g_mv.small.reserve((size_t)n * 4, "prdt_kin_mv", msg);
  if (rc) return rc;
  TU_CHK(hipMemcpyAsync(g_mv.small.p, pos, n * 4, hipMemcpyHostToDevice, s));
  prdt_mv_sub_kernel<<<dim3(nb(n), (unsigned)n), 256, 0, s>>>(Gd, ldg, g_mv.small.as<int>(), n, out_d);
  TU_CHK(hipGetLastError());
  TU_CHK(hipStreamSynchronize(s)); // pos and the list buffer may change after the return
  return GEMMA_HIP_OK;
}

int prdt_mv_apply_x(long ni, long d, const double *G, long ldg, int g_where, const int *ind, const double *W, long c, const double *Y,
                    const double *Vg, const double *Ve, const double *B, double *y_miss, long *bad_pivot, hipStream_t s, std::string &msg) {
  MvLists l;
  l.set(ind, ni, d);
  const long N = (long)l.oi.size(), M = (long)l.mi.size();
  if (M == 0) return GEMMA_HIP_OK;
  int rc;
  double *Gc = g_mv.G.as<double>();
  if (g_where != 2 && (rc = prdt_mv_stage_G_x(G, ni, ldg, g_where == 1, &Gc, s, msg))) return rc;
  if ((rc = gemma_hip_center_d(Gc, (size_t)ni, s))) {
    msg = gemma_hip_last_error();
    return rc;
  }
  const long lda = (N + 1) & ~1L;
  // small: [lists | W ni x c | Y ni x d | x N | Z ni x d | GZ ni x d | y_miss M]
  const size_t doubles = (size_t)ni * (c + 3 * d) + N + M;
  if ((rc = g_mv.small.reserve(mv_lists_bytes(l) + doubles * 8, "prdt_kin_mv", msg)) ||
      (rc = g_mv.H.reserve((size_t)std::max<long>(N, 1) * lda * 8, "prdt_kin_mv", msg)))
    return rc;
  int *oi, *oa, *ou, *ui, *mi, *ma;
  char *next;
  if ((rc = mv_upload_lists(l, oi, oa, ou, ui, mi, ma, next, s, msg))) return rc;
  double *p = reinterpret_cast<double *>(next);
  double *Wd = p; p += ni * c;
  double *Yd = p; p += ni * d;
  double *x = p; p += N;
  double *Z = p; p += ni * d;
  double *GZ = p; p += ni * d;
  double *ym = p;
  TU_CHK(hipMemcpyAsync(Wd, W, ni * c * 8, hipMemcpyHostToDevice, s));
  TU_CHK(hipMemcpyAsync(Yd, Y, ni * d * 8, hipMemcpyHostToDevice, s));
  TU_CHK(hipMemsetAsync(Z, 0, ni * d * 8, s));
  const PmvSmall sm = mv_small(d, c, Vg, Ve, B);
  if (N > 0) {
    double *H = g_mv.H.as<double>();
    TU_CHK(hipMemsetAsync(H, 0, (size_t)N * lda * 8, s)); // what lies below the diagonal is scratch of the factor's diagonal tiles
    mv_launch_assemble(Gc, ni, ou, oa, ui, N, sm, H, lda, s);
    prdt_mv_resid_kernel<<<nb(N), 256, 0, s>>>(Yd, Wd, oi, oa, N, sm, x);
    TU_CHK(hipGetLastError());
    if ((rc = spd_factor_solve_device(H, N, lda, x, nullptr, bad_pivot, g_mv.spd, "prdt_kin_mv: H_oo", s, msg))) return rc;
    prdt_mv_scatter_kernel<<<nb(N), 256, 0, s>>>(x, oi, oa, N, (int)d, Z);
    TU_CHK(hipGetLastError());
  }
  TU_CHK(launch_dgemm('N', 'N', ni, d, ni, 1.0, Gc, ni, Z, d, 0.0, GZ, d, false, false, s));
  prdt_mv_epilogue_kernel<<<nb(M), 256, 0, s>>>(GZ, Z, Wd, mi, ma, M, sm, ym);
  TU_CHK(hipGetLastError());
  TU_CHK(hipMemcpyAsync(y_miss, ym, M * 8, hipMemcpyDeviceToHost, s));
  TU_CHK(hipStreamSynchronize(s));
  return GEMMA_HIP_OK;
}

// tests: the upper triangle of H_oo alone, written into the caller's N x lda host array (everything else of it is left as it was)
int prdt_mv_dbg_assemble_x(long ni, long d, const double *Gc_host, const int *ind, const double *Vg, const double *Ve, double *H_host,
                           long lda, hipStream_t s, std::string &msg) {
  MvLists l;
  l.set(ind, ni, d);
  const long N = (long)l.oi.size();
  if (N == 0) return GEMMA_HIP_OK;
  int rc;
  double *Gc;
  if ((rc = prdt_mv_stage_G_x(Gc_host, ni, ni, false, &Gc, s, msg)) ||
      (rc = g_mv.small.reserve(mv_lists_bytes(l), "prdt_kin_mv", msg)) || (rc = g_mv.H.reserve((size_t)N * lda * 8, "prdt_kin_mv", msg)))
    return rc;
  int *oi, *oa, *ou, *ui, *mi, *ma;
  char *next;
  if ((rc = mv_upload_lists(l, oi, oa, ou, ui, mi, ma, next, s, msg))) return rc;
  TU_CHK(hipMemcpyAsync(g_mv.H.p, H_host, (size_t)N * lda * 8, hipMemcpyHostToDevice, s));
  mv_launch_assemble(Gc, ni, ou, oa, ui, N, mv_small(d, 0, Vg, Ve, nullptr), g_mv.H.as<double>(), lda, s);
  TU_CHK(hipGetLastError());
  TU_CHK(hipMemcpyAsync(H_host, g_mv.H.p, (size_t)N * lda * 8, hipMemcpyDeviceToHost, s));
  TU_CHK(hipStreamSynchronize(s));
  return GEMMA_HIP_OK;
}

// tests and the probe: A x = r by the factor + solve path.  Device form: A (n x n, lda; upper triangle read, the factor left in
// place) and x (r in, the solution out) on the device; host form: both on the host, A dense and not changed.
int prdt_mv_dbg_solve_x(double *A, long n, long lda, double *x, bool device, long *bad_pivot, hipStream_t s, std::string &msg) {
  if (device) return spd_factor_solve_device(A, n, lda, x, nullptr, bad_pivot, g_mv.spd, "spd_solve", s, msg);
  const long ld = (n + 1) & ~1L;
  int rc;
  if ((rc = g_mv.H.reserve((size_t)n * ld * 8, "prdt_kin_mv", msg)) || (rc = g_mv.small.reserve((size_t)n * 8, "prdt_kin_mv", msg))) return rc;
  TU_CHK(hipMemcpy2DAsync(g_mv.H.p, ld * 8, A, lda * 8, n * 8, n, hipMemcpyHostToDevice, s));
  TU_CHK(hipMemcpyAsync(g_mv.small.p, x, n * 8, hipMemcpyHostToDevice, s));
  if ((rc = spd_factor_solve_device(g_mv.H.as<double>(), n, ld, g_mv.small.as<double>(), nullptr, bad_pivot, g_mv.spd, "spd_solve", s, msg)))
    return rc;
  TU_CHK(hipMemcpy(x, g_mv.small.p, n * 8, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

void prdt_tu_shutdown() {
  ridge_finish_x();
  prdt_release();
  prdt_mv_release_x();
}

} // namespace gemma_hip

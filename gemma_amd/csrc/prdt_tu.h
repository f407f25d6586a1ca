// Entry points of the genomic-prediction translation unit (prdt_tu.hip = geno_mv.hip.h + the small dense pieces on its own
// instance of the fp64 MFMA GEMM and the eigensolver's entry point).  Separate object file, as the eigensolver's (eigh_tu.h) and the
// variance-component unit's (vc_tu.h): C++ linkage, hidden behind the C ABI (abi_prdt.inc.h).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>

namespace gemma_hip {

// ridge / BLUP (-bslmm 2, BSLMM::RidgeR): r = U (Uty / (lambda eval + 1)) on the device, bv = U (lambda eval o b).
// U (n x n, ldu), eval: device pointers when ue_device; Uty: device pointer when uty_device; bv_out: like Uty.
int ridge_setup_x(long n, const double *U, long ldu, const double *eval, bool ue_device, const double *Uty, bool uty_device, double lambda,
                  long ns_test, double *bv_out, hipStream_t s, std::string &msg);
// the vector of the product set directly (host r[n]; alpha = scale * X_c^T r): what the kernel tests and the probe drive
int ridge_set_r_x(long n, const double *r, double scale, std::string &msg);
int ridge_set_indicator_x(const int *indicator_idv, long ni_total, std::string &msg);
int ridge_batch_x(int geno_kind, const void *geno, long l, long ld, bool device, double *alpha_out, hipStream_t s, std::string &msg);
void ridge_finish_x();
bool ridge_ready_x();
size_t ridge_n_x();        // analysed individuals (length of r)
size_t ridge_ni_total_x(); // individuals per row of a block

int prdt_begin_x(const int *indicator_idv, long ni_total, std::string &msg);
int prdt_add_x(int geno_kind, const void *geno, long l, long ld, bool device, const double *effect, int *used_out, hipStream_t s,
               std::string &msg);
// PRDT::AddBV: G (ni_total x ni_total, ldg; host or device, not changed), u_hat[number of training individuals] (host)
int prdt_add_bv_x(const double *G, long ni_total, long ldg, bool device, const double *u_hat, hipStream_t s, std::string &msg);
int prdt_end_x(double pheno_mean, int probit, double *y_prdt, std::string &msg);
bool prdt_active_x();
size_t prdt_ni_total_x();
size_t prdt_n_train_x();

// Kinship-only prediction for several phenotypes (prdt_mv.hip.h).  prdt_mv_apply_x: the Kronecker system alone, ind (ni x d, host),
// W (ni x c), Y (ni x d), Vg / Ve (d x d), B (d x c), y_miss on the host.  g_where: 0 = G (ni x ni, ldg) on the host, 1 = on the
// device (copied, not changed), 2 = already staged by prdt_mv_stage_G_x (centred in place).  *bad_pivot with GEMMA_HIP_ENOTPD.
int prdt_mv_apply_x(long ni, long d, const double *G, long ldg, int g_where, const int *ind, const double *W, long c, const double *Y,
                    const double *Vg, const double *Ve, const double *B, double *y_miss, long *bad_pivot, hipStream_t s, std::string &msg);
// G (host or device) into the unit's own ni x ni buffer: *Gd
int prdt_mv_stage_G_x(const double *G, long ni, long ldg, bool device, double **Gd, hipStream_t s, std::string &msg);
// out_d (n x n, device) = Gd[pos][pos], pos[n] on the host
int prdt_mv_sub_x(const double *Gd, long ldg, const int *pos, long n, double *out_d, hipStream_t s, std::string &msg);
void prdt_mv_release_x();
// tests: the assembled upper triangle of H_oo from a centred Gc (all on the host; H_host N x lda is read, overwritten on its upper
// triangle and returned), and the factor + solve path on a host matrix (not changed) or on a device matrix (factored in place)
int prdt_mv_dbg_assemble_x(long ni, long d, const double *Gc_host, const int *ind, const double *Vg, const double *Ve, double *H_host,
                           long lda, hipStream_t s, std::string &msg);
int prdt_mv_dbg_solve_x(double *A, long n, long lda, double *x, bool device, long *bad_pivot, hipStream_t s, std::string &msg);
void prdt_tu_shutdown();

} // namespace gemma_hip

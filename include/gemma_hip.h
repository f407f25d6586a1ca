/*
 * gemma_hip.h -- C ABI of the MI355X (gfx950) implementation of GEMMA's
 * kinship + univariate-LMM hot path.
 *
 * GEMMA has no plugin/FFI layer; the boundary is cut at the internal C++
 * waists listed in SURVEY.md section 8(b).  Every entry point below names the
 * reference interface it replaces (file:line relative to the GEMMA tree).
 * INTEGRATION.md shows the few lines a GEMMA maintainer adds at each site.
 *
 * Conventions
 *  - plain pointers and sizes only; all matrices are row-major with an explicit
 *    leading dimension (maps 1:1 onto gsl_matrix{data,tda});
 *  - every function returns 0 on success or a GEMMA_HIP_E* code;
 *    gemma_hip_last_error() holds the detail text of the last failure;
 *  - entry points without suffix take HOST pointers (the library stages through
 *    device memory and never frees caller memory); the `_d` twins take DEVICE
 *    pointers plus a hipStream_t (passed as void*, NULL = the null stream) and
 *    are asynchronous on that stream;
 *  - one calling host thread (GEMMA is single-threaded); one process per GPU.
 *    Multi-GPU = one process per device, SNP blocks sharded by the caller and
 *    (U, eval, UtW, Uty) broadcast once into every rank's buffers (RCCL) before
 *    gemma_hip_lmm_setup_d;
 *  - there is NO CPU fallback: without a usable gfx950 device every call
 *    returns GEMMA_HIP_ENODEV.
 */
#ifndef GEMMA_HIP_H
#define GEMMA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4: gemma_mvlmm_null sized for 8 phenotypes / 11 covariates, gemma_mvlmm_opt gained `gxe` (round 4); 3: gemma_mvlmm_opt gained
 * `crt` (round 3); 2: the round-2 entry points */
#define GEMMA_HIP_ABI_VERSION 4

enum {
  GEMMA_HIP_OK = 0,
  GEMMA_HIP_EINVAL = 1,   /* bad argument / shape ("Range error in dgemm", src/fastblas.cpp:207) */
  GEMMA_HIP_ENODEV = 2,   /* no gfx950 device / not initialised */
  GEMMA_HIP_ENOMEM = 3,   /* device allocation failed */
  GEMMA_HIP_ERUNTIME = 4, /* HIP runtime / kernel failure */
  GEMMA_HIP_ESTATE = 5,   /* call sequence violated (e.g. lmm_batch before lmm_setup) */
  GEMMA_HIP_ENOCONV = 6,  /* eigensolver did not converge (INFO != 0, src/lapack.cpp:213,224) */
  GEMMA_HIP_ENOTPD = 7    /* matrix not positive definite (gemma_hip_spd_inverse, the REML fit of gemma_hip_vc_reml) */
};

/* == class SUMSTAT, src/param.h:54-66 (8 doubles per analysed SNP, in SNP order) */
typedef struct {
  double beta, se, lambda_remle, lambda_mle, p_wald, p_lrt, p_score, logl_H1;
} gemma_sumstat;

/* genotype block encodings accepted by kin_add / lmm_batch */
enum {
  /* fp64, SNP-major: l rows of ld doubles (ld >= n); NaN = missing.  Rows hold exactly
   * the individuals the consumer works on (analysed ones for lmm_batch, all for kin_add). */
  GEMMA_GENO_F64_SNP_MAJOR = 0,
  /* PLINK .bed payload, SNP-major: l rows of ld bytes (ld >= ceil(ni_total/4)), 4 individuals
   * per byte, low bits first, codes 00->2 01->missing(bit0=1,bit1=0) 10->1 11->0 exactly as
   * src/lmm.cpp:1797-1812.  Individuals are dropped on device with the indicator given to
   * gemma_hip_lmm_set_indicator (lmm_batch only; kin_add always uses all ni_total). */
  GEMMA_GENO_PLINK_2BIT = 1,
  /* fp64, individual-major: n rows of ld doubles, SNP j = strided column j (ld >= l) -- the
   * reference's own Xlarge layout (src/lmm.cpp:1502,1635; src/gemma_io.cpp:1439,1546).
   * Missing values must already be imputed by the caller (as the reference does before the
   * copy into Xlarge); for kin_add the columns must already be centred/scaled. */
  GEMMA_GENO_F64_IDV_MAJOR = 2
};

/* ---- lifetime ---------------------------------------------------------- */
int gemma_hip_init(int device /* -1: keep the current HIP device */, int verbose);
void gemma_hip_shutdown(void);
int gemma_hip_abi_version(void);
const char *gemma_hip_strerror(int code);
const char *gemma_hip_last_error(void);
/* name[len], number of CUs, HBM bytes of the device in use */
int gemma_hip_device_info(char *name, size_t len, int *n_cu, size_t *hbm_bytes);

/* ---- B2: GEMM ---------------------------------------------------------- */
/* replaces fast_dgemm / fast_eigen_dgemm, src/fastblas.h:34-39 (-> cblas_dgemm,
 * src/fastblas.cpp:202-204) and the raw fast_cblas_dgemm, src/fastblas.cpp:66-170:
 * C(MxN) = alpha*op(A)*op(B) + beta*C, row-major, ta/tb in {'N','T'}.
 * fp64 MFMA (v_mfma_f64_16x16x4_f64), LDS-tiled. */
int gemma_hip_dgemm(char ta, char tb, size_t M, size_t N, size_t K, double alpha, const double *A,
                    size_t lda, const double *B, size_t ldb, double beta, double *C, size_t ldc);
int gemma_hip_dgemm_d(char ta, char tb, size_t M, size_t N, size_t K, double alpha,
                      const double *A_d, size_t lda, const double *B_d, size_t ldb, double beta,
                      double *C_d, size_t ldc, void *stream);

/* ---- B1: streaming kinship --------------------------------------------- */
/* replaces the body of BimbamKin / PlinkKin, src/gemma_io.cpp:1418-1597 / :1599-1738, called
 * from PARAM::CalcKin src/param.cpp:1300-1321: per SNP over all n_total individuals mean over
 * non-missing, impute, centre, (k_mode 2: scale by 1/sqrt(var), var as :1511-1514),
 * K += Xb Xb^T per block, finally K /= ns_used (:1570) and symmetric fill (:1724-1729). */
int gemma_hip_kin_begin(size_t n_total, int k_mode /* 1 centred, 2 standardised */);
int gemma_hip_kin_add(int geno_kind, const void *geno, size_t l, size_t ld);
int gemma_hip_kin_add_d(int geno_kind, const void *geno_d, size_t l, size_t ld, void *stream);
int gemma_hip_kin_end(double *K /* n_total^2, row-major, full symmetric */, size_t *ns_used);
int gemma_hip_kin_end_d(double *K_d, size_t *ns_used, void *stream);

/* leave-one-chromosome-out kinship (-loco, src/param.cpp:52-66,497-500): given the kinship of ALL
 * analysed SNPs (ns_all of them) and of the SNPs on one chromosome (ns_chr), both from kin_begin/add/end_d,
 * overwrite K_chr_d with the kinship of the remaining SNPs: (ns_all K_all - ns_chr K_chr)/(ns_all - ns_chr). */
int gemma_hip_kin_loco_d(const double *K_all_d, size_t ns_all, double *K_chr_d, size_t ns_chr, size_t n,
                         void *stream);

/* ---- first-pass SNP QC ------------------------------------ */
/* The per-SNP filters of ReadFile_geno (src/gemma_io.cpp:753-853; kind F64_SNP_MAJOR, rows over all ni_total
 * individuals, NaN = "NA") and ReadFile_bed (:942-1049; kind PLINK_2BIT), statistics over the analysed
 * individuals only: missingness > miss_level, maf outside [maf_level, 1-maf_level] (skipped when maf_level == -1),
 * non-polymorphic, HWE exact test p < hwe_level (0 = off), r2 with the covariates > r2_level (only when
 * n_cvt > 1).  W is the n x n_cvt covariate matrix of the analysed individuals (host, row-major).
 * indicator_idv may be NULL when ni_total == n.  Outputs (host): indicator_snp[l], maf[l], n_miss[l]
 * (the latter two may be NULL). */
typedef struct {
  double maf_level;  /* 0.01  (src/param.cpp:94-107) */
  double miss_level; /* 0.05 */
  double hwe_level;  /* 0 */
  double r2_level;   /* 0.9999 */
} gemma_qc_cfg;
int gemma_hip_snp_qc(int geno_kind, const void *geno, size_t l, size_t ld, const int *indicator_idv,
                     size_t ni_total, const double *W, size_t n, size_t n_cvt, const gemma_qc_cfg *cfg,
                     int *indicator_snp, double *maf, size_t *n_miss);

/* ---- B3: centring + eigendecomposition --------------------------------- */
/* CenterMatrix(gsl_matrix*), src/mathfunc.cpp:147-177 (in place) */
int gemma_hip_center(double *G, size_t n);
int gemma_hip_center_d(double *G_d, size_t n, void *stream);
/* EigenDecomp_Zeroed, src/lapack.cpp:260-291 (-> lapack_eigen_symmv/dsyevr_, :149-236):
 * G (destroyed) -> U (row-major, eigenvector k = column k), eval ascending with values
 * < 1e-10 set to 0; *trace_G = mean(eval) (the function's return value, :277). */
int gemma_hip_eigh(double *G, size_t n, double *U, double *eval, double *trace_G);
int gemma_hip_eigh_d(double *G_d, size_t n, double *U_d, double *eval_d, double *trace_G,
                     void *stream);
/* The solver's device workspace is ~5 n^2 doubles in thirty-odd buffers, and hipMalloc / hipFree of such sizes cost 25-50 ms per GB
 * (0.1-0.2 s of a 1.9 s solve at n = 20 000, 1-2 s of 19 s at n = 50 000).  gemma_hip_eigh_reserve(n) allocates the workspace of order n
 * ahead of the solve (a caller that knows its n does this while it reads its files) and from then on every solve leaves its buffers in a
 * pool for the next one (LOCO: one decomposition per chromosome); gemma_hip_eigh_release hands the idle buffers back (lmm_setup* does
 * so by itself when the pool holds more than a quarter of the device).  GEMMA_HIP_EIGH_CACHE=1 keeps every solve's buffers without a
 * reserve call.  Without either the solver allocates and frees per call, as before.  gemma_hip_eigh_reserve touches nothing but the solver's
 * own pool: after gemma_hip_init it is the ONE entry point that may run on a second thread beside another call of the library (the file
 * driver issues it while the first pass reads the genotype file); join it before the first gemma_hip_eigh* call. */
int gemma_hip_eigh_reserve(size_t n);
int gemma_hip_eigh_release(size_t *bytes_freed /* may be NULL */);
/* The same as a COLLECTIVE over the library's communicator (gemma_hip_comm_init): every rank passes the same G and
 * receives the same (U, eval).  The reduction and the divide & conquer run on every rank (same code, same bits -- checked),
 * the two back-transformations are shared out by eigenvector (rows of Z^T) and the slices exchanged once; with one rank, or
 * GEMMA_HIP_EIGH_SHARD=0, it is gemma_hip_eigh_d. */
int gemma_hip_eigh_sharded_d(double *G_d, size_t n, double *U_d, double *eval_d, double *trace_G, void *stream);
/* CalcUtX(U,X,UtX), src/mathfunc.cpp:504-506: UtX (n x m) = U^T X (X n x m row-major) */
int gemma_hip_calc_utx(const double *U, const double *X, size_t n, size_t m, double *UtX);

/* ---- B4: per-batch association ------------------------------------------ */
/* the state batch_compute (src/lmm.cpp:1513-1564) reads from class LMM, src/lmm.h:53-74 */
typedef struct {
  int a_mode;          /* 1 Wald, 2 LRT, 3 score, 4 all, 9 (src/gemma.h:39-43) */
  size_t n;            /* ni_test */
  size_t n_cvt;        /* covariates incl. intercept (>= 1) */
  double l_min, l_max; /* 1e-5, 1e5 (src/param.cpp:94-107) */
  size_t n_region;     /* 10 */
  double l_mle_null;   /* null-model ML lambda (score test, src/lmm.cpp:1542) */
  double logl_mle_H0;  /* null-model ML log-likelihood (LRT, src/lmm.cpp:1553) */
  int plink_nan_rule;  /* 1: AnalyzePlink's handling of a failed lambda search (src/lmm.cpp:1870-1884) */
} gemma_lmm_cfg;

/* Null model (calc_null = true): CalcLambda('L'/'R', eval, UtW, Uty, ...) src/lmm.cpp:2143-2180 as
 * called at src/gemma.cpp:2711,2734, plus CalcPve (src/lmm.cpp:2183-2205) and the vg/ve part of
 * CalcLmmVgVeBeta (:2253-2259).  Host pointers.  out8 = { l_mle_null, logl_mle_H0, l_remle_null,
 * logl_remle_H0, pve, pve_se, vg_remle, ve_remle }. */
int gemma_hip_lmm_null(size_t n, size_t n_cvt, const double *eval, const double *UtW,
                       const double *Uty, double l_min, double l_max, size_t n_region,
                       double trace_G, double *out8);

/* uploads U (n x n row-major, eigenvectors in columns), eval, UtW (n x n_cvt row-major), Uty */
int gemma_hip_lmm_setup(const gemma_lmm_cfg *cfg, const double *U, const double *eval,
                        const double *UtW, const double *Uty);
/* same with device-resident inputs (borrowed until lmm_finish): the multi-GPU path, after the
 * single RCCL broadcast of (U, eval, UtW, Uty) */
int gemma_hip_lmm_setup_d(const gemma_lmm_cfg *cfg, const double *U_d, const double *eval_d,
                          const double *UtW_d, const double *Uty_d, void *stream);
/* for GEMMA_GENO_PLINK_2BIT: indicator_idv over ni_total individuals (sum == cfg.n);
 * NULL/0 resets to "all individuals analysed" */
int gemma_hip_lmm_set_indicator(const int *indicator_idv, size_t ni_total);
/* one block of l SNPs: mean-impute (src/lmm.cpp:1590-1618 / :1819-1827), UtX = U^T X (:1521),
 * then per SNP CalcUab, CalcRLScore, CalcLambda('R')+CalcRLWald, CalcLambda('L')+LRT (:1526-1562).
 * out[l] in SNP order. l is not limited to LMM_BATCH_SIZE.
 * U^T X: fp64 MFMA GEMM for real-valued input; for hard calls (GEMMA_GENO_PLINK_2BIT, or fp64 rows holding only
 * 0/1/2 and one missing / imputed value -- detected per batch) the same product as 2 D int8 MFMA products of
 * {genotype, missing mask} with D balanced base-256 digits of U, accumulated exactly in int32.  PRECISION OF THE OPERAND (round 6):
 * every column of U is scaled by its exact maximum and rounded at 1.01 * 2^(-8 D) of it.  D = 7 below n = 16384: 2^-56 of the column
 * maximum, below an fp64 entry's own rounding in the column's top binades, and the product is closer to the exact dot products than an
 * fp64 GEMM (which rounds every partial sum).  From n = 16384 up D = 6: U is ROUNDED to 2^-48 of each column's maximum -- narrower than
 * the reference's fp64 operand (2^-53 per entry); measured against long-double products the rms error of U^T x is 4.6 x that of the fp64
 * MFMA GEMM, the maximum 4.4 x, eight orders below the 1e-6 bar on the statistics.  GEMMA_HIP_I8_FORM=7g6m is the strict
 * form -- seven digits for the genotype product, the mask product (whose term is sqrt(n / missing calls) smaller) on the upper six:
 * rms and maximum error a quarter / an eighth of the fp64 GEMM's for 10/9 of the matrix work; GEMMA_HIP_I8_DIGITS=7 seven digits for both at
 * any n (14 products: 7/6 of the time), GEMMA_HIP_UTX_I8=0 selects the fp64 GEMM always.  The _d form is asynchronous on its stream for
 * GEMMA_GENO_PLINK_2BIT; for fp64 input it synchronises the stream once per call (the hard-call verdict is read back). */
int gemma_hip_lmm_batch(int geno_kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out);
int gemma_hip_lmm_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld,
                          gemma_sumstat *out_d, void *stream);
/* gemma_hip_lmm_batch_d with TWO BLOCKS IN FLIGHT on a CU partition (round 5; the loop of src/lmm.cpp:1526-1562 has no dependency
 * between blocks except AnalyzePlink's beta / se carry, which stays in block order): ingest, records and the int8 product of this
 * block run on 192 of the 256 CUs while the digit combine and the per-SNP stage of the PREVIOUS block run on the other 64 (two of the
 * eight CUs of every shader engine; GEMMA_HIP_PIPE_CUS=32|64|...; 0 = two plain streams).  The call returns when the work is QUEUED:
 * out_d of a block is complete only after gemma_hip_lmm_pipe_flush(stream) has ordered `stream` behind it (or after any other
 * batch entry point, which flushes first); geno_d may be overwritten once work queued on `stream` AFTER the next call (or the
 * flush) runs.  Records are the ones gemma_hip_lmm_batch_d writes, bit for bit.  PLINK 2-bit blocks on the records kernel only;
 * every other input takes gemma_hip_lmm_batch_d. */
int gemma_hip_lmm_batch_pipe_d(int geno_kind, const void *geno_d, size_t l, size_t ld, gemma_sumstat *out_d, void *stream);
int gemma_hip_lmm_pipe_flush(void *stream);
/* The same for a STREAM of host blocks, pipelined (pinned, double-buffered H2D; the feeder this replaces is the
 * per-SNP read loop of src/lmm.cpp:1776-1827): submit copies the block into one of two pinned staging slots and queues its
 * H2D copy (copy stream), the batch (compute stream, after the copy) and the D2H of its SUMSTAT records; collect waits for
 * the OLDEST submitted block and hands its records over.  At most two blocks in flight: submit(k + 1) before collect(k) moves
 * block k + 1 across PCIe while block k computes.  The caller's buffer is free again when submit returns. */
int gemma_hip_lmm_batch_submit(int geno_kind, const void *geno, size_t l, size_t ld);
int gemma_hip_lmm_batch_collect(gemma_sumstat *out /* room for the block's l records */, size_t *l /* may be NULL */);
/* LMM::AnalyzeGene (src/lmm.cpp:1365-1471; `-gene`): every row of Y (l x ld, row-major, ld >= cfg.n) is a PHENOTYPE
 * (a gene's expression over the analysed individuals); the tested variable is the one fixed vector whose rotation
 * U^T x was handed to gemma_hip_lmm_setup in the Uty slot.  Per row: U^T y_g (:1415), the row's own null ML fit
 * (l_H0, logl_H0, :1424-1427), CalcRLScore at l_H0, CalcLambda('R')+CalcRLWald, CalcLambda('L')+LRT against logl_H0
 * (:1434-1450).  l_mle_null / logl_mle_H0 of the cfg are not used. */
int gemma_hip_lmm_gene_batch(const double *Y, size_t l, size_t ld, gemma_sumstat *out);
int gemma_hip_lmm_gene_batch_d(const double *Y_d, size_t l, size_t ld, gemma_sumstat *out_d, void *stream);
/* GXE variants, LMM::AnalyzeBimbamGXE / AnalyzePlinkGXE (src/lmm.cpp:2283-2608; `-gxe`): the covariates of SNP s are
 * [W, env, x_s] and the tested variable is x_s . env.  After lmm_setup: set_env(env over the cfg.n analysed individuals)
 * rotates env (:2308); gxe_batch takes SNP-major blocks (GEMMA_GENO_F64_SNP_MAJOR or GEMMA_GENO_PLINK_2BIT with the
 * lmm_set_indicator mapping), mean-imputes, recodes 2 - x when x_mean > 1 (beta changes sign, :2352-2354,:2403), and per
 * SNP runs the c+2-covariate null ML fit (a_mode 2/4), CalcRLScore at cfg.l_mle_null, REML + Wald, ML + LRT (:2376-2400). */
int gemma_hip_lmm_set_env(const double *env);
int gemma_hip_lmm_gxe_batch(int geno_kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out);
int gemma_hip_lmm_gxe_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, gemma_sumstat *out_d, void *stream);
/* the second half of lmm_batch on a caller-supplied UtX (SNP-major l x ld_utx, device):
 * what remains of batch_compute after the fast_dgemm at src/lmm.cpp:1521 */
int gemma_hip_lmm_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, gemma_sumstat *out_d,
                          void *stream);
/* releases the LMM state; reports GPU time spent in the UtX GEMM and in the per-SNP stage in
 * minutes, the unit of LMM::time_UtX / time_opt (src/lmm.cpp:1523,1556) */
int gemma_hip_lmm_finish(double *time_UtX_min, double *time_opt_min);

/* ---- T univariate LMMs over one U^T x (trait panels) ------------------------------------------------------ */
/* T phenotypes on the same individuals, kinship and covariates: a block is ingested and rotated (U^T x) ONCE and the per-SNP
 * stage of LMM::Analyze runs for every phenotype.  The records of phenotype t are, bit for bit, those of gemma_hip_lmm_setup with
 * column t of UtY and cfg's null fields set to l_mle_null[t] / logl_mle_H0[t], followed by gemma_hip_lmm_batch on the same blocks
 * in the same order (each phenotype has its own PLINK beta / se carry chain).  The scan runs on ONE set of analysed individuals:
 * per-phenotype missingness is not supported -- the caller analyses the individuals that have every phenotype (and covariate), as
 * the reference does for `-n a b c` (ProcessCvtPhen).
 * UtY: n x T row-major (the layout gemma_hip_mvlmm_null takes); l_mle_null / logl_mle_H0: T values each (read for a_mode 2/3/4/9 as
 * cfg's two fields are; may be NULL for a_mode 1); cfg's own two null fields are ignored.  T = 1..GEMMA_LMM_MULTI_MAX, else
 * GEMMA_HIP_EINVAL; tables that do not fit: GEMMA_HIP_ENOMEM with the byte count in the message.  gemma_hip_lmm_set_indicator and
 * gemma_hip_lmm_finish serve both forms; a single-phenotype batch entry point after a multi setup, and a multi batch after a
 * single-phenotype setup, return GEMMA_HIP_ESTATE.  No multi form of -gxe, -gene, batch_pipe_d, batch_submit / collect, mvLMM.
 * The fixed-lambda tables of up to 5 - n_cvt phenotypes at a time come from one read of U^T x (GEMMA_HIP_MULTI_TABLE=0: one read
 * per phenotype; the same bits either way). */
#define GEMMA_LMM_MULTI_MAX 64
int gemma_hip_lmm_multi_setup(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *logl_mle_H0,
                              const double *U, const double *eval, const double *UtW, const double *UtY);
/* device pointers; U_d and eval_d are borrowed until gemma_hip_lmm_finish, UtW_d and UtY_d are read by work queued on `stream` */
int gemma_hip_lmm_multi_setup_d(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *logl_mle_H0,
                                const double *U_d, const double *eval_d, const double *UtW_d, const double *UtY_d, void *stream);
/* on the kept U (gemma_hip_eigh_kept_K / gemma_hip_eigh_keep); UtW, UtY: host */
int gemma_hip_lmm_multi_setup_kept(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *logl_mle_H0,
                                   const double *UtW, const double *UtY);
/* one block: ingest + U^T x once, then the per-SNP stage for every phenotype.  out: T x l records, phenotype-major (out[t * l + s]). */
int gemma_hip_lmm_multi_batch(int geno_kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out);
int gemma_hip_lmm_multi_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, gemma_sumstat *out_d, void *stream);

/* ---- score panel: `-lmm 3` of T phenotypes over one U^T x, T in the thousands -------------------------------- */
/* The first pass over an omics panel (expression, protein, metabolite levels on the same individuals, kinship and covariates) is
 * the score test at each phenotype's null lambda: LMM::CalcRLScore (src/lmm.cpp:1170-1211) at l_mle_null, no lambda search per
 * SNP.  At a fixed lambda the statistic is a closed form of c + 2 weighted sums over the individuals per (SNP, phenotype) pair, and
 * for all pairs of a block those sums are ONE product of [x.x | x] (the block's U^T x) against an n x T (c + 2) weight matrix:
 * a block costs ingest + U^T x once and one matrix kernel with the statistics in its epilogue.  The reference has no such mode
 * (it runs `-lmm 3 -n t` once per trait); the records are the ones those runs print.
 * cfg->a_mode must be 3 (the other modes search lambda per SNP: gemma_hip_lmm_multi_*) and cfg->n_cvt 1..16, else GEMMA_HIP_EINVAL;
 * cfg's own two null fields are ignored.  l_mle_null: T values on the host, UtY: n x T row-major.  T >= 1 with no fixed upper cap:
 * a setup keeps 8 n (c + 2) bytes per phenotype (rounded up to groups of 16), and buffers that do not fit return GEMMA_HIP_ENOMEM
 * with the byte count in the message.  A phenotype whose UtW^T diag(h) UtW is not positive definite (collinear covariates, a
 * non-finite lambda) fails the setup with GEMMA_HIP_EINVAL and a message naming it.
 * gemma_hip_lmm_set_indicator and gemma_hip_lmm_finish serve this form too; every single-phenotype or multi batch entry point after a
 * score-panel setup, and a score-panel batch after a single-phenotype or multi setup, return GEMMA_HIP_ESTATE.
 * Rows that are monomorphic or all-missing after imputation get what the formulas give on a P_xx of rounding noise. */
typedef struct {
  double beta, se, p_score;
} gemma_score_rec;
int gemma_hip_lmm_score_panel_setup(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null,
                                    const double *U, const double *eval, const double *UtW, const double *UtY);
/* device pointers; U_d and eval_d are borrowed until gemma_hip_lmm_finish, UtW_d and UtY_d are read before the call returns */
int gemma_hip_lmm_score_panel_setup_d(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null,
                                      const double *U_d, const double *eval_d, const double *UtW_d, const double *UtY_d, void *stream);
/* on the kept U (gemma_hip_eigh_kept_K / gemma_hip_eigh_keep); UtW, UtY: host */
int gemma_hip_lmm_score_panel_setup_kept(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null,
                                         const double *UtW, const double *UtY);
/* one block: ingest + U^T x as gemma_hip_lmm_batch runs them (same genotype kinds, indicator mapping and mean imputation), then the
 * product.  out: T x l records, phenotype-major (out[t * l + s]). */
int gemma_hip_lmm_score_panel_batch(int geno_kind, const void *geno, size_t l, size_t ld, gemma_score_rec *out);
int gemma_hip_lmm_score_panel_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, gemma_score_rec *out_d, void *stream);
/* the product alone, on a caller-made U^T x (l x n SNP-major, leading dimension ld_utx >= n) */
int gemma_hip_lmm_score_panel_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, gemma_score_rec *out_d, void *stream);

/* The hits form of a block: instead of the T x l records, the pairs with p_score <= p_max and the best pair of every phenotype.
 * The product is the one of the records form and a hit's (beta, se, p_score) are the bits of the record of its pair; the F tail
 * runs only on pairs whose F statistic passes a pre-filter at the critical value of p_max, and nothing of size T x l is stored.
 *   hits / cap   the list and its size in entries; snp is the row inside the block.  n_hits always receives the number of
 *                qualifying pairs of the block: where it exceeds cap the call still returns GEMMA_HIP_OK, the list holds an
 *                unspecified cap of the hits, and the caller repeats the block with a larger list.  hits == NULL with cap == 0
 *                counts only.  The host form returns the list sorted by (pheno, snp); the _d forms leave it in ARRIVAL ORDER
 *                (which differs from run to run: sort it, by (pheno, snp), where the order matters).
 *   best         NULL, or T entries: per phenotype the pair with the largest finite F of the block (the smallest p_score), the
 *                smallest row among equal F; snp = -1 and NaN fields where the block has no such pair (and for l == 0).
 *   p_max        in [0, 1]; anything else, NaN included: GEMMA_HIP_EINVAL.
 * A pair whose P_xx is below 1e-8 of sum h x^2 (the row is collinear with the covariates -- monomorphic --, its statistics are
 * rounding noise) or NaN (no called genotype) is neither a hit nor a best.  State rules and genotype handling as the records form. */
typedef struct {
  uint32_t snp, pheno;
  double beta, se, p_score;
} gemma_score_hit;
typedef struct {
  double beta, se, p_score;
  int64_t snp;
} gemma_score_best;
int gemma_hip_lmm_score_panel_hits_batch(int geno_kind, const void *geno, size_t l, size_t ld, double p_max,
                                         gemma_score_hit *hits, size_t cap, unsigned long long *n_hits, gemma_score_best *best);
int gemma_hip_lmm_score_panel_hits_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, double p_max,
                                           gemma_score_hit *hits_d, size_t cap, unsigned long long *n_hits_d, gemma_score_best *best_d,
                                           void *stream);
/* the product alone, on a caller-made U^T x */
int gemma_hip_lmm_score_panel_hits_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, double p_max,
                                           gemma_score_hit *hits_d, size_t cap, unsigned long long *n_hits_d, gemma_score_best *best_d,
                                           void *stream);

/* The refinement of the hits: each pair's own lambda-hats, the Wald test and the likelihood-ratio test -- the `-lmm 4` columns of
 * (SNP, phenotype) -- for a list of pairs, one wavefront per pair, every evaluation streaming the pair's two rows (a scattered list
 * has no fixed-lambda table to share).  The contract: for every pair, the eight fields of gemma_hip_lmm_score_panel_refine_assoc_d
 * are byte-equal to row `snp` of gemma_hip_lmm_setup_d with a_mode 4, the same cfg, plink_nan_rule 0, column `pheno` of UtY and
 * l_mle_null[pheno] / logl_mle_H0[pheno], followed by gemma_hip_lmm_assoc_d on the same UtX, with GEMMA_HIP_ASSOC_GRID=0 in the
 * environment of that setup.  p_score, beta and se of a refined record are those of the `-lmm 4` body, not copies of the hit; a
 * failed lambda search follows the BIMBAM rule (NaN beta, se, p_wald: a pair has no previous SNP).
 *   refine_setup   after a score-panel setup: keeps what the refinement needs, a T x n transposed U^T Y of its own (the score-panel
 *                  setup still releases its copy) and the T logl_mle_H0; l_min, l_max and n_region are the setup's cfg, l_mle_null
 *                  the setup's own.  A copy that does not fit: GEMMA_HIP_ENOMEM with the byte count.  Both forms return with UtY and
 *                  logl_mle_H0 read.  gemma_hip_lmm_finish and a new setup take the refinement state down with the score panel.
 *   pairs / m      gemma_score_hit entries of which only snp and pheno are read: a hits list can be passed straight in.  A pair
 *                  with snp >= l or pheno >= T gets an all-NaN record and no memory access; m == 0 returns GEMMA_HIP_OK and touches
 *                  nothing.  out[i] belongs to pairs[i]; the order and repetitions of the list are the caller's.
 *   refine_last_d  the same on the U^T x of the most recent score-panel batch (records or hits form) of this setup.
 *   hits_refine_batch  the host form of a block: the hits form plus one gemma_sumstat per returned hit, refined[i] for hits[i] after
 *                  the sort; where n_hits > cap, refined is unspecified as the list is.  Only this form synchronises; the _d forms
 *                  queue their work on `stream`.
 * GEMMA_HIP_ESTATE: any of these before a score-panel setup; refine_assoc_d, refine_last_d or hits_refine_batch before refine_setup;
 * refine_last_d with no score-panel block since the setup, or after any entry point that has overwritten the U^T x buffer
 * (gemma_hip_dbg_utx, for one).  GEMMA_HIP_EINVAL: a null pointer with m > 0 (cap > 0 for refined), ld_utx < n. */
int gemma_hip_lmm_score_panel_refine_setup(const double *UtY /* n x T row-major, host */, const double *logl_mle_H0 /* T, host */);
int gemma_hip_lmm_score_panel_refine_setup_d(const double *UtY_d, const double *logl_mle_H0 /* host */, void *stream);
/* records of m pairs on a caller-made U^T x (as ..._hits_assoc_d takes it) */
int gemma_hip_lmm_score_panel_refine_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, const gemma_score_hit *pairs_d, size_t m,
                                             gemma_sumstat *out_d, void *stream);
int gemma_hip_lmm_score_panel_refine_last_d(const gemma_score_hit *pairs_d, size_t m, gemma_sumstat *out_d, void *stream);
int gemma_hip_lmm_score_panel_hits_refine_batch(int geno_kind, const void *geno, size_t l, size_t ld, double p_max,
                                                gemma_score_hit *hits, size_t cap, unsigned long long *n_hits,
                                                gemma_score_best *best, gemma_sumstat *refined /* cap records */);

/* ---- null fits of a whole panel: what gemma_hip_lmm_null gives for one column of U^T Y, for every column ------------------- */
/* The nulls the panel setups above are handed (l_mle_null, logl_mle_H0) and each trait's own result -- heritability, vg / ve, the
 * covariate effects (the reference prints them in its log, src/gemma.cpp:3402-3430) -- in one launch per chunk of columns, one
 * wavefront per phenotype.  fit[t] equals, in all eight fields and in every bit, what gemma_hip_lmm_null returns for column t.
 * UtY: n x T row-major, the layout the panel setups take.  beta / se_beta: NULL (both), or T x n_cvt row-major: the covariate
 * effects at l_remle_null and their standard errors, CalcLmmVgVeBeta src/lmm.cpp:2210-2281, for n_cvt <= 16; a phenotype whose
 * UtW^T H UtW is not positive definite there (or whose lambda is not finite) gets NaN in its own row and the call still succeeds.
 * Stateless like gemma_hip_lmm_null: no LMM setup is needed or disturbed.  The columns are walked in chunks sized from the free
 * device memory (GEMMA_HIP_NULL_PANEL_CHUNK=<columns>, read at the call, forces the size); a chunk that does not fit returns
 * GEMMA_HIP_ENOMEM with the byte count.  GEMMA_HIP_EINVAL: T == 0, a null pointer (other than beta with se_beta), one of beta /
 * se_beta without the other, n <= n_cvt, n above 2 097 120 (65 535 x 32), n_cvt outside 1..65, beta with n_cvt > 16, l_max <= l_min, n_region outside 1..64.
 * The _d form takes device pointers throughout, queues its work on `stream` and synchronises it before it returns. */
typedef struct {
  double l_mle_null, logl_mle_H0, l_remle_null, logl_remle_H0, pve, pve_se, vg_remle, ve_remle;
} gemma_null_fit; /* = out8 of gemma_hip_lmm_null */
int gemma_hip_lmm_null_panel(size_t n, size_t n_cvt, size_t T, const double *eval, const double *UtW, const double *UtY,
                             double l_min, double l_max, size_t n_region, double trace_G, gemma_null_fit *fit, double *beta,
                             double *se_beta);
int gemma_hip_lmm_null_panel_d(size_t n, size_t n_cvt, size_t T, const double *eval_d, const double *UtW_d, const double *UtY_d,
                               double l_min, double l_max, size_t n_region, double trace_G, gemma_null_fit *fit_d, double *beta_d,
                               double *se_beta_d, void *stream);

/* ---- multivariate LMM (-lmm 1..4 -n a b c ...) ------------------------------------ */
/* MVLMM::AnalyzeBimbam / AnalyzePlink, src/mvlmm.cpp:2972-3416 / :3418-3899, and with opt->gxe the interaction test of
 * AnalyzeBimbamGXE / AnalyzePlinkGXE (:3970-4414 / :4416-4870).  d phenotypes (1..GEMMA_MV_DMAX), n_cvt covariates with
 * n_cvt + 1 <= GEMMA_MV_CMAX rows of X (gxe: n_cvt + 3): register-resident kernels for d <= 7 with up to 3 covariates, d <= 3
 * with up to 6 and d = 8 with one, one run-time-shaped kernel (slower) for every other shape and for gxe.  opt->crt = 1 applies the Edgeworth
 * correction (CalcCRT / PCRT, :2054-2358 / :2952-2970) as -crt does.
 * gemma_mvlmm_null holds what the null-model block (:3056-3208) leaves behind: V_g, V_e (d x d row-major, leading
 * dimension d), B (d x n_cvt) and the log-likelihood, for the REMLE and the MLE fit. */
#define GEMMA_MV_DMAX 8
#define GEMMA_MV_CMAX 12
typedef struct {
  double Vg_remle[GEMMA_MV_DMAX * GEMMA_MV_DMAX], Ve_remle[GEMMA_MV_DMAX * GEMMA_MV_DMAX], B_remle[GEMMA_MV_DMAX * GEMMA_MV_CMAX],
      logl_remle_H0;
  double Vg_mle[GEMMA_MV_DMAX * GEMMA_MV_DMAX], Ve_mle[GEMMA_MV_DMAX * GEMMA_MV_DMAX], B_mle[GEMMA_MV_DMAX * GEMMA_MV_CMAX], logl_mle_H0;
} gemma_mvlmm_null;
/* PARAM defaults (src/param.cpp:94-107): em_iter 10000, em_prec 1e-4, nr_iter 100, nr_prec 1e-4, p_nr 1e-3, crt 0 */
typedef struct {
  size_t em_iter, nr_iter;
  double em_prec, nr_prec, p_nr;
  size_t crt; /* PARAM::crt (-crt, src/gemma.cpp:1398-1399): 1 = PCRT on the SNPs that reach MphNR (:3302-3306,3329-3331,3349-3351) */
  size_t gxe; /* 1 (-gxe with several phenotypes, src/gemma.cpp:2840-2851): after gemma_hip_lmm_set_env; mvlmm_set then takes the null
               * fit of (W, env) -- gemma_hip_mvlmm_null called with U^T env appended to UtW as covariate n_cvt + 1 (:4046-4070) --
               * and mvlmm_batch tests x o env per SNP with (W, env, x) as covariates; SNP-major input only; beta changes sign with
               * the allele switch of :4232-4236 */
} gemma_mvlmm_opt;
/* The null block: MphInitial (:2763-2948; one univariate REML fit per trait, and for d > 4 one two-trait fit per pair),
 * MphEM + MphNR + MphCalcBeta for 'R', then for 'L' starting from the REMLE fit.  Host pointers: eval (n), UtW (n x
 * n_cvt row-major), UtY (n x d row-major) -- the arguments of AnalyzeBimbam.  Stand-alone (no lmm_setup needed). */
int gemma_hip_mvlmm_null(size_t n, size_t n_cvt, size_t d, const double *eval, const double *UtW, const double *UtY,
                         double l_min, double l_max, size_t n_region, const gemma_mvlmm_opt *opt, gemma_mvlmm_null *out);
/* After gemma_hip_lmm_setup (which holds U, eval, UtW, cfg.a_mode, cfg.n, cfg.n_cvt; its Uty slot is not read by this
 * path): the rotated phenotypes UtY (n x d row-major, host) and the null fit the per-SNP loop starts from (:3206-3208:
 * the MLE block; logl_mle_H0 is the LRT reference). */
int gemma_hip_mvlmm_set(size_t d, const double *UtY, const gemma_mvlmm_null *null_fit, const gemma_mvlmm_opt *opt);
/* One block of SNPs (:3218-3375), same genotype encodings / indicator mapping / imputation as lmm_batch.  Per SNP the
 * record MPHSUMSTAT (src/param.h:68-77) as doubles: beta[d], Vbeta[v], Vg[v], Ve[v], p_wald, p_lrt, p_score with
 * v = d (d + 1) / 2 (upper triangles, row by row) -- out holds l x (d + 3 v + 3) doubles. */
int gemma_hip_mvlmm_batch(int geno_kind, const void *geno, size_t l, size_t ld, double *out);
int gemma_hip_mvlmm_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, double *out_d, void *stream);
/* Which multivariate kernel the library launched last, recorded where a missing fixed instance falls back to the run-time kernel.
 * which 0: the last per-SNP launch (mvlmm_batch*); 1: the last d-variate null fit of mvlmm_null (not its pairwise two-trait
 * fits).  *form: GEMMA_MV_KERNEL_*; *d: phenotypes; *rows: rows of X of that launch (per-SNP: covariates + the SNP [+ env and
 * the interaction row]; null fit: covariates).  Any of the three pointers may be null. */
enum { GEMMA_MV_KERNEL_NONE = 0, GEMMA_MV_KERNEL_FIXED = 1, GEMMA_MV_KERNEL_RUN_TIME = 2 };
int gemma_hip_dbg_last_mvlmm_kernel(int which, int *form, int *d, int *rows);

/* ---- the null block's standard errors, and two-trait null fits of a whole panel -------------------------------------------- */
/* gemma_hip_mvlmm_null_se: gemma_hip_mvlmm_null -- the same computation, the same bits in `out`, the same report through
 * gemma_hip_dbg_last_mvlmm_kernel(1, ...) -- plus what the reference's null block leaves in VVg_*_null, VVe_*_null and
 * se_beta_*_null (src/mvlmm.cpp:3074-3093, :3140-3159), as VARIANCES (the reference prints safe_sqrt of them, :3110 / :918):
 * VVg / VVe [v], v = d (d + 1) / 2 in GetIndex order (upper triangle row by row): the diagonal of MphNR's variance matrix -H^-1
 * (:2742-2744), H being the Hessian of MphNR's last CalcDev call; VB [d x n_cvt]: the diagonal of MphCalcBeta's Vbeta (:835-921). */
typedef struct {
  double VVg_remle[GEMMA_MV_DMAX * (GEMMA_MV_DMAX + 1) / 2], VVe_remle[GEMMA_MV_DMAX * (GEMMA_MV_DMAX + 1) / 2],
      VB_remle[GEMMA_MV_DMAX * GEMMA_MV_CMAX];
  double VVg_mle[GEMMA_MV_DMAX * (GEMMA_MV_DMAX + 1) / 2], VVe_mle[GEMMA_MV_DMAX * (GEMMA_MV_DMAX + 1) / 2],
      VB_mle[GEMMA_MV_DMAX * GEMMA_MV_CMAX];
} gemma_mvlmm_null_se;
int gemma_hip_mvlmm_null_se(size_t n, size_t n_cvt, size_t d, const double *eval, const double *UtW, const double *UtY,
                            double l_min, double l_max, size_t n_region, const gemma_mvlmm_opt *opt, gemma_mvlmm_null *out,
                            gemma_mvlmm_null_se *se);
/* gemma_hip_mvlmm_null_pairs: for every listed pair (i, j), i < j, of the T columns of UtY (n x T row-major) the two-trait null fit
 * gemma_hip_mvlmm_null(d = 2) gives on columns i and j -- Vg, Ve, logl and B in the same bits -- with the variances above and the
 * genetic / residual correlations: one wavefront per pair, every pair of a chunk in one launch.  Entries are ordered 00, 01, 11.
 * rg = Vg01 / sqrt(Vg00 Vg11), var_rg by the delta method from the 3 x 3 V_g block of -H^-1 (re / var_re likewise; the library's
 * own, the reference prints none); a non-finite or non-positive diagonal gives NaN.  status 0: ok; 1: some field of the pair is not
 * finite (the call still succeeds, other pairs are untouched).  pairs: 2 m ints (i0, j0, i1, j1, ...), or NULL for all i < j row by
 * row (m then 0 or T (T - 1) / 2; fit holds T (T - 1) / 2).  B / VB: NULL (both), or m x 2 x 2 x n_cvt (pass REMLE / MLE, trait,
 * covariate).  The univariate starts of all T columns come from one null-panel launch; the pairs are walked in chunks sized from
 * the free device memory (16 n bytes of gathered rows per pair; GEMMA_HIP_MVPAIR_CHUNK=<pairs>, read at the call, forces the size;
 * a chunk that does not fit returns GEMMA_HIP_ENOMEM with the byte count).  Stateless: no LMM setup is needed or disturbed.
 * GEMMA_HIP_EINVAL: a null pointer (other than pairs, and B with VB), one of B / VB without the other, T < 2, m == 0 with pairs
 * given, m neither 0 nor T (T - 1) / 2 without, a pair with i >= j or j >= T, n <= n_cvt + 1, n_cvt outside 1..6 (the fixed
 * two-trait instances).  The _d form takes device pointers throughout (pairs included), queues its work on `stream` and
 * synchronises it before it returns; it copies the list back (8 bytes per pair) to check it before anything is launched. */
typedef struct { double Vg[3], Ve[3], VVg[3], VVe[3], rg, var_rg, re, var_re, logl; } gemma_mvpair_block; /* 00, 01, 11 */
typedef struct { int i, j, status, pad; gemma_mvpair_block remle, mle; } gemma_mvpair_fit;
int gemma_hip_mvlmm_null_pairs(size_t n, size_t n_cvt, size_t T, const double *eval, const double *UtW, const double *UtY,
                               const int *pairs, size_t m, double l_min, double l_max, size_t n_region, const gemma_mvlmm_opt *opt,
                               gemma_mvpair_fit *fit, double *B, double *VB);
int gemma_hip_mvlmm_null_pairs_d(size_t n, size_t n_cvt, size_t T, const double *eval_d, const double *UtW_d, const double *UtY_d,
                                 const int *pairs_d, size_t m, double l_min, double l_max, size_t n_region,
                                 const gemma_mvlmm_opt *opt, gemma_mvpair_fit *fit_d, double *B_d, double *VB_d, void *stream);

/* ---- linear model without a random effect (-lm 1..4) ----------------------- */
/* LM::AnalyzeBimbam / AnalyzePlink, src/lm.cpp:382-640 (CalcvPv :224-263, LmCalcP :266-287): per SNP ordinary
 * regression of y on (W, x); a_mode 51 Wald, 52 LRT, 53 score, 54 all (src/gemma.h:39-43).  W (n x n_cvt) and y are
 * host arrays over the analysed individuals.  Blocks use the same genotype encodings, indicator
 * (gemma_hip_lmm_set_indicator) and mean imputation as lmm_batch; SUMSTAT carries beta, se (score se for a_mode 53),
 * p_wald, p_lrt, p_score, the lambdas are 0 and logl_H1 is -0.0 as in the reference. */
int gemma_hip_lm_setup(int a_mode, size_t n, size_t n_cvt, const double *W, const double *y);
int gemma_hip_lm_batch(int geno_kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out);
int gemma_hip_lm_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, gemma_sumstat *out_d, void *stream);
int gemma_hip_lm_finish(void);

/* ---- the device-resident chain behind the host-pointer API ------------------------------ */
/* In a file-driven run K, the analysed block G and U cross PCIe five times (K out of kin_end, G into eigh, U out, U in
 * for CalcUtX, U in for lmm_setup: 8 n^2 bytes each).  These entry points keep them where they are produced.  One kept K
 * and one kept (U, eval) per process; lmm_finish does not release them, gemma_hip_kept_release does.
 *   kin_begin / kin_add ... -> kin_end_keep            K (ni_total^2) stays on the device; with a communicator of more than one
 *                                                       rank and allreduce != 0 the ranks' partial sums over THEIR SNPs are
 *                                                       all-reduced first (SNP-sharded kinship) and ns_used is the total
 *   kept_K_get                                          copy of the kept K for <o>.cXX.txt (PARAM::WriteMatrix)
 *   eigh_kept_K(indicator_idv)                          rows / columns of the analysed individuals (what ReadFile_kin keeps,
 *                                                       src/gemma_io.cpp:1205-1243), CenterMatrix, EigenDecomp_Zeroed -- all on the
 *                                                       device; U and eval stay there, eval and trace_G also come back
 *   eigh_keep(G)                                        the same from a host G (the -k file route): G is centred by the caller
 *   kept_bcast(root)                                    ONE ncclBroadcast of (U, eval) to every rank of the communicator
 *   calc_utx_kept / lmm_setup_kept                      CalcUtX and lmm_setup on the kept U
 *   kept_U_get                                          copy of U / eval for the -eigen artefacts */
int gemma_hip_kin_end_keep(size_t *ns_used, int allreduce);
int gemma_hip_kept_K_get(double *K /* ni_total^2 */);
int gemma_hip_eigh_kept_K(const int *indicator_idv /* NULL: all */, size_t ni_total, double *eval /* n_test, may be NULL */,
                          double *trace_G);
int gemma_hip_eigh_keep(const double *G /* n^2, already centred; not modified */, size_t n, double *eval /* may be NULL */,
                        double *trace_G);
int gemma_hip_kept_n(size_t *n /* order of the kept U, 0 = none */);
/* gemma_hip_eigh_kept_K as a collective (every rank holds the same kept K after the all-reduce of kin_end_keep): every rank ends
 * with the same kept (U, eval); gemma_hip_kept_bcast is then not needed */
int gemma_hip_eigh_kept_K_sharded(const int *indicator_idv, size_t ni_total, double *eval, double *trace_G);
int gemma_hip_kept_bcast(int root, double *trace_G /* out on every rank: mean(eval) of the root's decomposition; may be NULL */);
int gemma_hip_kept_U_get(double *U /* n^2, may be NULL */, double *eval /* n, may be NULL */);
int gemma_hip_calc_utx_kept(const double *X, size_t n, size_t m, double *UtX);
int gemma_hip_lmm_setup_kept(const gemma_lmm_cfg *cfg, const double *UtW, const double *Uty);
int gemma_hip_kept_release(void);

/* ---- multi-GPU: RCCL over xGMI, one process per GPU ------------------------------------------ */
/* SNPs are independent (src/lmm.cpp:1513-1514); the shared state is read-only.  Two collectives exist on the path: ONE
 * broadcast of (U, eval) from the rank that ran the eigensolver, and -- for a SNP-sharded kinship -- ONE all-reduce of the
 * n^2 partial sums.  Both are issued directly on RCCL (ncclBroadcast / ncclAllReduce, librccl bound with dlopen when a
 * communicator of more than one rank is created).  Bootstrap: rank 0 calls comm_unique_id (ncclGetUniqueId), the host
 * program ships the 128 bytes to the other ranks, every rank calls comm_init with its device current (ncclCommInitRank).
 * GEMMA_HIP_COMM=shm in the environment selects a host shared-memory transport instead: a TEST hook for boxes with one
 * GPU (RCCL refuses two ranks on one device); it is never chosen implicitly. */
#define GEMMA_HIP_COMM_ID_BYTES 128
int gemma_hip_comm_unique_id(void *id /* GEMMA_HIP_COMM_ID_BYTES */);
int gemma_hip_comm_init(const void *id /* may be NULL when world == 1 */, int rank, int world);
int gemma_hip_comm_info(int *rank, int *world, int *transport /* 0 none, 1 RCCL, 2 shm test transport */);
int gemma_hip_comm_bcast_d(void *buf_d, size_t bytes, int root, void *stream);
int gemma_hip_comm_allreduce_sum_d(double *buf_d, size_t count, void *stream);
int gemma_hip_comm_finalize(void);
/* The first contact of a new communicator: ONE KiB through both collectives (an all-reduce of rank + 1, a broadcast from rank 0 and one
 * from the last rank; every value checked on every rank) before anything n^2 is trusted to them.  Synchronous; a caller that cannot
 * afford a hang runs it under its own wall-clock deadline (bench.py: a helper thread).  Every collective above is cut into pieces of at
 * most 1 GiB issued back to back on the caller's stream.  GEMMA_HIP_COMM_FAIL=init|selftest|allreduce|bcast|allreduce_large|bcast_large
 * makes that entry point fail on every rank (the *_large forms only from 1 MiB up, i.e. after a passed self-test): failure injection
 * for the callers' fall-backs. */
int gemma_hip_comm_selftest(void *stream);
/* what the communicator has carried since gemma_hip_comm_init; the seconds are host wall time around synchronised collectives and stay
 * zero unless GEMMA_HIP_COMM_TIMING=1 is in the environment */
typedef struct {
  long allreduce_calls, allreduce_pieces, bcast_calls, bcast_pieces;
  double allreduce_bytes, bcast_bytes, allreduce_s, bcast_s;
} gemma_comm_stats;
int gemma_hip_comm_stats(gemma_comm_stats *out);

/* ---- measurement -------------------------------------------------------- */
enum { GEMMA_STAGE_INGEST = 0, GEMMA_STAGE_UTX_GEMM = 1, GEMMA_STAGE_ASSOC = 2,
       GEMMA_STAGE_KIN_GEMM = 3, GEMMA_STAGE_EIGH = 4,
       GEMMA_STAGE_UTX_POST = 5, /* int8-digit path only: int32 digit sums -> fp64 U^T x */
       GEMMA_STAGE_COUNT = 6 };
/* when on, every kernel of a stage is bracketed by hipEvents on its launch stream */
int gemma_hip_profile_enable(int on);
/* synchronises, then returns accumulated GPU milliseconds and launch count; reset != 0 clears */
int gemma_hip_profile_read(int stage, double *total_ms, long *launches, int reset);

/* ---- diagnostics: the stages of gemma_hip_eigh in isolation (host pointers; tests only) ---- */
/* Householder tridiagonalisation: d[n], e[n-1], tau[n], VT (n x n, row j = reflector u_j; may be NULL) */
int gemma_hip_dbg_tridiag(const double *G, size_t n, double *d, double *e, double *tau, double *VT);
/* divide and conquer on a symmetric tridiagonal: w[n] ascending, ZT (n x n, row k = eigenvector k) */
int gemma_hip_dbg_stedc(const double *d, const double *e, size_t n, double *w, double *ZT);
/* two-stage reduction of the eigensolver alone (n even, >= 384): band (n x 129, row j = B(j..j+128, j)) after the dense ->
 * band stage, d[n], e[n-1] after the bulge chase */
int gemma_hip_dbg_eigh2(const double *G, size_t n, double *band, double *d, double *e);
/* stage seconds of the last eigendecomposition that ran with GEMMA_HIP_EIGH_TIMING=1 in the environment: t8 = {reduction (to band /
 * to tridiagonal), bulge chase, divide & conquer, back-transformation Q2, Q1 (one-stage: all of it), sort + transpose, n, 1|2 stages} */
int gemma_hip_dbg_eigh_last(double *t8);
/* the U^T x stage of gemma_hip_lmm_batch alone (after lmm_setup; host pointers): UtX is l x n row-major, row s =
 * (U^T x_s)^T of the mean-imputed SNP s (the column fast_dgemm("T","N",U,Xlarge) produces, GEMMA src/lmm.cpp:1521).
 * path 0: fp64 MFMA GEMM; path 1: exact int8-digit product where the input allows it (PLINK 2-bit; fp64 rows of hard calls;
 * fp64 rows of fixed-point dosages k/100 or k/1000 -- csrc/i8gemm.hip.h), else the fp64 GEMM */
int gemma_hip_dbg_utx(int geno_kind, const void *geno, size_t l, size_t ld, int path, double *UtX);
/* what the last U^T x (lmm_batch*, dbg_utx) ran on: 0 fp64 MFMA GEMM (src/lmm.cpp:1521 as one fp64 product), 1 int8-digit
 * product of hard calls, 2 / 3 int8-digit product of fixed-point dosages k/100 / k/1000 (BIMBAM mean genotypes,
 * doc/manual.tex:398-404) */
int gemma_hip_dbg_last_utx_path(int *path);
/* the MATRIX KERNEL that product launched, as the library's own launch site recorded it (bench.py labels `roofline.kernel` from this
 * and refuses counter files taken on another kernel -- VERDICT r4 #1b).  `name` is the kernel's symbol as rocprofv3 prints it;
 * `launches` counts launches since the library was loaded. */
enum {
  GEMMA_UTX_KERNEL_DGEMM_F64 = 0,    /* dgemm_mfma_glds_kernel: src/lmm.cpp:1521 as one fp64 MFMA product */
  GEMMA_UTX_KERNEL_DENSE_I8 = 1,     /* i8gemm_packed_kernel_t<true>: digit products, mask product dense (GEMMA_HIP_I8_SPARSE=0) */
  GEMMA_UTX_KERNEL_SPARSE_BYTES = 2, /* i8gemm_sparse_kernel: mask product on the 2:4 sparse MFMA, byte genotypes (=1) */
  GEMMA_UTX_KERNEL_RECORDS_R32 = 3,  /* i8gemm_sparse2_kernel: records, 32-row matrix instructions (GEMMA_HIP_I8_ROWS=32) */
  GEMMA_UTX_KERNEL_RECORDS_R16 = 4,  /* i8gemm_sparse2_r16_kernel: records, v_mfma_i32_16x16x64_i8 + v_smfmac_i32_16x16x128_i8 (default) */
  GEMMA_UTX_KERNEL_DOSAGE_I8 = 5,    /* i8gemm_packed_kernel_t<false, true>: byte planes of fixed-point dosages, 32-row instructions (GEMMA_HIP_DOSAGE_ROWS=32) */
  GEMMA_UTX_KERNEL_DOSAGE_I8_R16 = 6, /* i8gemm_dense16_kernel_t<true>: the same planes on v_mfma_i32_16x16x64_i8 (default) */
  GEMMA_UTX_KERNEL_COUNT = 7
};
typedef struct {
  int variant;  /* GEMMA_UTX_KERNEL_* */
  int rows;     /* rows of the matrix instruction: 16 | 32 (0: fp64) */
  int digits;   /* base-256 digits of U in the product (0: fp64) */
  int fuse;     /* 1: two digits per int32 plane */
  int raster;   /* row blocks of the cross-XCD raster (0: per-XCD ranges) */
  long launches;
  char name[64];
} gemma_utx_kernel_info;
int gemma_hip_dbg_last_utx_kernel(gemma_utx_kernel_info *info);
/* Blocks WITHOUT a missing call (round 6).  With x = g + mean * m the mask product U^T (mean * m) is identically zero for them; the
 * records path notices on the device -- the kernel that builds the records sets a flag when it meets a missing call -- and the launch
 * site queues both forms of the 16-row kernel, of which the one that is not the block's returns at once: complete blocks take the
 * genotype product alone (i8gemm_sparse2_r16_g_kernel) and the digit combine reads no mask rows.  U^T x is the same, bit for bit (a
 * mask product of zeros adds +0.0); GEMMA_HIP_I8_COMPLETE=0 sends every block through both products.  *any: that flag for the last
 * records product of a plain batch (1 / 0; -1: form off or no such product yet).  Synchronises the device. */
int gemma_hip_dbg_last_block_missing(int *any);
/* rows of the last sparse int8 product's block whose mask operand dropped calls (groups of four with 3 - 4 missing calls keep two):
 * *short_rows = rows with 1 .. 16 of them (completed from a short per-row list), *long_rows = rows with more (fp64 fix-up pass);
 * -1 / -1 when no such product ran.  *epilogue = 1: the last int8 product wrote U^T x from the epilogue of its plane-0 launch
 * (i8gemm_sparse2_r16_ep_kernel / _ep_g_kernel: the default on the 16-row records kernel) and no digit combine ran; 0: every plane
 * went to memory and i8_combine_kernel read them back (GEMMA_HIP_I8_EPILOGUE=0, the other kernels, the two-block pipe); -1: none
 * yet.  Synchronises the device. */
int gemma_hip_dbg_last_i8_post(long *short_rows, long *long_rows, int *epilogue);
/* re-read the GEMMA_HIP_* switches of the batch path.  The library reads them once per setup (gemma_hip_init, lmm_setup*, lm_setup,
 * mvlmm_null / mvlmm_set, kin_begin), never per launch; a caller that changes one between two batches of ONE setup calls this. */
int gemma_hip_reload_env(void);
/* base-256 digits of U the int8 product uses at this n: 7 (U to 2^-56 of the column maximum); 6 from n = 16384 up
 * (U rounded to 2^-48 of the column maximum -- see gemma_hip_lmm_batch); GEMMA_HIP_I8_DIGITS=6|7 and GEMMA_HIP_I8_FORM=7g6m override */
int gemma_hip_dbg_i8_digits(size_t n, int *digits);

/* ---- variance components: -vc 1 (Haseman-Elston) and -vc 2 (REML, AI) ------------------------------------------------ */
/* Inverse of a symmetric positive-definite matrix in place, with its log determinant: the fast_inverse (LU, src/fastblas.cpp)
 * of UpdateParam, src/vc.cpp:168-258.  Blocked Cholesky (diagonal blocks in LDS, panels and trailing updates on the fp64 MFMA
 * GEMM), then U^-1 and U^-1 U^-T on the same GEMM.  The upper triangle of A is read; the full symmetric inverse is written.
 * Any n >= 1, lda >= n.  On the first pivot that is not > 0 the call returns GEMMA_HIP_ENOTPD, *bad_pivot = its 0-based index
 * (may be NULL) and computes nothing further; A is then partly overwritten.  Unlike the reference's LU, an indefinite matrix is an
 * error.  Device form: synchronises `stream` (it reads the pivot flag after every 128-row block). */
int gemma_hip_spd_inverse(double *A, size_t n, size_t lda, double *logdet, long *bad_pivot);
int gemma_hip_spd_inverse_d(double *A_d, size_t n, size_t lda, double *logdet, long *bad_pivot, void *stream);

/* The fit of class VC (src/vc.h) on n_vc <= 8 kinships, called where src/gemma.cpp:2378-2388 calls VC::CalcVChe /
 * VC::CalcVCreml.  K[l] (n x n, leading dimension ldk) are the kinships as the call site hands them over: read by ReadFile_kin /
 * ReadFile_mk and centred by CenterMatrix(G); v_traceG[l] is taken as the mean diagonal of K[l] (src/gemma.cpp:2341-2369).
 * W (n x n_cvt, n_cvt <= 64, with the intercept) and y (n) are host arrays.  vc_setup copies host kinships to the device;
 * vc_setup_d keeps the caller's device pointers (which must stay valid until vc_release); the fit runs on the null stream and
 * synchronises it, so work on other streams that writes the kinships must be complete first.  One fit state per process. */
int gemma_hip_vc_setup(size_t n, size_t n_vc, const double *const *K, size_t ldk, const double *W, size_t n_cvt, const double *y);
int gemma_hip_vc_setup_d(size_t n, size_t n_vc, const double *const *K_d, size_t ldk, const double *W, size_t n_cvt,
                         const double *y);
/* Results (caller-sized): sigma2[n_vc + 1], se_sigma2[n_vc + 1] (last = the residual component), pve[n_vc], se_pve[n_vc],
 * *pve_total, *se_pve_total.  -vc 1: VC::CalcVChe, src/vc.cpp:1503-1724. */
int gemma_hip_vc_he(double *sigma2, double *se_sigma2, double *pve, double *se_pve, double *pve_total, double *se_pve_total);
/* -vc 2: VC::CalcVCreml, src/vc.cpp:1726-1931.  Starts from the HE fit (log 0.1 for components <= 0), solves dev1 = 0 by Powell's
 * hybrid method with the AI matrix as Jacobian (GSL hybridsj restated, include/gemma_vc_hybrid.hpp) on log sigma2 (sigma2 with
 * noconstrain), until sum |dev1| < 1e-3 or 100 iterations; the Hessian inverse by LU on the host.  *iterations: solver
 * iterations; *status: 0 converged, 1 iteration limit, 2 / 3 no progress (GSL_ENOPROG / GSL_ENOPROGJ, where the reference's loop
 * breaks too).  counts[2] (may be NULL): device evaluations of (dev1, dev2) and SPD inverses of the fit (f, J and fdf at one
 * point share one evaluation).  iter_sigma2 (may be NULL): sigma2 of iteration 0 .. *iterations, (n_vc + 1) each, at most
 * iter_cap rows -- the reference's per-iteration "sigma2 = " lines.  With noconstrain, a step to where H is not positive
 * definite ends the fit with GEMMA_HIP_ENOTPD (the reference's LU inverse would carry on with an indefinite H). */
int gemma_hip_vc_reml(int noconstrain, double *sigma2, double *se_sigma2, double *pve, double *se_pve, double *pve_total,
                      double *se_pve_total, int *iterations, int *status, long *counts, double *iter_sigma2, size_t iter_cap);
/* seconds of the last REML fit's evaluations: {H assembly, SPD inverse, P correction, mat-vecs, traces} (HIP events) */
int gemma_hip_vc_timing(double *t5);
int gemma_hip_vc_release(void);

/* ---- genomic prediction: -bslmm 2 (ridge regression / BLUP) and -predict 1 / 2 -------------------------------------------- */
/* BSLMM::RidgeR (src/bslmm.cpp:1194-1221), called where src/gemma.cpp:2959-2960 calls it -- without the n x p matrix UtX the
 * reference allocates for it (src/gemma.cpp:2878, :2951).  With b = Uty / (lambda eval + 1):
 *   bv    = U (lambda eval o b)                          returned by ridge_setup (bv_out[n], may be NULL)
 *   alpha = (lambda / ns_test) UtX' b = (lambda / ns_test) X_c' r,   r = U b  (n numbers, formed by ridge_setup and kept on the device)
 * so the effects of a block of SNPs are one matrix-vector product on its packed rows (ridge_batch), in the centring of
 * ReadFile_bed / ReadFile_geno with a UtX argument (src/gemma_io.cpp:1956-2084, :1742-1845): mean over the analysed non-missing
 * calls, a missing call contributes 0.  ns_test = the number of analysed SNPs of the whole fit (UtX->size2).
 * Host form: U (n x n), eval, Uty, bv_out on the host.  _d: all four on the device (U with leading dimension ldu), on `stream`,
 * which is synchronised.  _kept: U and eval of the device-resident chain (eigh_kept_K / eigh_keep), Uty and bv_out on the host. */
int gemma_hip_ridge_setup(size_t n, const double *U, const double *eval, const double *Uty, double lambda, size_t ns_test,
                          double *bv_out);
int gemma_hip_ridge_setup_d(size_t n, const double *U_d, size_t ldu, const double *eval_d, const double *Uty_d, double lambda,
                            size_t ns_test, double *bv_out_d, void *stream);
int gemma_hip_ridge_setup_kept(const double *Uty, double lambda, size_t ns_test, double *bv_out);
/* The product alone: r[n] (host) is taken as it is and ridge_batch returns scale * X_c' r -- for callers that iterate on the
 * genotype product (and for its tests), in place of ridge_setup. */
int gemma_hip_ridge_set_r(size_t n, const double *r, double scale);
/* Rows of the blocks cover ni_total individuals of which the n with indicator_idv != 0 are analysed (cPar.indicator_idv); without
 * this call rows cover exactly the n analysed ones.  EINVAL when the indicator does not select n individuals. */
int gemma_hip_ridge_set_indicator(const int *indicator_idv, size_t ni_total);
/* alpha_out[l] for l SNP-major rows: GEMMA_GENO_PLINK_2BIT (ld bytes per row, >= ceil(ni_total / 4)) or
 * GEMMA_GENO_F64_SNP_MAJOR (ld doubles per row, NaN = missing).  A SNP without a non-missing analysed call gets 0 (every entry
 * of the reference's column is 0).  fp64 accumulation in an order fixed by the shapes alone: repeated calls agree bit for bit.
 * _d: geno and alpha_out on the device, asynchronous on `stream`.  Any l: a block of more rows than one launch takes is cut. */
int gemma_hip_ridge_batch(int geno_kind, const void *geno, size_t l, size_t ld, double *alpha_out);
int gemma_hip_ridge_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, double *alpha_out_d, void *stream);
int gemma_hip_ridge_finish(void);

/* The -predict block of src/gemma.cpp:1660-1729 on the device.  prdt_begin: indicator_idv over ni_total individuals, 1 = training
 * (phenotyped), 0 = to be predicted; y_prdt (one entry per 0, in order) starts at zero.
 * prdt_add = PRDT::AnalyzePlink / AnalyzeBimbam (src/prdt.cpp:310-444, :207-308; call site src/gemma.cpp:1705-1709) for l rows
 * over all ni_total individuals with their effect sizes effect[l] (the SNPs of mapRS2est only): x_train_mean over the non-missing
 * training calls, x_mean over the non-missing test calls, a missing test call counts x_mean - x_train_mean, every other
 * g - x_train_mean.  used_out[l] (may be NULL): 0 for a SNP missing in every test individual (skipped, the reference's "will be
 * ignored"), else 1.  A used SNP without a non-missing training call has x_train_mean = 0 / 0 and turns every prediction into
 * NaN, as in the reference.  The sum over SNPs is cut into partitions by l alone and combined in index order.
 * prdt_add_bv = PRDT::AddBV (src/prdt.cpp:133-205; call site src/gemma.cpp:1698): G (ni_total x ni_total, not changed) is centred
 * with the weighted CenterMatrix(G, w) (src/mathfunc.cpp:181-201, w = the indicator), y_prdt += G_fo G_oo^+ u_hat with the
 * eigenvalues of G_oo below 1e-10 zeroed; u_hat[n_bv] on the host, n_bv = the number of training individuals.
 * prdt_end: y_prdt += pheno_mean, probit != 0 (-predict 2): y_prdt = Phi(y_prdt) (src/gemma.cpp:1715-1722); copies the result to
 * the host and ends the state.  prdt_add_d is asynchronous on its stream; all adds of one prediction go to ONE stream (they
 * accumulate into the same y_prdt), and prdt_end synchronises the stream of the last add before it reads the sums.
 * Host forms of ridge_batch / prdt_add read only the leading ceil(ni_total / 4) bytes (or ni_total doubles) of each row of ld. */
int gemma_hip_prdt_begin(const int *indicator_idv, size_t ni_total);
int gemma_hip_prdt_add(int geno_kind, const void *geno, size_t l, size_t ld, const double *effect, int *used_out);
int gemma_hip_prdt_add_d(int geno_kind, const void *geno_d, size_t l, size_t ld, const double *effect_d, int *used_out_d, void *stream);
int gemma_hip_prdt_add_bv(const double *G, size_t ni_total, const double *u_hat, size_t n_bv);
int gemma_hip_prdt_add_bv_d(const double *G_d, size_t ni_total, size_t ldg, const double *u_hat, size_t n_bv, void *stream);
int gemma_hip_prdt_end(double pheno_mean, int probit, double *y_prdt);
/* -predict from a kinship alone (a_mode 43) for ONE phenotype: src/gemma.cpp:1732-1820 and :1873-1882 with PRDT::MvnormPrdt
 * (src/prdt.cpp:448-553).  ni individuals (those with covariates, indicator_cvt); G_full (ni x ni, as ReadFile_kin hands it over,
 * not centred, not changed); indicator_pheno[ni]: 1 = phenotype observed; W_full (ni x n_cvt, with the intercept); y_full[ni]
 * (entries of the unobserved individuals are not read).  The kinship of the observed individuals is centred and decomposed,
 * lambda is the REML estimate (CalcLambda 'R'), vg / ve / beta come from CalcLmmVgVeBeta, H = ve I + vg CenterMatrix(G_full) and
 *   y_miss = W_miss beta + H_mo H_oo^-1 (y_obs - W_obs beta)        y_miss[number of zeros of indicator_pheno], in order.
 * H_oo is inverted as a symmetric positive-definite matrix (GEMMA_HIP_ENOTPD where ve = 0 makes it singular; the reference's LU
 * would carry on).  fit3 (may be NULL) = {vg, ve, lambda}. */
int gemma_hip_prdt_kin(size_t ni, const double *G_full, const int *indicator_pheno, const double *W_full, size_t n_cvt,
                       const double *y_full, double l_min, double l_max, size_t n_region, double *y_miss, double *fit3);
/* The same for d = 2..GEMMA_MV_DMAX phenotypes: the else branch of src/gemma.cpp:1821-1871 with PRDT::MvnormPrdt, without the
 * (ni d)^2 matrix H_full = G (x) Vg + I (x) Ve.  Entries are ordered i * d + a (individual-major, as KroneckerSym and MvnormPrdt
 * order them): indicator_pheno (ni x d, 1 = observed), Y_full (ni x d, unobserved entries are not read), y_miss one value per zero
 * of indicator_pheno in that order.  With Gc = CenterMatrix(G_full), o the observed entries and r = (Y - W B^T)[o]:
 *   H_oo[(i,a),(j,b)] = Gc_ij Vg_ab + delta_ij Ve_ab  (assembled on the device),  z = H_oo^-1 r  (Cholesky factor and two
 *   triangular solves, no inverse),  y_miss_ia = (W B^T)_ia + (Gc Z Vg + Z Ve)_ia  with Z = z scattered over ni x d.
 * _apply: the system alone for given Vg, Ve (d x d, leading dimension d) and B (d x n_cvt, n_cvt <= GEMMA_MV_CMAX): no
 * eigensolver, no null fit.  _apply_d: G_full on the device (leading dimension ldg, not changed), on `stream`, which is
 * synchronised; every other argument on the host.
 * prdt_kin_mv: the whole block -- the kinship of the individuals with every phenotype is taken from G_full, centred and decomposed
 * on the device, U'W and U'Y, the REMLE fit of gemma_hip_mvlmm_null (opt NULL = the PARAM defaults; n_cvt + 1 <= GEMMA_MV_CMAX),
 * then _apply with its Vg_remle, Ve_remle, B_remle.  fit (may be NULL) receives that null fit.  d == 1 is handed to
 * gemma_hip_prdt_kin (fit: Vg_remle[0] = vg, Ve_remle[0] = ve, everything else 0).
 * GEMMA_HIP_EINVAL: a null pointer, d or n_cvt beyond the caps, no observed entry, no more individuals with every phenotype than
 * n_cvt + 1 (prdt_kin_mv), y_miss == NULL while something is missing, ni > 65535.  Nothing missing: GEMMA_HIP_OK (prdt_kin_mv
 * still returns the fit).  GEMMA_HIP_ENOTPD, with the failing pivot in the message, when H_oo is not positive definite. */
int gemma_hip_prdt_kin_mv_apply(size_t ni, size_t d, const double *G_full, const int *indicator_pheno, const double *W_full,
                                size_t n_cvt, const double *Y_full, const double *Vg, const double *Ve, const double *B, double *y_miss);
int gemma_hip_prdt_kin_mv_apply_d(size_t ni, size_t d, const double *G_full_d, size_t ldg, const int *indicator_pheno,
                                  const double *W_full, size_t n_cvt, const double *Y_full, const double *Vg, const double *Ve,
                                  const double *B, double *y_miss, void *stream);
int gemma_hip_prdt_kin_mv(size_t ni, size_t d, const double *G_full, const int *indicator_pheno, const double *W_full, size_t n_cvt,
                          const double *Y_full, double l_min, double l_max, size_t n_region, const gemma_mvlmm_opt *opt, double *y_miss,
                          gemma_mvlmm_null *fit);

/* ---- MQS summary-statistic variance components: -gs and -vc 1 -beta (Zhou 2017) ---------------------------------------------- */
/* PARAM::CalcS (src/param.cpp:1717-1812), called where src/gemma.cpp:1977 (-gs) and :2166 / :2198 (-vc 1 / 2 with -beta) call it.
 * A session computes the weighted, covariate-residualised, category-partitioned kinships of PlinkKin / BimbamKinUncentered with
 * weights (src/gemma_io.cpp:2947-3170, :2753-2945) over the ANALYSED individuals, then CenterMatrix + ScaleMatrix per category
 * (src/mathfunc.cpp:147-177, :271-286), compAKtoS (src/param.cpp:1325-1378) and JackknifeAKtoS (:1596-1713).
 * mqs_begin: indicator_idv over ni_total individuals (NULL: all analysed; n = the number of non-zero entries), n_vc in 1..8
 * categories, W (n x n_cvt on the host, n_cvt in 1..64, with the intercept; (W^T W)^-1 is formed on the host, EINVAL when
 * singular).  slot 0 starts over, fills K and makes A = K (CalcS with an empty mapRS2wA); slot 1 needs the finished K of a slot 0
 * session with the same ni_total, n and n_vc, keeps it and fills A (the second CalcS of src/gemma.cpp:2198).  slot 2 is slot 1 with
 * A starting from the kept, centred + scaled K instead of 0: the reference's PlinkKin adds to the matrix it is handed, and its second
 * CalcS hands it the A of the first, so this is the A that -vc 2 -beta of the reference computes.
 * mqs_add: l SNP-major rows (GEMMA_GENO_PLINK_2BIT, ld bytes per row; GEMMA_GENO_F64_SNP_MAJOR, ld doubles per row, NaN = missing)
 * of the SNPs with indicator_snp != 0, cat[l] = mapRS2cat of each SNP (0 when n_vc == 1; < 0: the SNP is in no category or has no
 * weight and is skipped; >= n_vc: EINVAL, nothing of the block is accumulated), weight[l] = mapRS2weight (NULL: 1).  Per SNP: mean
 * over the called genotypes, impute, centre, x <- x - W (W^T W)^-1 W^T x, var = x^T x / n of that residual; var == 0 (and a SNP
 * without any called genotype, which poisons the reference's matrix with NaN) drops the SNP, otherwise x sqrt(w / var) joins the
 * panel of its category and K_c += X_c X_c^T on the fp64 matrix units.  _d: geno, cat and weight on the device, on `stream`, which
 * is synchronised once per block (the per-category counts come back to the host).
 * mqs_end: K_c /= ns_c (a category without SNPs stays the zero matrix: its rows and columns of S and Svar are 0, where the
 * reference divides 0 by 0), centre, scale; ns[n_vc] (may be NULL) = ns_c; S (2 n_vc x n_vc, row-major, may be NULL) = S on top of
 * Svar, as prefix.S.txt.  A slot 1 session centres and scales A only.
 * mqs_get: the centred + scaled matrix i_vc of slot 0 (K) or 1 (A; K when A = K), n x n, to the host.
 * mqs_S / mqs_S_d: S and Svar alone from given centred + scaled matrices: matrix i of A (K) is n x n at A + i n ld with leading
 * dimension ld; A == K is allowed and halves the work.  The jackknife is evaluated in its exact O(n^2 n_vc^2) form (DESIGN.md
 * section 13), Svar as the variance around the mean of the n leave-one-out values; with n_cvt == 1 S is the bias-corrected
 * n d - (n - 1) mean, as in the reference.  All sums run in a fixed order: repeated calls agree bit for bit.
 * mqs_release returns all device memory of the state. */
int gemma_hip_mqs_begin(size_t ni_total, const int *indicator_idv, size_t n_vc, const double *W, size_t n_cvt, int slot);
int gemma_hip_mqs_add(int geno_kind, const void *geno, size_t l, size_t ld, const int *cat, const double *weight);
int gemma_hip_mqs_add_d(int geno_kind, const void *geno_d, size_t l, size_t ld, const int *cat_d, const double *weight_d, void *stream);
int gemma_hip_mqs_end(double *S, double *ns);
int gemma_hip_mqs_get(int slot, size_t i_vc, double *out);
int gemma_hip_mqs_S(size_t n, size_t n_vc, const double *A, const double *K, size_t ld, size_t n_cvt, double *S);
int gemma_hip_mqs_S_d(size_t n, size_t n_vc, const double *A_d, const double *K_d, size_t ld, size_t n_cvt, double *S, void *stream);
int gemma_hip_mqs_release(void);

/* ---- MQS confidence intervals: -ci 1 / -ci 2 (a_mode 66 / 67), the two genotype passes under CalcCIss ------------------------------ */
/* In place of PlinkXwz / BimbamXwz (src/vc.cpp:2314-2437, :2225-2312) and PlinkXtXwz / BimbamXtXwz (:2568-2688, :2480-2566), called
 * where src/gemma.cpp:2400-2554 calls them.  Over the n analysed individuals a SNP has mu = mean of its called genotypes,
 * var = (sum g^2 + mu^2 n_miss) / n - mu^2 and x_i = g_i - mu (0 where missing); there is no covariate residual here.
 * ci_begin: indicator_idv over ni_total individuals (NULL: all analysed), n_vc in 1..8 categories.
 * ci_xwz (pass 1, block by block): l SNP-major rows (GEMMA_GENO_PLINK_2BIT, ld bytes per row; GEMMA_GENO_F64_SNP_MAJOR, ld doubles
 * per row, NaN = missing) of the analysed SNPs in file order, cat[l] in 0 .. n_vc - 1 (anything else: EINVAL, nothing of the block
 * is accumulated), z[l], w[l] (NULL: 1, -ci 1).  One pass over the block accumulates Xz[i][c] += z / sqrt(var) x_i and
 * XWz[i][c] += w z / sqrt(var) x_i for c = cat of the SNP.  A SNP without a called genotype or with var == 0 among the analysed
 * individuals contributes nothing and is counted in *n_skipped (may be NULL; of this block; always on the host): the reference
 * divides by 0 there.  _d: geno, cat, z and w on the device, on `stream`, which is synchronised once per block.
 * ci_xwz_end: ends pass 1; Xz, XWz (n x n_vc, row-major, either may be NULL) to the host; XWz stays on the device for pass 2.
 * ci_xtxwz (pass 2, block by block): XtXWz[s][j] = (sum_i x_si XWz[i][j]) / sqrt(var_s), l x n_vc row-major; the row of a skipped
 * SNP is 0.  _d: geno and XtXWz on the device, asynchronous on `stream`.
 * The 2-bit route runs both passes on v_mfma_f64_16x16x4_f64 from the packed calls; the fp64 route centres the rows and uses the
 * fp64 GEMM.  All sums run in an order fixed by the shapes: repeated sessions agree bit for bit.  Calls out of order (anything
 * before ci_begin, ci_xtxwz before ci_xwz_end, ci_xwz after it) return GEMMA_HIP_EINVAL and leave the state as it was.
 * ci_release returns all device memory of the state (as does gemma_hip_shutdown). */
int gemma_hip_ci_begin(size_t ni_total, const int *indicator_idv, size_t n_vc);
int gemma_hip_ci_xwz(int geno_kind, const void *geno, size_t l, size_t ld, const int *cat, const double *z, const double *w,
                     size_t *n_skipped);
int gemma_hip_ci_xwz_d(int geno_kind, const void *geno_d, size_t l, size_t ld, const int *cat_d, const double *z_d, const double *w_d,
                       size_t *n_skipped, void *stream);
int gemma_hip_ci_xwz_end(double *Xz, double *XWz);
int gemma_hip_ci_xtxwz(int geno_kind, const void *geno, size_t l, size_t ld, double *XtXWz);
int gemma_hip_ci_xtxwz_d(int geno_kind, const void *geno_d, size_t l, size_t ld, double *XtXWz_d, void *stream);
int gemma_hip_ci_release(void);

/* ---- Windowed SNP correlation: -calccor (a_mode 71), the prefix.cor.txt that -cor reads back -------------------------------------- */
/* VARCOV::AnalyzePlink / AnalyzeBimbam (src/varcov.cpp:249-446) with Calc_Cor (:220-238), called where src/gemma.cpp:2046-2059 calls
 * them.  With c the called mask, g the genotype and mu = sum g / sum c over the ANALYSED individuals, the column of a SNP is
 * x = c (g - mu) (Plink_ReadOneSNP / Bimbam_ReadOneSNP, src/gemma_io.cpp:1069-1184, and the centring at src/varcov.cpp:308 / :408);
 * var_t = x_t.x_t / n and cor_{t,k} = x_t.x_{t+k} / sqrt((x_t.x_t)(x_{t+k}.x_{t+k})) for k = 1 .. n_nb[t], counting analysed SNPs.
 * cor_begin (replaces the set-up of src/varcov.cpp:257-276 / :357-376): indicator_idv over ni_total individuals (NULL: all
 * analysed); n = the number of non-zero entries.
 * cor_block (replaces the loop over t with its sliding X_mat, src/varcov.cpp:281-332 / :381-432): geno holds l_in >= l_out
 * consecutive analysed SNPs (indicator_snp != 0) as they lie in the file (GEMMA_GENO_PLINK_2BIT, ld bytes per row;
 * GEMMA_GENO_F64_SNP_MAJOR, ld doubles per row, NaN = missing); rows l_out .. l_in - 1 are the halo the windows of the first l_out
 * reach into.  n_nb[l_out] = CalcNB's window sizes (src/varcov.cpp:168-217); var[l_out]; cor[sum n_nb], the windows one after the
 * other: cor_{t,k} at (sum_{u < t} n_nb[u]) + k - 1 (may be NULL when every window is empty).  EINVAL when some t + n_nb[t] >= l_in,
 * when n_nb[t] < 0, or before cor_begin.  The window of SNP t is exactly n_nb[t]: leftover rows of the reference's sliding buffer
 *  are not reproduced.
 * PLINK rows take the exact integer route: four int8 products per pair on the matrix units, combined in int64 before the one
 * division and square root (n <= 2^20 analysed individuals; EINVAL above); the result does not depend on how the SNPs are cut into
 * blocks.  fp64 rows take the fp64 matrix units.  A SNP without a called genotype gives NaN (var and every cor with it), a
 * monomorphic one var = 0 and NaN correlations, as the reference's 0 / 0 does.  No atomics: two runs agree bit for bit.
 * _d: geno, n_nb, var and cor on the device, on `stream`, which is synchronised once per block (the windows come to the host).
 * cor_release (replaces the frees of src/varcov.cpp:340-345 / :440-445) returns all device memory of the state. */
int gemma_hip_cor_begin(size_t ni_total, const int *indicator_idv);
int gemma_hip_cor_block(int geno_kind, const void *geno, size_t l_in, size_t ld, size_t l_out, const int *n_nb, double *var,
                        double *cor);
int gemma_hip_cor_block_d(int geno_kind, const void *geno_d, size_t l_in, size_t ld, size_t l_out, const int *n_nb_d, double *var_d,
                          double *cor_d, void *stream);
int gemma_hip_cor_release(void);

#ifdef __cplusplus
}
#endif
#endif /* GEMMA_HIP_H */

// C ABI of the MI355X kinship + univariate-LMM path (see include/gemma_hip.h).
// Host-side glue only: device memory, streams, launches, staging copies.  This unit holds NO kernel: it includes the declaration
// half (X.h) of every kernel header and dgemm.h; the kernels are compiled in utx_i8_kernels.hip, firstpass_kernels.hip,
// lmm_kernels.hip, dgemm_tu.hip, the mvlmm_kernels*.hip and the feature units (tests/test_build_units.py holds it to that).
// mvlmm.hip.h (MvArgs and device templates nobody instantiates here) and comm.hip.h (host code) define no kernel either.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gemma_hip.h"
#include "tu_common.h"
#include "dgemm.h"
#include "eigh_tu.h"
#include "vc_tu.h"
#include "prdt_tu.h"
#include "mqs_tu.h"
#include "cor_tu.h"
#include "ingest.h"
#include "lm_assoc.h"
#include "lmm_assoc.h"
#include "lmm_grid.h"
#include "lmm_score_panel.h"
#include "lmm_null_panel.h"
#include "lmm_pair.h"
#include "i8gemm.h"
#include "i8gemm_sparse.h"
#include "i8gemm_sparse2.h"
#include "i8gemm_sparse2_r16.h"
#include "plink_records.h"
#include "i8gemm_dense16.h"
#include "qc.h"
#include "mvlmm.hip.h"
#include "mvlmm_pair.h"
#include "comm.hip.h"
#include "kin_i8.h"
#include "i8_plan.h"

using namespace gemma_hip;

namespace {

struct StageProf {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  double acc_ms = 0.0;
  long launches = 0;
};

// Environment switches of the batch path.  Read ONCE per setup -- gemma_hip_init, every lmm_setup* / lm_setup / mvlmm_set,
// kin_begin and gemma_hip_reload_env -- never on a launch path (a getenv per launch walks the whole environment block under
// libc's lock; round 4 had three of them on every records-kernel launch).  Tests and bench legs that flip a switch between
// two batches of one setup call gemma_hip_reload_env().
struct Knobs {
  I8Switches i8;           // the switches the form of the int8 U^T x depends on (i8_plan.h)
  int i8_digits = 0;       // GEMMA_HIP_I8_DIGITS: 6 | 7 forces the digit count (0: by n)
  int i8_scale_max = 1;    // GEMMA_HIP_I8_SCALE: "pow2" = columns of U scaled by a power of two (rounds 1-5); default: by their exact maximum
  int dosage_i8 = 1;       // GEMMA_HIP_UTX_DOSAGE_I8
  int dosage_rows = 16;    // GEMMA_HIP_DOSAGE_ROWS: 32 = the dosage planes on the 32-row dense kernel (rounds 3-4)
  int table_v2 = 1;        // GEMMA_HIP_TABLE_V2
  int table_pf = 0;        // GEMMA_HIP_TABLE_PF
  int multi_table = 1;     // GEMMA_HIP_MULTI_TABLE: 0 = gemma_hip_lmm_multi_batch computes every phenotype's fixed-lambda table on its own
  int force_generic = 0;   // GEMMA_HIP_FORCE_GENERIC
  int assoc_variant = 44;  // GEMMA_HIP_ASSOC_VARIANT
  int mvlmm_rt = 0;        // GEMMA_HIP_MVLMM_RT
  int pipe_cus = 64;       // GEMMA_HIP_PIPE_CUS: CUs of the post partition of gemma_hip_lmm_batch_pipe_d (0: two plain streams, no masks)
  int kin_i8 = 1, kin_upper = 1, kin_lists = 1, kin_lists_oom = 0; // GEMMA_HIP_KIN_I8 / _UPPER / _LISTS / _LISTS_OOM
  long long kin_list_cap = 0;                                       // GEMMA_HIP_KIN_LIST_CAP (0: by block size)
  // the tables of the per-SNP stage (make_grid / make_cheb): the setup that builds them has loaded these in lmm_common_setup
  int assoc_grid = 1;         // GEMMA_HIP_ASSOC_GRID: 0 = no fixed-lambda table
  int assoc_cheb = 1;         // GEMMA_HIP_ASSOC_CHEB: 0 = no bracket-interval series
  int cheb_lowlambda = 1;     // GEMMA_HIP_CHEB_LOWLAMBDA: 0 = the intervals below lambda = 1e-3 stream (round 2)
  int assoc_final_series = 1; // GEMMA_HIP_ASSOC_FINAL_SERIES: 0 = the final likelihood at lambda-hat streams the SNP's row (round 2)
  static int geti(const char *name, int dflt) {
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
  }
  static int on_unless_0(const char *name) { // by the first character, as every switch of this kind always was
    const char *e = getenv(name);
    return (e && e[0] == '0') ? 0 : 1;
  }
  static int off_unless_1(const char *name) {
    const char *e = getenv(name);
    return (e && e[0] == '1') ? 1 : 0;
  }
  void load() {
    i8.utx_i8 = geti("GEMMA_HIP_UTX_I8", 1);
    const int dg = geti("GEMMA_HIP_I8_DIGITS", 0);
    i8_digits = (dg == 6 || dg == 7) ? dg : 0;
    const char *es = getenv("GEMMA_HIP_I8_SPARSE");
    i8.sparse = (es && es[0] >= '0' && es[0] <= '2') ? es[0] - '0' : 2;
    i8.fuse = on_unless_0("GEMMA_HIP_I8_FUSE");
    i8.gm = geti("GEMMA_HIP_I8_GM", 0);
    i8.raster = geti("GEMMA_HIP_I8_RASTER", S2_DEFAULT_RASTER);
    i8.rows = geti("GEMMA_HIP_I8_ROWS", 16) == 32 ? 32 : 16;
    const char *esc = getenv("GEMMA_HIP_I8_SCALE");
    i8_scale_max = (esc && strcmp(esc, "pow2") == 0) ? 0 : 1;
    const char *efm = getenv("GEMMA_HIP_I8_FORM");
    i8.mdrop = (efm && strcmp(efm, "7g6m") == 0) ? 1 : 0;
    if (i8.mdrop) i8_digits = 7;
    i8.complete = on_unless_0("GEMMA_HIP_I8_COMPLETE");
    i8.epilogue = on_unless_0("GEMMA_HIP_I8_EPILOGUE");
    i8.epi_depth = geti("GEMMA_HIP_I8_EPI_DEPTH", 4) <= 1 ? 1 : 4;
    i8.direct = on_unless_0("GEMMA_HIP_I8_DIRECT");
    dosage_i8 = on_unless_0("GEMMA_HIP_UTX_DOSAGE_I8");
    dosage_rows = geti("GEMMA_HIP_DOSAGE_ROWS", 16) == 32 ? 32 : 16;
    i8.overlap = off_unless_1("GEMMA_HIP_OVERLAP");
    i8.chunks = geti("GEMMA_HIP_OVERLAP_CHUNKS", 4);
    table_v2 = on_unless_0("GEMMA_HIP_TABLE_V2");
    table_pf = off_unless_1("GEMMA_HIP_TABLE_PF");
    multi_table = on_unless_0("GEMMA_HIP_MULTI_TABLE");
    force_generic = off_unless_1("GEMMA_HIP_FORCE_GENERIC");
    assoc_variant = geti("GEMMA_HIP_ASSOC_VARIANT", 44);
    mvlmm_rt = off_unless_1("GEMMA_HIP_MVLMM_RT");
    pipe_cus = geti("GEMMA_HIP_PIPE_CUS", 64);
    kin_i8 = on_unless_0("GEMMA_HIP_KIN_I8");
    kin_upper = on_unless_0("GEMMA_HIP_KIN_UPPER");
    kin_lists = on_unless_0("GEMMA_HIP_KIN_LISTS");
    kin_lists_oom = off_unless_1("GEMMA_HIP_KIN_LISTS_OOM");
    const char *kc = getenv("GEMMA_HIP_KIN_LIST_CAP");
    kin_list_cap = (kc && *kc) ? atoll(kc) : 0;
    assoc_grid = on_unless_0("GEMMA_HIP_ASSOC_GRID");
    assoc_cheb = on_unless_0("GEMMA_HIP_ASSOC_CHEB");
    cheb_lowlambda = on_unless_0("GEMMA_HIP_CHEB_LOWLAMBDA");
    assoc_final_series = on_unless_0("GEMMA_HIP_ASSOC_FINAL_SERIES");
  }
};

struct Ctx {
  bool inited = false;
  Knobs knobs;
  int device = -1;
  int verbose = 0;
  std::string last_error;
  hipDeviceProp_t prop;
  bool profiling = false;
  StageProf prof[GEMMA_STAGE_COUNT];

  // kinship state
  bool kin_active = false;
  size_t kin_n = 0;
  int kin_mode = 1;
  size_t kin_ns = 0;
  DevBuf kin_K, kin_X, kin_stage;
  // gemma_hip_kin_add (host blocks): the upload of block k + 1 runs on its own stream beside the kernels of block k (round 6); it
  // waits for the ingest of block k -- the only reader of the staging buffer -- and the null stream waits for the upload
  hipStream_t kin_copy = nullptr;
  hipEvent_t kin_copied = nullptr, kin_ingested = nullptr;
  bool kin_ingested_valid = false, kin_host_call = false;
  DevBuf qc_G, qc_M, qc_W, qc_O; // gemma_hip_snp_qc: block, index map, W^T, statistics -- kept between the calls of a first pass (round 6:
                                 // four hipMalloc + hipFree per 100 MB block were a fifth of the pass), released by kin_begin / shutdown
  // exact-integer path of the centred kinship of hard calls (kin_i8.hip.h)
  bool kin_i8 = false, kin_i8_used = false;
  DevBuf i8_meta, i8_rowsur; // sparse mask operand: the words of the packed block, dropped calls per row
  DevBuf U_even;            // odd n: U copied to an even leading dimension for the fp64 GEMM's aligned path
  const double *U_even_of = nullptr; // the U that copy was made from
  DevBuf kin_GtG, kin_S, kin_a, kin_At, kin_Gt;
  DevBuf kin_A2, kin_cnt, kin_off, kin_listS, kin_listJ, kin_sub, kin_cj, kin_flag; // lists of the missing calls of a block
  DevBuf kin_tmap;                    // tiles of G^T G that meet the upper triangle
  // lmm_batch_d on PLINK blocks in row chunks: the digit combine and the per-SNP stage of chunk c on a side stream beside the
  // int8 product of chunk c + 1 (overlap_*)
  hipStream_t ov_stream = nullptr;
  hipEvent_t ov_ready[16] = {}, ov_done = nullptr;
  // gemma_hip_lmm_batch_pipe_d: the product of block i + 1 on one CU partition beside the combine + per-SNP stage of block i on the
  // other (xp_*).  What both stages of a block touch exists twice (A / C / mean / rowsur alternate between the live members of
  // this struct and `shadow`); what only one stream touches exists once.
  struct XPipe {
    hipStream_t P = nullptr, Q = nullptr;
    hipEvent_t in_ready = nullptr, prod_done[2] = {}, post_done[2] = {};
    hipEvent_t ingest_done = nullptr; // recorded on P behind the ingest of the last block handed in (the caller's stream waits for it)
    bool ingest_valid = false;
    bool post_valid[2] = {false, false};
    unsigned long long count = 0;
    bool pending = false;
    int cus = -1; // partition the streams were made for
    DevBuf shadow_A, shadow_C, shadow_mean, shadow_rowsur;
  } xp;
  int kin_tmap_tm = 0, kin_tmap_tn = 0, kin_tmap_count = 0;

  // lmm state
  bool lmm_active = false;
  gemma_lmm_cfg cfg;
  const double *U = nullptr, *eval = nullptr; // device
  DevBuf own_U, own_eval, own_Uty, own_UtW, UtWt, idx_map;
  size_t ni_total = 0; // PLINK rows cover this many individuals (0 = n)
  bool have_map = false;
  DevBuf X, UtX, stage_in, stage_out;
  DevBuf grid_T; // fixed-lambda table of the batch (lmm_grid.hip.h); its setup half is the phenotype's (PhenoSlot)
  DevBuf cheb_T, cheb_slots, cheb_list, cheb_count, cheb_D, cheb_Ck, cheb_Gk, cheb_Lk, cheb_iv, cheb_dends, cheb_res; // bracket-interval series
  DevBuf table_P; // K-slice partial sums of the table products (table_v2_kernel)
  DevBuf gxe_env, gxe_UtWt, gxe_Z, gxe_UtZ, gxe_flip; // GXE variants
  bool gxe_ready = false;
  double gxe_lnbeta = 0.0;
  DevBuf mv_Yt, mv_out; // multivariate LMM: U^T Y transposed (d x n)
  DevBuf mv_scratch;    // Newton-Raphson tables of the run-time kernel, one slab per workgroup
  bool mv_ready = false, mv_gxe = false;
  size_t mv_d = 0;
  MvArgs mv_proto;
  struct MvLast {
    int form = 0, d = 0, rows = 0;
  } mv_last[2]; // the kernel of the last per-SNP launch [0] / the last d-variate null fit [1] (gemma_hip_dbg_last_mvlmm_kernel)
  DevBuf i8_Bt, i8_q, i8_qinv, i8_cmax, i8_A, i8_C, i8_mean; // exact int8-digit U^T x (i8gemm.hip.h)
  // (tile_m, tile_n) per workgroup of the records kernel: the cross-XCD raster (i8gemm_sparse2.hip.h).  One map per launch shape,
  // each in its OWN buffer, built once (a block cut into row chunks has two shapes -- full chunks and the last one -- and
  // a single slot was rebuilt, with a stream synchronisation and a blocking copy, twice per batch; a map in use by a kernel on
  // another stream could be overwritten).  The host copy stays alive for the asynchronous upload.
  struct RasterSlot {
    DevBuf dev;
    std::vector<int2> host;
    int tm = 0, tn = 0, rb = 0, xcds = 8;
    unsigned long long used = 0;
  } i8_raster[6];
  unsigned long long i8_raster_clock = 0;
  DevBuf i8_surlist;           // per row: count + up to SUR_MAX individuals the sparse mask operand dropped
  DevBuf i8_colsum;            // column sums of U from its digit planes (fixed-point dosage path)
  bool i8_colsum_ready = false;
  int last_utx_path = 0;       // what the last U^T x took: 0 fp64 GEMM, 1 int8 hard calls, 2 int8 dosages k/100, 3 int8 dosages k/1000
  gemma_utx_kernel_info last_utx_kernel = {}; // the matrix kernel that product launched (gemma_hip_dbg_last_utx_kernel)
  int i8_last_epi = -1;                       // 1 / 0: the last int8 product wrote U^T x from the records kernel's epilogue / left it to the digit combine
  long i8_rowsur_n = 0;                       // rows (padded) of the last records product: the per-row counts of dropped calls in i8_rowsur
  long i8_flag_at = -1;                       // int index of the any-missing flag of the last records product in i8_rowsur (-1: none)
  bool i8_ready = false;
  size_t i8_ldk = 0, i8_npad = 0;
  int i8_digits = I8_DIGITS;
  // What of a setup belongs to the PHENOTYPE lives in a PhenoSlot and nowhere else: `single` for a single-phenotype setup (and the
  // setup-wide proto of lmm_common_setup for every family), slots[t] for phenotype t of gemma_hip_lmm_multi_setup.  What builds or
  // runs the per-SNP stage takes its slot as a parameter.  Everything else of the setup (U and its digit planes, eval, UtWt, idx_map,
  // cheb_iv / cheb_D / cheb_Ck..Lk, the per-batch buffers) exists once.
  struct PhenoSlot {
    AssocArgs proto;               // with its own l_mle_null / logl_mle_H0 and the pointers into this slot's tables
    const double *Uty = nullptr;
    DevBuf grid_R, grid_F, cheb_R, cheb_F; // the setup half of the fixed-lambda table and of the bracket-interval series
    DevBuf carry;                  // PLINK NaN rule: the carry chain of this phenotype, in block order
    GridGeom grid_geom, cheb_geom;
    double cheb_mid[ASSOC_MAX_REGION], cheb_inv_half[ASSOC_MAX_REGION];
    unsigned long long cheb_qmask = 0; // bit k: tabulated interval k is in Q form (ends at or below lambda = 1e-3)
    int carry_flip = 0;
    void release() { // a buffer added above is released here and nowhere else
      grid_R.release(); grid_F.release(); cheb_R.release(); cheb_F.release(); carry.release();
      Uty = nullptr;
    }
  };
  PhenoSlot single;                // the phenotype of a single-phenotype setup
  std::vector<PhenoSlot> slots;    // multi setup: the T phenotypes (`single` then holds the setup-wide proto alone)
  size_t multi_T = 0;              // 0: single-phenotype setup
  DevBuf multi_Yt;                 // U^T Y transposed (T x n): slot t's Uty is row t
  DevBuf multi_R, multi_T_buf;     // shared table: a group's weight matrix (one per group, back to back) and its G tables
  int multi_G = 0;                 // phenotypes per pass of the shared table product (0: no shared table for this setup)
  // score panel (gemma_hip_lmm_score_panel_setup): -lmm 3 of score_T phenotypes from one product per block (lmm_score_panel.hip.h)
  size_t score_T = 0;              // 0: no score-panel setup
  ScoreGeom score_geom;
  DevBuf score_R, score_Pyy, score_Yt, score_lam, score_bad; // weight matrix, P_yy and lambda per phenotype; U^T Y transposed (setup only)
  // the hits form: the pre-filter's threshold on F (one double, valid for score_fthr_p of this setup), the per-wave best cells,
  // and the host form's device-side list, counter and best
  DevBuf score_fthr, score_cells, score_hits, score_cnt, score_best;
  double score_fthr_p = -1.0;      // p_max the threshold was made for (-1: none)
  hipStream_t score_fthr_s = nullptr; // ... and the stream it was made on (another stream makes its own: no order between the two)
  // the refinement of a score panel's hit pairs (gemma_hip_lmm_score_panel_refine_*): Wald / LRT of (SNP, phenotype) pairs, lmm_pair.hip.h
  bool refine_ready = false;       // gemma_hip_lmm_score_panel_refine_setup done for this score-panel setup
  DevBuf refine_Yt, refine_logl;   // its own T x n transposed U^T Y; logl_mle_H0 per phenotype (l_mle_null is score_lam)
  DevBuf refine_out;               // the host form's records
  AssocArgs refine_proto;          // a_mode 4, BIMBAM NaN rule, the cfg's grid, no tables
  const double *last_UtX = nullptr; // the U^T x of the most recent score-panel block (nullptr: none, or overwritten since: compute_utx)
  size_t last_l = 0, last_ldx = 0;

  // linear model (-lm) state
  bool lm_active = false;
  LmArgs lm_proto;
  DevBuf lm_Wt, lm_y, lm_small;

  // misc scratch
  DevBuf scratch;

  // pipelined host-block path (lmm_batch_submit / _collect): two pinned staging slots, a copy and a compute stream
  struct PipeSlot {
    void *pin_in = nullptr, *pin_out = nullptr;
    size_t pin_in_cap = 0, pin_out_cap = 0;
    DevBuf dev_in, dev_out;
    hipEvent_t h2d = nullptr, done = nullptr;
    size_t l = 0;
    bool busy = false;
  } pipe[2];
  hipStream_t pipe_copy = nullptr, pipe_comp = nullptr;
  int pipe_head = 0, pipe_count = 0; // oldest busy slot, number in flight

  // device-resident chain (kin_end_keep -> eigh_kept_K -> lmm_setup_kept) and the communicator
  DevBuf kept_K, kept_UE; // K: ni_total^2; UE: U (n^2) followed by eval (n) -- one buffer, one broadcast
  size_t kept_K_n = 0, kept_n = 0;
  double kept_trace = 0.0;
  Comm comm;
} g_ctx;

int fail(int code, const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_ctx.last_error = buf;
  if (g_ctx.verbose) fprintf(stderr, "gemma_hip: %s\n", buf);
  return code;
}

// the tail of an entry point around a feature unit: the unit's code, its message into last_error
int ret(int rc, const std::string &msg) { return rc ? fail(rc, "%s", msg.c_str()) : GEMMA_HIP_OK; }

#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(GEMMA_HIP_ERUNTIME, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                                      \
  } while (0)

#define NEED_INIT()                                                                              \
  do {                                                                                           \
    if (!g_ctx.inited) {                                                                         \
      int rc_ = gemma_hip_init(-1, 0);                                                           \
      if (rc_ != GEMMA_HIP_OK) return rc_;                                                       \
    }                                                                                            \
  } while (0)

struct ProfScope {
  int stage;
  hipStream_t s;
  hipEvent_t a = nullptr, b = nullptr;
  ProfScope(int st, hipStream_t stream) : stage(st), s(stream) {
    if (g_ctx.profiling) {
      if (hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess)
        (void)hipEventRecord(a, s);
      else
        a = b = nullptr;
    }
  }
  ~ProfScope() {
    if (a && b) {
      (void)hipEventRecord(b, s);
      g_ctx.prof[stage].ev.emplace_back(a, b);
    }
  }
};

int prof_collect(int stage) {
  StageProf &p = g_ctx.prof[stage];
  for (auto &pr : p.ev) {
    (void)hipEventSynchronize(pr.second);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
      p.acc_ms += ms;
      p.launches += 1;
    }
    (void)hipEventDestroy(pr.first);
    (void)hipEventDestroy(pr.second);
  }
  p.ev.clear();
  return GEMMA_HIP_OK;
}

inline hipStream_t S(void *s) { return reinterpret_cast<hipStream_t>(s); }

} // namespace

static void pipe_release(); // pipelined host-block path, defined with lmm_batch_submit
static void xp_release();   // two-block product / post pipeline, defined with lmm_batch_pipe_d
static int xp_flush_fwd(hipStream_t s);
static void raster_release() {
  for (auto &r : g_ctx.i8_raster) {
    r.dev.release();
    r.host.clear();
    r.tm = r.tn = r.rb = 0;
    r.used = 0;
  }
}
// the buffers gemma_hip_snp_qc keeps between the blocks of a first pass: a failed block, kin_begin and shutdown
static void qc_release() { g_ctx.qc_G.release(); g_ctx.qc_M.release(); g_ctx.qc_W.release(); g_ctx.qc_O.release(); }
static void kin_i8_release(); // integer kinship path, defined with kin_begin
// one release list per state, each beside the entry points that fill it: kinship (abi_kinship.inc.h), LMM (abi_lmm_stage.inc.h), -lm
// (abi_gxe_lm.inc.h).  A member added to Ctx is released by adding it to its state's list and nowhere else.
static void kin_release();
static void lmm_release();
static void lm_release();

// ------------------------------------------------------------------------------ lifetime
extern "C" int gemma_hip_abi_version(void) { return GEMMA_HIP_ABI_VERSION; }

extern "C" const char *gemma_hip_strerror(int code) {
  switch (code) {
  case GEMMA_HIP_OK: return "ok";
  case GEMMA_HIP_EINVAL: return "invalid argument (range error)";
  case GEMMA_HIP_ENODEV: return "no usable gfx950 device";
  case GEMMA_HIP_ENOMEM: return "device memory allocation failed";
  case GEMMA_HIP_ERUNTIME: return "HIP runtime error";
  case GEMMA_HIP_ESTATE: return "call sequence violated";
  case GEMMA_HIP_ENOCONV: return "eigensolver did not converge";
  case GEMMA_HIP_ENOTPD: return "matrix not positive definite";
  default: return "unknown error";
  }
}

extern "C" const char *gemma_hip_last_error(void) { return g_ctx.last_error.c_str(); }

extern "C" int gemma_hip_init(int device, int verbose) {
  g_ctx.verbose = verbose;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    (void)hipGetLastError();
    return fail(GEMMA_HIP_ENODEV, "no HIP device visible (this library has no CPU fallback)");
  }
  if (device >= 0) {
    if (device >= ndev) return fail(GEMMA_HIP_ENODEV, "device %d out of range (%d visible)", device, ndev);
    HIPCHK(hipSetDevice(device));
  }
  int cur = 0;
  HIPCHK(hipGetDevice(&cur));
  HIPCHK(hipGetDeviceProperties(&g_ctx.prop, cur));
  if (strncmp(g_ctx.prop.gcnArchName, "gfx950", 6) != 0)
    return fail(GEMMA_HIP_ENODEV, "device %d is %s; this build targets gfx950 only", cur,
                g_ctx.prop.gcnArchName);
  g_ctx.device = cur;
  g_ctx.inited = true;
  g_ctx.knobs.load();
  gemm_aux_init();
  if (verbose)
    fprintf(stderr, "gemma_hip: device %d %s (%s), %d CUs, %.1f GB\n", cur, g_ctx.prop.name,
            g_ctx.prop.gcnArchName, g_ctx.prop.multiProcessorCount,
            (double)g_ctx.prop.totalGlobalMem / 1e9);
  return GEMMA_HIP_OK;
}

extern "C" void gemma_hip_shutdown(void) {
  if (!g_ctx.inited) return;
  (void)hipDeviceSynchronize();
  for (int s = 0; s < GEMMA_STAGE_COUNT; ++s) prof_collect(s);
  kin_release();
  qc_release();
  lmm_release(); // every buffer an LMM setup or batch owns: ONE list, beside the members' users (abi_lmm_stage.inc.h)
  lm_release();
  pipe_release(); // pinned slots, copy stream and events of the pipelined host-block path
  xp_release();
  if (g_ctx.ov_stream) {
    (void)hipStreamDestroy(g_ctx.ov_stream);
    for (auto &e : g_ctx.ov_ready)
      if (e) (void)hipEventDestroy(e);
    if (g_ctx.ov_done) (void)hipEventDestroy(g_ctx.ov_done);
    g_ctx.ov_stream = nullptr;
    for (auto &e : g_ctx.ov_ready) e = nullptr;
    g_ctx.ov_done = nullptr;
  }
  if (g_ctx.kin_copy) {
    (void)hipStreamDestroy(g_ctx.kin_copy);
    if (g_ctx.kin_copied) (void)hipEventDestroy(g_ctx.kin_copied);
    if (g_ctx.kin_ingested) (void)hipEventDestroy(g_ctx.kin_ingested);
    g_ctx.kin_copy = nullptr;
    g_ctx.kin_copied = g_ctx.kin_ingested = nullptr;
    g_ctx.kin_ingested_valid = false;
  }
  g_ctx.kept_K.release(); g_ctx.kept_UE.release();
  g_ctx.kept_K_n = g_ctx.kept_n = 0;
  g_ctx.comm.finalize();
  gemm_aux_destroy();
  eigh_tu_shutdown();
  vc_tu_shutdown();
  prdt_tu_shutdown();
  mqs_tu_shutdown();
  cor_tu_shutdown();
  g_ctx.inited = false;
}

extern "C" int gemma_hip_device_info(char *name, size_t len, int *n_cu, size_t *hbm_bytes) {
  NEED_INIT();
  if (name && len) {
    snprintf(name, len, "%s (%s)", g_ctx.prop.name, g_ctx.prop.gcnArchName);
  }
  if (n_cu) *n_cu = g_ctx.prop.multiProcessorCount;
  if (hbm_bytes) *hbm_bytes = g_ctx.prop.totalGlobalMem;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_profile_enable(int on) {
  g_ctx.profiling = (on != 0);
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_profile_read(int stage, double *total_ms, long *launches, int reset) {
  NEED_INIT();
  if (stage < 0 || stage >= GEMMA_STAGE_COUNT) return fail(GEMMA_HIP_EINVAL, "bad stage %d", stage);
  prof_collect(stage);
  if (total_ms) *total_ms = g_ctx.prof[stage].acc_ms;
  if (launches) *launches = g_ctx.prof[stage].launches;
  if (reset) {
    g_ctx.prof[stage].acc_ms = 0.0;
    g_ctx.prof[stage].launches = 0;
  }
  return GEMMA_HIP_OK;
}

// ------------------------------------------------------------------------------ GEMM
static int check_gemm(char ta, char tb, size_t M, size_t N, size_t K, size_t lda, size_t ldb,
                      size_t ldc) {
  const bool tA = (ta == 'T' || ta == 't'), tB = (tb == 'T' || tb == 't');
  if (!tA && ta != 'N' && ta != 'n') return fail(GEMMA_HIP_EINVAL, "dgemm: bad TransA '%c'", ta);
  if (!tB && tb != 'N' && tb != 'n') return fail(GEMMA_HIP_EINVAL, "dgemm: bad TransB '%c'", tb);
  const size_t a_cols = tA ? M : K, b_cols = tB ? K : N;
  if (lda < a_cols || ldb < b_cols || ldc < N)
    return fail(GEMMA_HIP_EINVAL, "Range error in dgemm (lda=%zu ldb=%zu ldc=%zu for M=%zu N=%zu K=%zu)",
                lda, ldb, ldc, M, N, K);
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_dgemm_d(char ta, char tb, size_t M, size_t N, size_t K, double alpha,
                                 const double *A, size_t lda, const double *B, size_t ldb,
                                 double beta, double *C, size_t ldc, void *stream) {
  NEED_INIT();
  int rc = check_gemm(ta, tb, M, N, K, lda, ldb, ldc);
  if (rc) return rc;
  if (M == 0 || N == 0) return GEMMA_HIP_OK;
  ProfScope ps(GEMMA_STAGE_UTX_GEMM, S(stream));
  HIPCHK(launch_dgemm(ta, tb, (long)M, (long)N, (long)K, alpha, A, (long)lda, B, (long)ldb, beta, C,
                      (long)ldc, false, false, S(stream)));
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_dgemm(char ta, char tb, size_t M, size_t N, size_t K, double alpha,
                               const double *A, size_t lda, const double *B, size_t ldb,
                               double beta, double *C, size_t ldc) {
  NEED_INIT();
  int rc = check_gemm(ta, tb, M, N, K, lda, ldb, ldc);
  if (rc) return rc;
  if (M == 0 || N == 0) return GEMMA_HIP_OK;
  const bool tA = (ta == 'T' || ta == 't'), tB = (tb == 'T' || tb == 't');
  const size_t a_rows = tA ? K : M, b_rows = tB ? N : K;
  const size_t a_bytes = a_rows * lda * 8, b_bytes = b_rows * ldb * 8, c_bytes = M * ldc * 8;
  ScopedBuf dA, dB, dC;
  if (dA.reserve(a_bytes ? a_bytes : 8) || dB.reserve(b_bytes ? b_bytes : 8) || dC.reserve(c_bytes))
    return fail(GEMMA_HIP_ENOMEM, "dgemm: cannot allocate %zu bytes", a_bytes + b_bytes + c_bytes);
  // the last row of a strided host view may be shorter than ld: copy row-wise via 2D copies
  auto h2d = [&](void *d, const double *h, size_t rows, size_t cols, size_t ld) -> hipError_t {
    if (rows == 0 || cols == 0) return hipSuccess;
    return hipMemcpy2D(d, ld * 8, h, ld * 8, cols * 8, rows, hipMemcpyHostToDevice);
  };
  HIPCHK(h2d(dA.p, A, a_rows, tA ? M : K, lda));
  HIPCHK(h2d(dB.p, B, b_rows, tB ? K : N, ldb));
  if (beta != 0.0) HIPCHK(h2d(dC.p, C, M, N, ldc));
  HIPCHK(launch_dgemm(ta, tb, (long)M, (long)N, (long)K, alpha, dA.as<double>(), (long)lda, dB.as<double>(), (long)ldb, beta,
                      dC.as<double>(), (long)ldc, false, false, 0));
  HIPCHK(hipMemcpy2D(C, ldc * 8, dC.p, ldc * 8, N * 8, M, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

// The stages of the C ABI, one file each: textual parts of THIS translation unit -- they share g_ctx and the helpers above, and
// together they compile in about three seconds now that no kernel is generated here, so separately compiled parts would buy nothing.
// abi_host_block.inc.h comes first: the geometry / argument check of a genotype block and the staging of a host block, which every
// block entry point of the parts below goes through.
#include "abi_host_block.inc.h"
#include "abi_kinship.inc.h"
#include "abi_eigen_qc.inc.h"
#include "abi_lmm_stage.inc.h"
#include "abi_utx.inc.h"
#include "abi_lmm_batch.inc.h"
#include "abi_gxe_lm.inc.h"
#include "abi_mvlmm.inc.h"
#include "abi_kept_comm.inc.h"
#include "abi_lmm_multi.inc.h"
#include "abi_lmm_score_panel.inc.h"
#include "abi_lmm_score_refine.inc.h"
#include "abi_lmm_null_panel.inc.h"
#include "abi_mvlmm_pairs.inc.h"
#include "abi_vc.inc.h"
#include "abi_prdt.inc.h"
#include "abi_mqs.inc.h"
#include "abi_cor.inc.h"

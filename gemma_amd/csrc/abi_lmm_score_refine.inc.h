// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace).
// This part: the refinement of a score panel's hits (gemma_hip_lmm_score_panel_refine_* / _hits_refine_batch): each pair's own
// lambda-hats, the Wald test and the likelihood-ratio test -- the `-lmm 4` record of (SNP, phenotype) -- from one launch over the
// list, one wavefront per pair (lmm_pair.hip.h).
//
// A fourth, optional piece of the score-panel state: gemma_hip_lmm_score_panel_refine_setup keeps a T x n transposed U^T Y of its own
// (the score-panel setup still lets its copy go) and the T logl_mle_H0; l_mle_null is the setup's (score_lam), the grid the cfg's.
// score_release (abi_lmm_stage.inc.h) takes it down with the rest.  The U^T x of the most recent score-panel block is remembered
// (last_UtX: set at the end of a batch, dropped by compute_utx and every other writer of g_ctx.UtX) for refine_last_d.

static_assert(sizeof(gemma_score_hit) == sizeof(ScoreHit), "PairArgs reads gemma_score_hit entries");
static_assert(sizeof(gemma_sumstat) == sizeof(SumStat), "the pair kernels write gemma_sumstat records");

#define NEED_REFINE(who)                                                                                                        \
  do {                                                                                                                          \
    NEED_SCORE(who);                                                                                                            \
    if (!g_ctx.refine_ready) return fail(GEMMA_HIP_ESTATE, who " before gemma_hip_lmm_score_panel_refine_setup");                \
  } while (0)

// UtY_d: n x T row-major on the device; logl: T values on the host.  Synchronises s: logl is the caller's, the ends are locals.
static int refine_setup_dev(const double *UtY_d, const double *logl, hipStream_t s) {
  const size_t n = g_ctx.cfg.n, T = g_ctx.score_T;
  g_ctx.refine_ready = false;
  if (T > (size_t)-1 / 8 / n || g_ctx.refine_Yt.reserve(T * n * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_refine_setup: the %zu x %zu copy of U^T Y does not fit (%zu bytes)", T, n, T * n * 8);
  if (g_ctx.refine_logl.reserve(T * 8) || g_ctx.scratch.reserve(16))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_refine_setup: per-phenotype constants (%zu bytes)", T * 8 + 16);
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, UtY_d, (long)n,
                     (long)T, (long)T, g_ctx.refine_Yt.as<double>(), (long)n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(g_ctx.refine_logl.p, logl, T * 8, hipMemcpyHostToDevice, s));
  // log|H| at l_min and l_max as the single-phenotype setup has them (make_utwt): the records are that launch's in every bit
  hipLaunchKernelGGL(logdet_ends_kernel, dim3(1), dim3(64), 0, s, g_ctx.eval, (int)n, g_ctx.cfg.l_min, g_ctx.cfg.l_max,
                     g_ctx.scratch.as<double>());
  HIPCHK(hipGetLastError());
  double ends[2];
  HIPCHK(hipMemcpyAsync(ends, g_ctx.scratch.p, 16, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  AssocArgs &a = g_ctx.refine_proto;
  a = g_ctx.single.proto; // n, the grid and ln B(df / 2, 1 / 2) of the cfg (lmm_common_setup); no table, no series
  a.a_mode = 4;
  a.plink_nan_rule = 0;
  a.l_mle_null = a.logl_mle_H0 = 0.0; // per pair: PairArgs
  a.have_grid = a.have_cheb = 0;
  a.grid_T = a.grid_F = nullptr;
  a.cheb_T = a.cheb_F = nullptr; a.cheb_slots = nullptr; a.cheb_res = nullptr;
  a.logdet_lmin = ends[0];
  a.logdet_lmax = ends[1];
  a.have_logdet_ends = 1;
  g_ctx.refine_ready = true;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_score_panel_refine_setup_d(const double *UtY_d, const double *logl_mle_H0, void *stream) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_refine_setup");
  if (!UtY_d || !logl_mle_H0) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_refine_setup: null pointer");
  return refine_setup_dev(UtY_d, logl_mle_H0, S(stream));
}

extern "C" int gemma_hip_lmm_score_panel_refine_setup(const double *UtY, const double *logl_mle_H0) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_refine_setup");
  if (!UtY || !logl_mle_H0) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_refine_setup: null pointer");
  const size_t n = g_ctx.cfg.n, T = g_ctx.score_T;
  g_ctx.refine_ready = false;
  if (T > (size_t)-1 / 8 / n || g_ctx.own_Uty.reserve(n * T * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_refine_setup: U^T Y does not fit (%zu bytes)", n * T * 8);
  HIPCHK(hipMemcpy(g_ctx.own_Uty.p, UtY, n * T * 8, hipMemcpyHostToDevice));
  const int rc = refine_setup_dev(g_ctx.own_Uty.as<double>(), logl_mle_H0, nullptr);
  g_ctx.own_Uty.release(); // the upload; refine_setup_dev has synchronised
  return rc;
}

// the records of m pairs on the l rows of UtX -> out_d[i]
static int launch_pairs(const char *who, const double *UtX, size_t l, size_t ld, const gemma_score_hit *pairs_d, size_t m,
                        gemma_sumstat *out_d, hipStream_t s) {
  const size_t nwg = (m + PR_WAVES - 1) / PR_WAVES;
  if (nwg > 0x7fffffffUL) return fail(GEMMA_HIP_EINVAL, "%s: %zu pairs in one list", who, m);
  AssocArgs a = g_ctx.refine_proto;
  a.UtX = UtX;
  a.ld = (long)ld;
  a.l = (long)l;
  a.eval = g_ctx.eval;
  a.UtWt = g_ctx.UtWt.as<double>();
  a.out = reinterpret_cast<SumStat *>(out_d);
  PairArgs p;
  p.pairs = reinterpret_cast<const ScoreHit *>(pairs_d);
  p.m = (long)m;
  p.Yt = g_ctx.refine_Yt.as<double>();
  p.l_mle_null = g_ctx.score_lam.as<double>();
  p.logl_mle_H0 = g_ctx.refine_logl.as<double>();
  p.T = (int)g_ctx.score_T;
  const dim3 grid((unsigned)nwg), block(64 * PR_WAVES);
  ProfScope ps(GEMMA_STAGE_ASSOC, s);
  // the families and template arguments of launch_assoc's defaults; GEMMA_HIP_FORCE_GENERIC=1 as there
  const size_t c = g_ctx.cfg.n_cvt;
  switch (g_ctx.knobs.force_generic ? (size_t)99 : c) {
  case 1: hipLaunchKernelGGL((lmm_pair_kernel<1, 4, 4>), grid, block, 0, s, a, p); break;
  case 2: hipLaunchKernelGGL((lmm_pair_kernel<2, 2, 2>), grid, block, 0, s, a, p); break;
  case 3: hipLaunchKernelGGL((lmm_pair_kernel<3, 2, 1>), grid, block, 0, s, a, p); break;
  case 4: hipLaunchKernelGGL((lmm_pair_kernel<4, 2, 1>), grid, block, 0, s, a, p); break;
  default: hipLaunchKernelGGL(lmm_pair_generic_kernel, grid, block, 0, s, a, (int)c, p); break; // c <= SP_CMAX = GEN_CMAX
  }
  HIPCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_score_panel_refine_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, const gemma_score_hit *pairs_d,
                                                        size_t m, gemma_sumstat *out_d, void *stream) {
  NEED_INIT();
  NEED_REFINE("lmm_score_panel_refine_assoc");
  if (m == 0) return GEMMA_HIP_OK;
  if (!UtX_d || !pairs_d || !out_d) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_refine_assoc: null pointer");
  if (ld_utx < g_ctx.cfg.n) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_refine_assoc: ld_utx=%zu < n=%zu", ld_utx, g_ctx.cfg.n);
  if (int rc = xp_flush_fwd(S(stream))) return rc;
  return launch_pairs("lmm_score_panel_refine_assoc", UtX_d, l, ld_utx, pairs_d, m, out_d, S(stream));
}

extern "C" int gemma_hip_lmm_score_panel_refine_last_d(const gemma_score_hit *pairs_d, size_t m, gemma_sumstat *out_d, void *stream) {
  NEED_INIT();
  NEED_REFINE("lmm_score_panel_refine_last");
  if (!g_ctx.last_UtX)
    return fail(GEMMA_HIP_ESTATE, "lmm_score_panel_refine_last: no score-panel block since the setup, or its U^T x has been overwritten");
  if (m == 0) return GEMMA_HIP_OK;
  if (!pairs_d || !out_d) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_refine_last: null pointer");
  return launch_pairs("lmm_score_panel_refine_last", g_ctx.last_UtX, g_ctx.last_l, g_ctx.last_ldx, pairs_d, m, out_d, S(stream));
}

extern "C" int gemma_hip_lmm_score_panel_hits_refine_batch(int kind, const void *geno, size_t l, size_t ld, double p_max,
                                                           gemma_score_hit *hits, size_t cap, unsigned long long *n_hits,
                                                           gemma_score_best *best, gemma_sumstat *refined) {
  NEED_INIT();
  NEED_REFINE("lmm_score_panel_hits_refine_batch");
  if (!refined && cap) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_hits_refine_batch: null records for a list of %zu entries", cap);
  int rc = gemma_hip_lmm_score_panel_hits_batch(kind, geno, l, ld, p_max, hits, cap, n_hits, best);
  if (rc) return rc;
  const size_t kept = *n_hits < cap ? (size_t)*n_hits : cap;
  if (!kept) return GEMMA_HIP_OK;
  for (size_t i = 0; i < kept; ++i)
    if (hits[i].snp >= l || hits[i].pheno >= g_ctx.score_T)
      return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_hits_refine_batch: pair %zu (snp %u, pheno %u) is out of range", i, hits[i].snp,
                  hits[i].pheno);
  if (g_ctx.refine_out.reserve(kept * sizeof(gemma_sumstat)))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_hits_refine_batch: %zu records (%zu bytes)", kept, kept * sizeof(gemma_sumstat));
  // the list as the caller sees it (sorted): refined[i] belongs to hits[i]; score_hits holds cap entries (hits_batch)
  HIPCHK(hipMemcpy(g_ctx.score_hits.p, hits, kept * sizeof(gemma_score_hit), hipMemcpyHostToDevice));
  if ((rc = gemma_hip_lmm_score_panel_refine_last_d(g_ctx.score_hits.as<gemma_score_hit>(), kept, g_ctx.refine_out.as<gemma_sumstat>(), nullptr)))
    return rc;
  HIPCHK(hipMemcpy(refined, g_ctx.refine_out.p, kept * sizeof(gemma_sumstat), hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

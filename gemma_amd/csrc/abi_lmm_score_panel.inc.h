// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace).
// This part: the score panel (gemma_hip_lmm_score_panel_*): `-lmm 3` of T phenotypes over one U^T x, T in the thousands.
//
// The third LMM state beside the single-phenotype and the multi setup.  A setup builds, per phenotype, the c + 2 weight columns of
// the closed form of CalcRLScore at the phenotype's null lambda (score_setup_kernel, lmm_score_panel.hip.h) -- n (c + 2) doubles
// per phenotype, no lambda-search tables -- and a block is compute_utx as every batch entry point runs it followed by ONE product
// kernel with the statistics in its epilogue (score_panel_kernel).
// The three setups are score_setup: lmm_bind (abi_lmm_stage.inc.h) for U, eval, UtW and U^T Y, then score_setup_dev; the host forms
// of a block stage it with host_batch / stage_block (abi_host_block.inc.h).

static int score_check(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null) {
  if (!cfg) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: null cfg");
  if (cfg->a_mode != 3)
    return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: a_mode %d (the score panel is a_mode 3; the other modes search lambda per SNP: "
                                  "gemma_hip_lmm_multi_setup)", cfg->a_mode);
  if (cfg->n_cvt < 1 || cfg->n_cvt > (size_t)SP_CMAX)
    return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: n_cvt=%zu covariates (1..%d)", cfg->n_cvt, SP_CMAX);
  if (T == 0 || T > (size_t)INT_MAX - 64) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: T=%zu phenotypes", T);
  if (!l_mle_null) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: l_mle_null of every phenotype is needed");
  return GEMMA_HIP_OK;
}
// After lmm_bind: g_ctx.U / g_ctx.eval in place.  UtW_d: n x c, UtY_d: n x T row-major, both on the device;
// l_mle_null: T values on the host.
static int score_setup_dev(size_t T, const double *l_mle_null, const double *UtW_d, const double *UtY_d, hipStream_t s) {
  const size_t n = g_ctx.cfg.n, c = g_ctx.cfg.n_cvt;
  ScoreGeom g;
  g.n = (int)n; g.nc = (int)((n + 15) / 16);
  g.c = (int)c; g.nk = (int)c + 2;
  g.T = (int)T; g.ng = (int)((T + 15) / 16);
  const size_t r_bytes = (size_t)g.nc * (size_t)g.ng * (size_t)g.nk * 256 * 8;
  if (g_ctx.score_R.reserve(r_bytes))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_setup: the weight matrix of %zu phenotypes does not fit (%zu bytes)", T, r_bytes);
  if (g_ctx.score_Yt.reserve(T * n * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_setup: U^T Y does not fit beside the weight matrix (%zu bytes)", T * n * 8);
  if (g_ctx.UtWt.reserve(c * n * 8) || g_ctx.score_Pyy.reserve(T * 8) || g_ctx.score_lam.reserve(T * 8) || g_ctx.score_bad.reserve(4))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_setup: per-phenotype constants (%zu bytes)", c * n * 8 + 2 * T * 8 + 4);
  g_ctx.score_fthr_p = -1.0; // the hits form's threshold belongs to a setup's df
  g_ctx.score_T = T; // from here on a failure leaves a score state that lmm_common_setup / the caller's score_release takes down
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((c + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, UtW_d, (long)n,
                     (long)c, (long)c, g_ctx.UtWt.as<double>(), (long)n);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, UtY_d, (long)n,
                     (long)T, (long)T, g_ctx.score_Yt.as<double>(), (long)n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemsetAsync(g_ctx.score_R.p, 0, r_bytes, s));
  HIPCHK(hipMemsetAsync(g_ctx.score_bad.p, 0x7f, 4, s)); // above every phenotype index
  HIPCHK(hipMemcpyAsync(g_ctx.score_lam.p, l_mle_null, T * 8, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(score_setup_kernel, dim3((unsigned)T), dim3(256), 0, s, g, g_ctx.eval, g_ctx.UtWt.as<double>(),
                     g_ctx.score_Yt.as<double>(), g_ctx.score_lam.as<double>(), g_ctx.score_R.as<double>(),
                     g_ctx.score_Pyy.as<double>(), g_ctx.score_bad.as<int>());
  HIPCHK(hipGetLastError());
  int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, g_ctx.score_bad.p, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s)); // l_mle_null and `bad` are the caller's / a local
  g_ctx.score_Yt.release();
  if (bad >= 0 && (size_t)bad < T)
    return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: phenotype %d: UtW^T H UtW at l_mle_null = %g is not positive definite "
                                  "(collinear covariates or a non-finite lambda)", bad, l_mle_null[bad]);
  g_ctx.score_geom = g;
  return GEMMA_HIP_OK;
}

// the three score-panel setups after their argument checks (lmm_bind: a failed setup leaves lmm_active false) -- and no score
// state behind.  score_setup_dev has synchronised its stream: the uploaded U^T Y, read by the setup kernel only, goes at once.
static int score_setup(const char *who, SetupSrc src, const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *U,
                       const double *eval, const double *UtW, const double *UtY, hipStream_t s) {
  const double *UtW_d, *UtY_d;
  int rc = lmm_bind(who, src, cfg, U, eval, UtW, UtY, T, &UtW_d, &UtY_d);
  if (rc) return rc;
  if ((rc = score_setup_dev(T, l_mle_null, UtW_d, UtY_d, s))) {
    score_release();
    return rc;
  }
  if (src != SetupSrc::Device) g_ctx.own_Uty.release();
  g_ctx.lmm_active = true;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_score_panel_setup_d(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *U_d,
                                                 const double *eval_d, const double *UtW_d, const double *UtY_d, void *stream) {
  NEED_INIT();
  if (int rc = score_check(cfg, T, l_mle_null)) return rc; // the shape first: T = 0 has no U^T Y to point to
  if (!U_d || !eval_d || !UtW_d || !UtY_d) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: null pointer");
  return score_setup("lmm_score_panel_setup", SetupSrc::Device, cfg, T, l_mle_null, U_d, eval_d, UtW_d, UtY_d, S(stream));
}

extern "C" int gemma_hip_lmm_score_panel_setup(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *U,
                                               const double *eval, const double *UtW, const double *UtY) {
  NEED_INIT();
  if (int rc = score_check(cfg, T, l_mle_null)) return rc; // the shape first: T = 0 has no U^T Y to point to
  if (!U || !eval || !UtW || !UtY) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup: null pointer");
  return score_setup("lmm_score_panel_setup", SetupSrc::Host, cfg, T, l_mle_null, U, eval, UtW, UtY, nullptr);
}

extern "C" int gemma_hip_lmm_score_panel_setup_kept(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *UtW,
                                                    const double *UtY) {
  NEED_INIT();
  if (!g_ctx.kept_n) return fail(GEMMA_HIP_ESTATE, "lmm_score_panel_setup_kept: no kept U");
  if (int rc = score_check(cfg, T, l_mle_null)) return rc; // the shape first: T = 0 has no U^T Y to point to
  if (!UtW || !UtY) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup_kept: null pointer");
  if (cfg->n != g_ctx.kept_n)
    return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_setup_kept: cfg.n=%zu, kept U is %zu", cfg->n, g_ctx.kept_n);
  return score_setup("lmm_score_panel_setup_kept", SetupSrc::Kept, cfg, T, l_mle_null, nullptr, nullptr, UtW, UtY, nullptr);
}

// the product + statistics of the l rows of UtX -> out_d[t * l + s]
static int launch_score_panel(const double *UtX, size_t l, size_t ld, gemma_score_rec *out_d, hipStream_t s) {
  const ScoreGeom &g = g_ctx.score_geom;
  ScoreArgs a;
  a.UtX = UtX; a.ld = (long)ld; a.l = (long)l; a.g = g;
  a.Rp = g_ctx.score_R.as<double>();
  a.Pyy = g_ctx.score_Pyy.as<double>();
  a.out = reinterpret_cast<ScoreRec *>(out_d);
  a.lnbeta_half_df = g_ctx.single.proto.lnbeta_half_df;
  const size_t npt = ((size_t)g.ng + 2 * SP_PG - 1) / (2 * SP_PG), nst = (l + 32 * SP_RG - 1) / (32 * SP_RG);
  if (npt * nst > 0x7fffffffUL) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_batch: %zu x %zu tiles in one block", nst, npt);
  ProfScope ps(GEMMA_STAGE_ASSOC, s);
  const bool al = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(UtX) & 15) == 0; // 16-byte loads of the row fragments
  if (al) hipLaunchKernelGGL(score_panel_kernel<true>, dim3((unsigned)(npt * nst)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL(score_panel_kernel<false>, dim3((unsigned)(npt * nst)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

// the block whose U^T x stays in g_ctx.UtX behind a batch: gemma_hip_lmm_score_panel_refine_last_d (abi_lmm_score_refine.inc.h)
static void score_remember(const double *UtX, size_t l, size_t ldx) {
  g_ctx.last_UtX = UtX;
  g_ctx.last_l = l;
  g_ctx.last_ldx = ldx;
}

#define NEED_SCORE(who)                                                                                                        \
  do {                                                                                                                         \
    if (!g_ctx.lmm_active || !g_ctx.score_T) return fail(GEMMA_HIP_ESTATE, who " before gemma_hip_lmm_score_panel_setup");      \
  } while (0)

extern "C" int gemma_hip_lmm_score_panel_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, gemma_score_rec *out_d, void *stream) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_assoc");
  if (l == 0) return GEMMA_HIP_OK;
  if (!UtX_d || !out_d || ld_utx < g_ctx.cfg.n) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_assoc: bad UtX/ld");
  {
    int rcf = xp_flush_fwd(S(stream));
    if (rcf) return rcf;
  }
  return launch_score_panel(UtX_d, l, ld_utx, out_d, S(stream));
}

extern "C" int gemma_hip_lmm_score_panel_batch_d(int kind, const void *geno, size_t l, size_t ld, gemma_score_rec *out_d, void *stream) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_batch");
  if (l == 0) return GEMMA_HIP_OK;
  int rc = block_geom("lmm_score_panel_batch", kind, g_ctx.cfg.n, true, geno, l, ld, out_d);
  if (rc) return rc;
  hipStream_t s = S(stream);
  double *UtX;
  size_t ldx;
  if ((rc = compute_utx(kind, geno, l, ld, -1, &UtX, &ldx, s))) return rc;
  if ((rc = launch_score_panel(UtX, l, ldx, out_d, s))) return rc;
  score_remember(UtX, l, ldx);
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_score_panel_batch(int kind, const void *geno, size_t l, size_t ld, gemma_score_rec *out) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_batch");
  if (l == 0) return GEMMA_HIP_OK;
  return host_batch("lmm_score_panel_batch", kind, geno, l, ld, g_ctx.stage_out, out, g_ctx.score_T * l * sizeof(gemma_score_rec),
                    [&](const void *in_d, void *out_d) {
                      return gemma_hip_lmm_score_panel_batch_d(kind, in_d, l, ld, static_cast<gemma_score_rec *>(out_d), nullptr);
                    });
}

// ---- the hits form: pairs with p_score <= p_max, the best pair per phenotype (lmm_score_panel.hip.h) ----
static int score_hits_check(const char *who, size_t l, double p_max, const void *hits, size_t cap, const void *n_hits) {
  if (!(p_max >= 0.0 && p_max <= 1.0)) return fail(GEMMA_HIP_EINVAL, "%s: p_max=%g is not in [0, 1]", who, p_max);
  if (!n_hits) return fail(GEMMA_HIP_EINVAL, "%s: n_hits is needed", who);
  if (!hits && cap) return fail(GEMMA_HIP_EINVAL, "%s: a null list of %zu entries (count only: cap = 0)", who, cap);
  if (l > 0xffffffffUL) return fail(GEMMA_HIP_EINVAL, "%s: l=%zu rows (snp is 32 bits)", who, l);
  return GEMMA_HIP_OK;
}

// the block's counter to zero and, for l == 0, the best of an empty block
static int score_hits_empty(unsigned long long *n_hits_d, gemma_score_best *best_d, hipStream_t s) {
  HIPCHK(hipMemsetAsync(n_hits_d, 0, sizeof(unsigned long long), s));
  if (best_d) {
    const ScoreGeom &g = g_ctx.score_geom;
    hipLaunchKernelGGL(score_best_kernel, dim3((unsigned)((g.T + 255) / 256)), dim3(256), 0, s, g, 0L, (const ScoreCell *)nullptr,
                       g_ctx.score_Pyy.as<double>(), g_ctx.single.proto.lnbeta_half_df, reinterpret_cast<ScoreBest *>(best_d));
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

static int launch_score_hits(const double *UtX, size_t l, size_t ld, double p_max, gemma_score_hit *hits_d, size_t cap,
                             unsigned long long *n_hits_d, gemma_score_best *best_d, hipStream_t s) {
  const ScoreGeom &g = g_ctx.score_geom;
  const size_t npt = ((size_t)g.ng + 2 * SP_PG - 1) / (2 * SP_PG), nst = (l + 32 * SP_RG - 1) / (32 * SP_RG);
  if (npt * nst > 0x7fffffffUL) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_hits: %zu x %zu tiles in one block", nst, npt);
  const size_t ntile = (l + 31) / 32;
  if (g_ctx.score_fthr.reserve(8)) return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_hits: 8 bytes");
  if (best_d && g_ctx.score_cells.reserve(ntile * (size_t)g.T * sizeof(ScoreCell)))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_hits: the per-wave best of %zu row tiles x %d phenotypes (%zu bytes)", ntile, g.T,
                ntile * (size_t)g.T * sizeof(ScoreCell));
  const double lnb = g_ctx.single.proto.lnbeta_half_df;
  if (g_ctx.score_fthr_p != p_max || g_ctx.score_fthr_s != s) { // once per (setup, p_max, stream)
    hipLaunchKernelGGL(score_fcrit_kernel, dim3(1), dim3(64), 0, s, p_max, (double)(g.n - g.c - 1), lnb, g_ctx.score_fthr.as<double>());
    HIPCHK(hipGetLastError());
    g_ctx.score_fthr_p = p_max;
    g_ctx.score_fthr_s = s;
  }
  HIPCHK(hipMemsetAsync(n_hits_d, 0, sizeof(unsigned long long), s));
  ScoreArgs a;
  a.UtX = UtX; a.ld = (long)ld; a.l = (long)l; a.g = g;
  a.Rp = g_ctx.score_R.as<double>();
  a.Pyy = g_ctx.score_Pyy.as<double>();
  a.out = nullptr;
  a.lnbeta_half_df = lnb;
  a.p_max = p_max;
  a.f_thr = g_ctx.score_fthr.as<double>();
  a.hits = reinterpret_cast<ScoreHit *>(hits_d);
  a.cap = cap;
  a.n_hits = n_hits_d;
  a.cells = best_d ? g_ctx.score_cells.as<ScoreCell>() : nullptr;
  ProfScope ps(GEMMA_STAGE_ASSOC, s);
  const bool al = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(UtX) & 15) == 0;
  if (al) hipLaunchKernelGGL((score_panel_kernel<true, true>), dim3((unsigned)(npt * nst)), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((score_panel_kernel<false, true>), dim3((unsigned)(npt * nst)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  if (best_d) {
    hipLaunchKernelGGL(score_best_kernel, dim3((unsigned)((g.T + 255) / 256)), dim3(256), 0, s, g, (long)ntile,
                       (const ScoreCell *)g_ctx.score_cells.as<ScoreCell>(), g_ctx.score_Pyy.as<double>(), lnb,
                       reinterpret_cast<ScoreBest *>(best_d));
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_score_panel_hits_assoc_d(const double *UtX_d, size_t l, size_t ld_utx, double p_max,
                                                      gemma_score_hit *hits_d, size_t cap, unsigned long long *n_hits_d,
                                                      gemma_score_best *best_d, void *stream) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_hits_assoc");
  int rc = score_hits_check("lmm_score_panel_hits_assoc", l, p_max, hits_d, cap, n_hits_d);
  if (rc) return rc;
  if (l == 0) return score_hits_empty(n_hits_d, best_d, S(stream));
  if (!UtX_d || ld_utx < g_ctx.cfg.n) return fail(GEMMA_HIP_EINVAL, "lmm_score_panel_hits_assoc: bad UtX/ld");
  if ((rc = xp_flush_fwd(S(stream)))) return rc;
  return launch_score_hits(UtX_d, l, ld_utx, p_max, hits_d, cap, n_hits_d, best_d, S(stream));
}

extern "C" int gemma_hip_lmm_score_panel_hits_batch_d(int kind, const void *geno, size_t l, size_t ld, double p_max,
                                                      gemma_score_hit *hits_d, size_t cap, unsigned long long *n_hits_d,
                                                      gemma_score_best *best_d, void *stream) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_hits_batch");
  int rc = score_hits_check("lmm_score_panel_hits_batch", l, p_max, hits_d, cap, n_hits_d);
  if (rc) return rc;
  hipStream_t s = S(stream);
  if (l == 0) return score_hits_empty(n_hits_d, best_d, s);
  if ((rc = block_geom("lmm_score_panel_hits_batch", kind, g_ctx.cfg.n, true, geno, l, ld, n_hits_d))) return rc;
  double *UtX;
  size_t ldx;
  if ((rc = compute_utx(kind, geno, l, ld, -1, &UtX, &ldx, s))) return rc;
  if ((rc = launch_score_hits(UtX, l, ldx, p_max, hits_d, cap, n_hits_d, best_d, s))) return rc;
  score_remember(UtX, l, ldx);
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_score_panel_hits_batch(int kind, const void *geno, size_t l, size_t ld, double p_max,
                                                    gemma_score_hit *hits, size_t cap, unsigned long long *n_hits,
                                                    gemma_score_best *best) {
  NEED_INIT();
  NEED_SCORE("lmm_score_panel_hits_batch");
  int rc = score_hits_check("lmm_score_panel_hits_batch", l, p_max, hits, cap, n_hits);
  if (rc) return rc;
  const size_t T = g_ctx.score_T;
  if (g_ctx.score_cnt.reserve(8) || (best && g_ctx.score_best.reserve(T * sizeof(gemma_score_best))) ||
      (cap && g_ctx.score_hits.reserve(cap * sizeof(gemma_score_hit))))
    return fail(GEMMA_HIP_ENOMEM, "lmm_score_panel_hits_batch: a list of %zu hits (%zu bytes)", cap, cap * sizeof(gemma_score_hit));
  gemma_score_hit *hits_d = cap ? g_ctx.score_hits.as<gemma_score_hit>() : nullptr;
  gemma_score_best *best_d = best ? g_ctx.score_best.as<gemma_score_best>() : nullptr;
  if (l == 0) {
    if ((rc = score_hits_empty(g_ctx.score_cnt.as<unsigned long long>(), best_d, nullptr))) return rc;
  } else {
    BlockGeom g;
    if ((rc = block_geom("lmm_score_panel_hits_batch", kind, g_ctx.cfg.n, true, geno, l, ld, n_hits, &g))) return rc;
    if ((rc = stage_block("lmm_score_panel_hits_batch", g, geno, ld))) return rc;
    rc = gemma_hip_lmm_score_panel_hits_batch_d(kind, g_ctx.stage_in.p, l, ld, p_max, hits_d, cap, g_ctx.score_cnt.as<unsigned long long>(),
                                                best_d, nullptr);
    if (rc) return rc;
  }
  HIPCHK(hipMemcpy(n_hits, g_ctx.score_cnt.p, sizeof(unsigned long long), hipMemcpyDeviceToHost));
  const size_t kept = *n_hits < cap ? (size_t)*n_hits : cap;
  if (kept) {
    HIPCHK(hipMemcpy(hits, hits_d, kept * sizeof(gemma_score_hit), hipMemcpyDeviceToHost));
    std::sort(hits, hits + kept, [](const gemma_score_hit &x, const gemma_score_hit &y) {
      return x.pheno != y.pheno ? x.pheno < y.pheno : x.snp < y.snp;
    });
  }
  if (best) HIPCHK(hipMemcpy(best, best_d, T * sizeof(gemma_score_best), hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

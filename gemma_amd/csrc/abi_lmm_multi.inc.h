// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace).
// This part: T univariate LMMs over one U^T x (gemma_hip_lmm_multi_*): the phenotype slots, the shared fixed-lambda table.
//
// A block costs ingest + U^T x ONCE (50 of 56 ms at n = B = 20 000) and the per-SNP stage per phenotype (3 ms).  What of a setup
// belongs to the phenotype is a Ctx::PhenoSlot; the per-SNP stage of phenotype t is launch_assoc on slot t, as a single-phenotype
// setup of y_t runs it on the single slot: same kernels, same arguments, same launch shapes, its own
// PLINK carry chain in block order.  Of the stage's two reads of U^T x the first (the dense fixed-lambda table) depends on the
// phenotype in nq of its columns only: table_v2_kernel on the weight matrix of a group of multi_G phenotypes and
// table_multi_reduce_kernel (lmm_grid.hip.h) give the group's tables from one read, bit for bit the tables launch_grid_table
// gives (GEMMA_HIP_MULTI_TABLE=0: every phenotype computes its own).
// The three setups are multi_setup: lmm_bind (abi_lmm_stage.inc.h) for U, eval, UtW and U^T Y, then multi_setup_slots; the host form
// of a block is host_batch (abi_host_block.inc.h).

// weight matrices of the shared table, one per group of multi_G phenotypes; needs the slots' Uty and the setup's UtWt / eval
static int multi_make_weights(hipStream_t s) {
  g_ctx.multi_G = 0;
  const size_t T = g_ctx.multi_T, c = g_ctx.cfg.n_cvt;
  const Ctx::PhenoSlot &p0 = g_ctx.slots[0];
  if (!p0.proto.have_grid || !table_v2_enabled() || p0.grid_geom.nbx != 2) return GEMMA_HIP_OK;
  const int G = std::min(MULTI_GMAX, MULTI_NBA * 16 / p0.grid_geom.nq - (int)c);
  if (G < 2 || T < 2) return GEMMA_HIP_OK; // c = 4: the budget holds one phenotype, which is the single-phenotype kernel
  const GridGeom gg = p0.grid_geom;
  const size_t r_elems = (size_t)gg.nc * (size_t)(gg.nbx + MULTI_NBA) * 256;
  const size_t groups = (T + G - 1) / G;
  if (g_ctx.multi_R.reserve(groups * r_elems * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_multi_setup: weights of the shared table (%zu bytes)", groups * r_elems * 8);
  AssocArgs k = p0.proto;
  k.eval = g_ctx.eval;
  k.UtWt = g_ctx.UtWt.as<double>();
  for (size_t grp = 0; grp < groups; ++grp) {
    MultiWeights mw;
    mw.G = (int)std::min((size_t)G, T - grp * G);
    for (int g = 0; g < MULTI_GMAX; ++g) mw.Uty[g] = g_ctx.slots[std::min(T - 1, grp * G + g)].Uty;
    hipLaunchKernelGGL(grid_weights_multi_kernel, dim3((unsigned)((r_elems + 255) / 256)), dim3(256), 0, s, k, gg, (int)c, mw,
                       g_ctx.multi_R.as<double>() + grp * r_elems);
    HIPCHK(hipGetLastError());
  }
  g_ctx.multi_G = G;
  return GEMMA_HIP_OK;
}

// After lmm_bind: g_ctx.U / g_ctx.eval in place.  UtW_d: n x c, UtY_d: n x T row-major, both on the device.
static int multi_setup_slots(size_t T, const double *l_mle_null, const double *logl_mle_H0, const double *UtW_d,
                             const double *UtY_d, hipStream_t s) {
  const size_t n = g_ctx.cfg.n;
  if (g_ctx.multi_Yt.reserve(T * n * 8)) return fail(GEMMA_HIP_ENOMEM, "lmm_multi_setup: U^T Y (%zu bytes)", T * n * 8);
  {
    dim3 grid((unsigned)((T + 31) / 32), (unsigned)((n + 31) / 32));
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(32, 8), 0, s, UtY_d, (long)n, (long)T, (long)T, g_ctx.multi_Yt.as<double>(),
                       (long)n);
    HIPCHK(hipGetLastError());
  }
  g_ctx.slots.clear();
  g_ctx.slots.resize(T);
  g_ctx.multi_T = T; // from here on a failure leaves a multi state that lmm_common_setup / the caller's multi_release takes down
  for (size_t t = 0; t < T; ++t) {
    Ctx::PhenoSlot &p = g_ctx.slots[t]; // built in place: whatever happens, multi_release finds every buffer in a slot
    // the setup's part of the proto: lmm_common_setup's for slot 0, which make_utwt completes (log-determinant ends); slot 0's for
    // the others, of which make_grid redoes the tables' part
    p.proto = t == 0 ? g_ctx.single.proto : g_ctx.slots[0].proto;
    if (p.carry.reserve(4 * 8)) return fail(GEMMA_HIP_ENOMEM, "lmm_multi_setup: carry");
    HIPCHK(hipMemset(p.carry.p, 0, 4 * 8));
    p.carry_flip = 0;
    p.proto.l_mle_null = l_mle_null ? l_mle_null[t] : 0.0;
    p.proto.logl_mle_H0 = logl_mle_H0 ? logl_mle_H0[t] : 0.0;
    p.Uty = g_ctx.multi_Yt.as<double>() + t * n;
    const int rc = t == 0 ? make_utwt(p, UtW_d, s) : make_grid(p, s);
    if (rc == GEMMA_HIP_ENOMEM) {
      const Ctx::PhenoSlot &p0 = g_ctx.slots[0];
      const size_t per = p0.grid_R.cap + p0.grid_F.cap + p0.cheb_R.cap + p0.cheb_F.cap;
      return fail(GEMMA_HIP_ENOMEM, "lmm_multi_setup: the tables of phenotype %zu of %zu do not fit (%zu bytes per phenotype)", t + 1, T,
                  per);
    }
    if (rc) return rc;
  }
  return multi_make_weights(s);
}

static int multi_check(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *logl_mle_H0) {
  if (!cfg) return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup: null cfg");
  if (T == 0 || T > (size_t)GEMMA_LMM_MULTI_MAX)
    return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup: T=%zu phenotypes (1..%d)", T, GEMMA_LMM_MULTI_MAX);
  if (cfg->a_mode != 1 && (!l_mle_null || !logl_mle_H0))
    return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup: a_mode %d needs l_mle_null and logl_mle_H0 of every phenotype", cfg->a_mode);
  return GEMMA_HIP_OK;
}
// the three multi setups after their argument checks (lmm_bind: a failed setup leaves lmm_active false) -- and no slots behind
static int multi_setup(const char *who, SetupSrc src, const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null,
                       const double *logl_mle_H0, const double *U, const double *eval, const double *UtW, const double *UtY,
                       hipStream_t s) {
  const double *UtW_d, *UtY_d;
  int rc = lmm_bind(who, src, cfg, U, eval, UtW, UtY, T, &UtW_d, &UtY_d);
  if (rc) return rc;
  if ((rc = multi_setup_slots(T, l_mle_null, logl_mle_H0, UtW_d, UtY_d, s))) {
    multi_release();
    return rc;
  }
  if (src != SetupSrc::Device) HIPCHK(hipDeviceSynchronize());
  g_ctx.lmm_active = true;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_multi_setup_d(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null,
                                           const double *logl_mle_H0, const double *U_d, const double *eval_d,
                                           const double *UtW_d, const double *UtY_d, void *stream) {
  NEED_INIT();
  if (!U_d || !eval_d || !UtW_d || !UtY_d) return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup: null pointer");
  if (int rc = multi_check(cfg, T, l_mle_null, logl_mle_H0)) return rc;
  return multi_setup("lmm_multi_setup", SetupSrc::Device, cfg, T, l_mle_null, logl_mle_H0, U_d, eval_d, UtW_d, UtY_d, S(stream));
}

extern "C" int gemma_hip_lmm_multi_setup(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null, const double *logl_mle_H0,
                                         const double *U, const double *eval, const double *UtW, const double *UtY) {
  NEED_INIT();
  if (!U || !eval || !UtW || !UtY) return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup: null pointer");
  if (int rc = multi_check(cfg, T, l_mle_null, logl_mle_H0)) return rc;
  return multi_setup("lmm_multi_setup", SetupSrc::Host, cfg, T, l_mle_null, logl_mle_H0, U, eval, UtW, UtY, nullptr);
}

extern "C" int gemma_hip_lmm_multi_setup_kept(const gemma_lmm_cfg *cfg, size_t T, const double *l_mle_null,
                                              const double *logl_mle_H0, const double *UtW, const double *UtY) {
  NEED_INIT();
  if (!g_ctx.kept_n) return fail(GEMMA_HIP_ESTATE, "lmm_multi_setup_kept: no kept U");
  if (!UtW || !UtY) return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup_kept: null pointer");
  if (int rc = multi_check(cfg, T, l_mle_null, logl_mle_H0)) return rc;
  if (cfg->n != g_ctx.kept_n)
    return fail(GEMMA_HIP_EINVAL, "lmm_multi_setup_kept: cfg.n=%zu, kept U is %zu", cfg->n, g_ctx.kept_n);
  return multi_setup("lmm_multi_setup_kept", SetupSrc::Kept, cfg, T, l_mle_null, logl_mle_H0, nullptr, nullptr, UtW, UtY, nullptr);
}

// the tables of group grp (Gn phenotypes) for the l rows of UtX -> multi_T_buf, Gn tables of l * grid_ld doubles
static int launch_table_multi(size_t grp, int Gn, const double *UtX, size_t l, size_t ld, hipStream_t s) {
  const Ctx::PhenoSlot &p0 = g_ctx.slots[0];
  const GridGeom &gg = p0.grid_geom;
  constexpr int NB16M = (2 + MULTI_NBA) * 16;
  const size_t nb16 = (size_t)p0.proto.grid_ld;
  const int ksplit = table_ksplit(gg.nc);
  if (g_ctx.table_P.reserve((size_t)ksplit * l * NB16M * 8) || g_ctx.multi_T_buf.reserve((size_t)Gn * l * nb16 * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_multi_batch: shared table partial sums (%zu bytes)", (size_t)ksplit * l * NB16M * 8);
  const size_t r_elems = (size_t)gg.nc * (size_t)(gg.nbx + MULTI_NBA) * 256;
  TableV2 a;
  a.UtX = UtX; a.ld = (long)ld; a.l = (long)l; a.n = (int)g_ctx.cfg.n; a.nc = gg.nc; a.ksplit = ksplit;
  a.Rp = g_ctx.multi_R.as<double>() + grp * r_elems;
  a.P = g_ctx.table_P.as<double>(); a.cap = (long)l;
  a.tg = TableGather();
  const size_t rows_per_block = (size_t)MULTI_RG * 16 * 4;
  const dim3 grid((unsigned)((l + rows_per_block - 1) / rows_per_block), (unsigned)ksplit);
  if (g_ctx.knobs.table_pf) hipLaunchKernelGGL((table_v2_kernel<2, MULTI_NBA, MULTI_RG, false, true>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((table_v2_kernel<2, MULTI_NBA, MULTI_RG, false, false>), grid, dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  TableMulti m;
  m.P = a.P; m.ksplit = ksplit; m.cap = (long)l; m.l = (long)l; m.nb16m = NB16M; m.nb16 = (int)nb16;
  m.y0 = p0.proto.grid_xa0 + (int)g_ctx.cfg.n_cvt * gg.nq; m.nq = gg.nq;
  m.T = g_ctx.multi_T_buf.as<double>(); m.tstride = (long)(l * nb16);
  hipLaunchKernelGGL(table_multi_reduce_kernel, dim3((unsigned)((l * nb16 + 255) / 256), (unsigned)Gn), dim3(256), 0, s, m);
  HIPCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_multi_batch_d(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out_d, void *stream) {
  NEED_INIT();
  if (!g_ctx.lmm_active || !g_ctx.multi_T) return fail(GEMMA_HIP_ESTATE, "lmm_multi_batch before lmm_multi_setup");
  if (l == 0) return GEMMA_HIP_OK;
  int rc = block_geom("lmm_multi_batch", kind, g_ctx.cfg.n, true, geno, l, ld, out_d);
  if (rc) return rc;
  hipStream_t s = S(stream);
  double *UtX;
  size_t ldx;
  if ((rc = compute_utx(kind, geno, l, ld, -1, &UtX, &ldx, s))) return rc;
  const size_t T = g_ctx.multi_T;
  bool shared = g_ctx.knobs.multi_table && g_ctx.multi_G >= 2 && table_v2_enabled() &&
                assoc_takes_tables(g_ctx.slots[0].proto, UtX, ldx);
  const size_t G = shared ? (size_t)g_ctx.multi_G : 1;
  const size_t tstride = l * (size_t)g_ctx.slots[0].proto.grid_ld;
  for (size_t t0 = 0; t0 < T; t0 += G) {
    const size_t Gn = std::min(G, T - t0);
    if (shared) {
      ProfScope ps(GEMMA_STAGE_ASSOC, s);
      rc = launch_table_multi(t0 / G, (int)Gn, UtX, l, ldx, s);
      if (rc && rc != GEMMA_HIP_ENOMEM) return rc;
      if (rc) shared = false; // an accelerator, not a requirement (launch_assoc): this and the later groups compute their own tables
    }
    for (size_t g = 0; g < Gn; ++g) {
      rc = launch_assoc(g_ctx.slots[t0 + g], UtX, l, ldx, out_d + (t0 + g) * l, s,
                        shared ? g_ctx.multi_T_buf.as<double>() + g * tstride : nullptr);
      if (rc) return rc;
    }
  }
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_multi_batch(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out) {
  NEED_INIT();
  if (!g_ctx.lmm_active || !g_ctx.multi_T) return fail(GEMMA_HIP_ESTATE, "lmm_multi_batch before lmm_multi_setup");
  if (l == 0) return GEMMA_HIP_OK;
  return host_batch("lmm_multi_batch", kind, geno, l, ld, g_ctx.stage_out, out, g_ctx.multi_T * l * sizeof(gemma_sumstat),
                    [&](const void *in_d, void *out_d) {
                      return gemma_hip_lmm_multi_batch_d(kind, in_d, l, ld, static_cast<gemma_sumstat *>(out_d), nullptr);
                    });
}

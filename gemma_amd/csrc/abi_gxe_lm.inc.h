// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace, and are
// included there in this order).
// This part: GXE, host-pointer batch, dbg_utx, the linear model (-lm) with its release list (lm_release), the null model, lmm_finish.

// ---- GXE variants: LMM::AnalyzeBimbamGXE / AnalyzePlinkGXE, src/lmm.cpp:2283-2608
// env over the analysed individuals (after lmm_setup): U^T env becomes the (c+1)-th shared covariate row (:2307-2309)
extern "C" int gemma_hip_lmm_set_env(const double *env) {
  NEED_INIT();
  if (!g_ctx.lmm_active) return fail(GEMMA_HIP_ESTATE, "lmm_set_env before lmm_setup");
  NEED_SINGLE("lmm_set_env");
  if (!env) return fail(GEMMA_HIP_EINVAL, "lmm_set_env: null pointer");
  const size_t n = g_ctx.cfg.n, c = g_ctx.cfg.n_cvt;
  if (c + 2 > (size_t)GEN_CMAX_WIDE)
    return fail(GEMMA_HIP_EINVAL, "lmm_set_env: n_cvt + 2 = %zu covariates not supported (<= %d)", c + 2, GEN_CMAX_WIDE);
  if (n <= c + 3) return fail(GEMMA_HIP_EINVAL, "lmm_set_env: n <= n_cvt + 3");
  if (g_ctx.gxe_env.reserve(n * 8) || g_ctx.gxe_UtWt.reserve((c + 1) * n * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_set_env: buffers");
  HIPCHK(hipMemcpy(g_ctx.gxe_env.p, env, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g_ctx.gxe_UtWt.p, g_ctx.UtWt.p, c * n * 8, hipMemcpyDeviceToDevice));
  // U^T env (gsl_blas_dgemv(CblasTrans, U, env), :2308): (n x 1) = U^T (n x n) * env (n x 1)
  HIPCHK(launch_dgemm('T', 'N', (long)n, 1, (long)n, 1.0, g_ctx.U, (long)n, g_ctx.gxe_env.as<double>(), 1, 0.0,
                      g_ctx.gxe_UtWt.as<double>() + c * n, 1, false, false, 0));
  HIPCHK(hipDeviceSynchronize());
  g_ctx.gxe_lnbeta = lnbeta_half((double)n - (double)(c + 2) - 1.0);
  g_ctx.gxe_ready = true;
  return GEMMA_HIP_OK;
}

// The rotated operands of a GXE block, univariate (below) and multivariate (mvlmm_gxe_batch_d, abi_mvlmm.inc.h) alike, on stream s.
struct GxeBlock {
  double *UtX, *UtZ; // U^T x_s and U^T (x_s . env), l rows of leading dimension ldx
  int *flip;         // the allele flip of every row
  size_t ldx;
};
// x, z = x . env and the flip of the l rows of a SNP-major block (ingest_gxe_kernel), both rotated by fp64 GEMMs (z is real-valued).
// who: the caller's name for the error text.
static int gxe_rotate_block(const char *who, int kind, const void *geno, size_t l, size_t ld, hipStream_t s, GxeBlock &b) {
  const size_t n = g_ctx.cfg.n;
  const size_t ldx = (n + 1) & ~(size_t)1;
  if (int rcf = xp_flush(s)) return rcf; // blocks of the two-block pipeline still in flight share these buffers
  g_ctx.last_UtX = nullptr;
  if (g_ctx.X.reserve(l * ldx * 8) || g_ctx.UtX.reserve(l * ldx * 8) || g_ctx.gxe_Z.reserve(l * ldx * 8) ||
      g_ctx.gxe_UtZ.reserve(l * ldx * 8) || g_ctx.gxe_flip.reserve(l * sizeof(int)))
    return fail(GEMMA_HIP_ENOMEM, "%s: cannot allocate 4 x %zu bytes", who, l * ldx * 8);
  double *X = g_ctx.X.as<double>(), *Z = g_ctx.gxe_Z.as<double>();
  b.UtX = g_ctx.UtX.as<double>();
  b.UtZ = g_ctx.gxe_UtZ.as<double>();
  b.flip = g_ctx.gxe_flip.as<int>();
  b.ldx = ldx;
  {
    ProfScope ps(GEMMA_STAGE_INGEST, s);
    IngestGxeArgs a;
    a.src = geno; a.ld = (long)ld; a.l = (long)l;
    a.idx_map = g_ctx.have_map ? g_ctx.idx_map.as<int>() : nullptr;
    a.n = (int)n; a.env = g_ctx.gxe_env.as<double>(); a.X = X; a.Z = Z; a.ldo = (long)ldx;
    a.flip = b.flip;
    const unsigned grid = (unsigned)((l + 3) / 4);
    if (kind == GEMMA_GENO_PLINK_2BIT)
      hipLaunchKernelGGL(ingest_gxe_kernel<true>, dim3(grid), dim3(256), 0, s, a);
    else
      hipLaunchKernelGGL(ingest_gxe_kernel<false>, dim3(grid), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  {
    ProfScope ps(GEMMA_STAGE_UTX_GEMM, s); // U^T x_s (:2364) and U^T (x_s . env) (:2366)
    const double *Ug;
    long ldu;
    int rcu = gemm_U(&Ug, &ldu, s);
    if (rcu) return rcu;
    HIPCHK(launch_dgemm('N', 'N', (long)l, (long)n, (long)n, 1.0, X, (long)ldx, Ug, ldu, 0.0, b.UtX, (long)ldx, false, false, s));
    HIPCHK(launch_dgemm('N', 'N', (long)l, (long)n, (long)n, 1.0, Z, (long)ldx, Ug, ldu, 0.0, b.UtZ, (long)ldx, false, false, s));
  }
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_gxe_batch_d(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out_d,
                                         void *stream) {
  NEED_INIT();
  if (!g_ctx.lmm_active || !g_ctx.gxe_ready) return fail(GEMMA_HIP_ESTATE, "lmm_gxe_batch before lmm_setup + lmm_set_env");
  if (l == 0) return GEMMA_HIP_OK;
  if (kind == GEMMA_GENO_F64_IDV_MAJOR) return fail(GEMMA_HIP_EINVAL, "lmm_gxe_batch: SNP-major input only");
  int rc = block_geom("lmm_gxe_batch", kind, g_ctx.cfg.n, true, geno, l, ld, out_d);
  if (rc) return rc;
  hipStream_t s = S(stream);
  const size_t c = g_ctx.cfg.n_cvt;
  GxeBlock b;
  if ((rc = gxe_rotate_block("lmm_gxe_batch", kind, geno, l, ld, s, b))) return rc;
  AssocArgs a = g_ctx.single.proto;
  a.UtX = b.UtX; a.UtZ = b.UtZ; a.flip = b.flip;
  a.ld = (long)b.ldx; a.l = (long)l;
  a.eval = g_ctx.eval; a.Uty = g_ctx.single.Uty; a.UtWt = g_ctx.gxe_UtWt.as<double>();
  a.out = reinterpret_cast<SumStat *>(out_d);
  a.lnbeta_half_df = g_ctx.gxe_lnbeta; // df = n - (c + 2) - 1
  a.grid_T = nullptr;
  a.have_grid = 0;
  const unsigned grid = (unsigned)((l + 3) / 4);
  {
    ProfScope ps(GEMMA_STAGE_ASSOC, s);
    switch (c + 2) {
    case 3: hipLaunchKernelGGL(lmm_gxe_kernel<3>, dim3(grid), dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL(lmm_gxe_kernel<4>, dim3(grid), dim3(256), 0, s, a); break;
    default:
      if (c + 2 > (size_t)GEN_CMAX) {
        int rcw = wide_attr(lmm_gxe_wide_kernel);
        if (rcw) return rcw;
        hipLaunchKernelGGL(lmm_gxe_wide_kernel, dim3((unsigned)l), dim3(64), wide_lds_bytes(c + 2), s, a, (int)(c + 2));
      } else {
        hipLaunchKernelGGL(lmm_gxe_generic_kernel, dim3(grid), dim3(256), 0, s, a, (int)(c + 2));
      }
      break;
    }
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_gxe_batch(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out) {
  NEED_INIT();
  if (!g_ctx.lmm_active || !g_ctx.gxe_ready) return fail(GEMMA_HIP_ESTATE, "lmm_gxe_batch before lmm_setup + lmm_set_env");
  if (l == 0) return GEMMA_HIP_OK;
  if (kind == GEMMA_GENO_F64_IDV_MAJOR) return fail(GEMMA_HIP_EINVAL, "lmm_gxe_batch: SNP-major input only");
  return host_batch("lmm_gxe_batch", kind, geno, l, ld, g_ctx.stage_out, out, l * sizeof(gemma_sumstat),
                    [&](const void *in_d, void *out_d) {
                      return gemma_hip_lmm_gxe_batch_d(kind, in_d, l, ld, static_cast<gemma_sumstat *>(out_d), nullptr);
                    });
}

extern "C" int gemma_hip_dbg_utx(int kind, const void *geno, size_t l, size_t ld, int path, double *UtX_host) {
  NEED_INIT();
  if (!g_ctx.lmm_active) return fail(GEMMA_HIP_ESTATE, "dbg_utx before lmm_setup");
  if (l == 0) return GEMMA_HIP_OK;
  BlockGeom g;
  int rc = block_geom("dbg_utx", kind, g_ctx.cfg.n, true, geno, l, ld, UtX_host, &g);
  if (!rc) rc = stage_block("dbg_utx", g, geno, ld);
  if (rc) return rc;
  const size_t n = g_ctx.cfg.n;
  double *UtX;
  size_t ldx;
  rc = compute_utx(kind, g_ctx.stage_in.p, l, ld, path ? 1 : 0, &UtX, &ldx, 0);
  if (rc) return rc;
  HIPCHK(hipMemcpy2D(UtX_host, n * 8, UtX, ldx * 8, n * 8, l, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_batch(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out) {
  NEED_INIT();
  if (!g_ctx.lmm_active) return fail(GEMMA_HIP_ESTATE, "lmm_batch before lmm_setup");
  NEED_SINGLE("lmm_batch");
  if (l == 0) return GEMMA_HIP_OK;
  return host_batch("lmm_batch", kind, geno, l, ld, g_ctx.stage_out, out, l * sizeof(gemma_sumstat),
                    [&](const void *in_d, void *out_d) {
                      return gemma_hip_lmm_batch_d(kind, in_d, l, ld, static_cast<gemma_sumstat *>(out_d), nullptr);
                    });
}

// ------------------------------------------------------------------------------ linear model (-lm)
extern "C" int gemma_hip_lm_setup(int a_mode, size_t n, size_t n_cvt, const double *W, const double *y) {
  NEED_INIT();
  g_ctx.knobs.load();
  if (g_ctx.lmm_active) return fail(GEMMA_HIP_ESTATE, "lm_setup while an LMM run is active");
  if (a_mode < 51 || a_mode > 54) return fail(GEMMA_HIP_EINVAL, "lm_setup: a_mode %d (51..54)", a_mode);
  if (!W || !y || n == 0 || n_cvt == 0 || n_cvt > (size_t)LM_CMAX || n <= n_cvt + 1 || n > 0x7fffffffUL)
    return fail(GEMMA_HIP_EINVAL, "lm_setup: bad arguments (n_cvt 1..%d)", LM_CMAX);
  const int c = (int)n_cvt;
  std::vector<double> WtW((size_t)c * c, 0.0), Wt((size_t)c * n), Wty(c, 0.0);
  double yy = 0.0;
  for (size_t i = 0; i < n; ++i) {
    yy += y[i] * y[i];
    for (int a = 0; a < c; ++a) {
      Wt[(size_t)a * n + i] = W[i * c + a];
      Wty[a] += W[i * c + a] * y[i];
      for (int b = 0; b < c; ++b) WtW[(size_t)a * c + b] += W[i * c + a] * W[i * c + b];
    }
  }
  if (!invert_small(WtW, c)) return fail(GEMMA_HIP_EINVAL, "lm_setup: W^T W is singular");
  double d = 0.0; // CalcvPv(WtWi, Wty, y, yPwy), src/lm.cpp:247-263
  for (int a = 0; a < c; ++a) {
    double t = 0.0;
    for (int b = 0; b < c; ++b) t += WtW[(size_t)a * c + b] * Wty[b];
    d += t * Wty[a];
  }
  if (g_ctx.lm_Wt.reserve(Wt.size() * 8) || g_ctx.lm_y.reserve(n * 8) || g_ctx.lm_small.reserve(((size_t)c * c + c) * 8))
    return fail(GEMMA_HIP_ENOMEM, "lm_setup: allocation");
  HIPCHK(hipMemcpy(g_ctx.lm_Wt.p, Wt.data(), Wt.size() * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g_ctx.lm_y.p, y, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g_ctx.lm_small.p, WtW.data(), (size_t)c * c * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g_ctx.lm_small.as<double>() + (size_t)c * c, Wty.data(), c * 8, hipMemcpyHostToDevice));
  LmArgs &a = g_ctx.lm_proto;
  memset(&a, 0, sizeof a);
  a.Wt = g_ctx.lm_Wt.as<double>();
  a.y = g_ctx.lm_y.as<double>();
  a.WtWi = g_ctx.lm_small.as<double>();
  a.Wty = g_ctx.lm_small.as<double>() + (size_t)c * c;
  a.yPwy = yy - d;
  a.n = (int)n;
  a.c = c;
  a.test_mode = a_mode - 50;
  a.lnbeta_half_df = lnbeta_half((double)n - (double)c - 1.0);
  g_ctx.cfg.n = n; // shared with the ingest / indicator code
  g_ctx.cfg.n_cvt = n_cvt;
  g_ctx.have_map = false;
  g_ctx.ni_total = 0;
  g_ctx.lm_active = true;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lm_batch_d(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out_d, void *stream) {
  NEED_INIT();
  if (!g_ctx.lm_active) return fail(GEMMA_HIP_ESTATE, "lm_batch before lm_setup");
  if (l == 0) return GEMMA_HIP_OK;
  const size_t n = g_ctx.cfg.n;
  if (int rc = block_geom("lm_batch", kind, n, true, geno, l, ld, out_d)) return rc;
  hipStream_t s = S(stream);
  const size_t ldx = (n + 1) & ~(size_t)1;
  if (g_ctx.X.reserve(l * ldx * 8)) return fail(GEMMA_HIP_ENOMEM, "lm_batch: cannot allocate %zu bytes", l * ldx * 8);
  double *X = g_ctx.X.as<double>();
  if (int rc = ingest_f64(kind, geno, l, ld, X, ldx, s)) return rc;
  LmArgs a = g_ctx.lm_proto;
  a.X = X; a.ld = (long)ldx; a.l = (long)l;
  a.out = reinterpret_cast<SumStat *>(out_d);
  {
    ProfScope ps(GEMMA_STAGE_ASSOC, s);
    hipLaunchKernelGGL(lm_assoc_kernel, dim3((unsigned)((l + 3) / 4)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lm_batch(int kind, const void *geno, size_t l, size_t ld, gemma_sumstat *out) {
  NEED_INIT();
  if (!g_ctx.lm_active) return fail(GEMMA_HIP_ESTATE, "lm_batch before lm_setup");
  if (l == 0) return GEMMA_HIP_OK;
  return host_batch("lm_batch", kind, geno, l, ld, g_ctx.stage_out, out, l * sizeof(gemma_sumstat),
                    [&](const void *in_d, void *out_d) {
                      return gemma_hip_lm_batch_d(kind, in_d, l, ld, static_cast<gemma_sumstat *>(out_d), nullptr);
                    });
}

// everything the -lm state owns (X, the staging buffers and the indicator map it shares with the LMM state)
static void lm_release() {
  g_ctx.lm_Wt.release(); g_ctx.lm_y.release(); g_ctx.lm_small.release();
  g_ctx.X.release(); g_ctx.stage_in.release(); g_ctx.stage_out.release(); g_ctx.idx_map.release();
  g_ctx.lm_active = false;
}

extern "C" int gemma_hip_lm_finish(void) {
  NEED_INIT();
  if (!g_ctx.lm_active) return fail(GEMMA_HIP_ESTATE, "lm_finish before lm_setup");
  HIPCHK(hipDeviceSynchronize());
  lm_release();
  return GEMMA_HIP_OK;
}

// Null model on device.  out[8] = { l_mle_null, logl_mle_H0, l_remle_null, logl_remle_H0,
// pve, pve_se, vg_remle, ve_remle } -- the quantities src/gemma.cpp:2711-2750 derives before
// the per-SNP loop (CalcLambda 'L'/'R' with calc_null, CalcPve src/lmm.cpp:2183-2205, and the
// vg/ve part of CalcLmmVgVeBeta :2253-2259).
extern "C" int gemma_hip_lmm_null(size_t n, size_t n_cvt, const double *eval, const double *UtW,
                                  const double *Uty, double l_min, double l_max, size_t n_region,
                                  double trace_G, double *out8) {
  NEED_INIT();
  if (!eval || !UtW || !Uty || !out8 || n == 0 || n_cvt == 0 || n_cvt > (size_t)GEN_CMAX_WIDE + 1)
    return fail(GEMMA_HIP_EINVAL, "lmm_null: bad arguments (n_cvt 1..%d)", GEN_CMAX_WIDE + 1);
  if (!(l_max > l_min) || n_region == 0 || n_region > (size_t)ASSOC_MAX_REGION || n <= n_cvt)
    return fail(GEMMA_HIP_EINVAL, "lmm_null: l_min/l_max/n_region/n");
  ScopedBuf dE, dW, dWt, dY, dO;
  if (dE.reserve(n * 8) || dW.reserve(n * n_cvt * 8) || dWt.reserve(n * n_cvt * 8) || dY.reserve(n * 8) ||
      dO.reserve(sizeof(NullOut)))
    return fail(GEMMA_HIP_ENOMEM, "lmm_null: allocation");
  HIPCHK(hipMemcpy(dE.p, eval, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dW.p, UtW, n * n_cvt * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dY.p, Uty, n * 8, hipMemcpyHostToDevice));
  dim3 grid((unsigned)((n_cvt + 31) / 32), (unsigned)((n + 31) / 32));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(32, 8), 0, 0, dW.as<double>(), (long)n, (long)n_cvt,
                     (long)n_cvt, dWt.as<double>(), (long)n);
  AssocArgs a;
  memset(&a, 0, sizeof a);
  a.n = (int)n; a.n_region = (int)n_region; a.l_min = l_min; a.l_max = l_max;
  a.eval = dE.as<double>(); a.Uty = dY.as<double>(); a.UtWt = dWt.as<double>();
  fill_lam_grid(a, l_min, l_max, n_region);
  NullOut *o = dO.as<NullOut>();
  switch (n_cvt) {
  case 1: hipLaunchKernelGGL(lmm_null_kernel<0>, dim3(1), dim3(64), 0, 0, a, o); break;
  case 2: hipLaunchKernelGGL(lmm_null_kernel<1>, dim3(1), dim3(64), 0, 0, a, o); break;
  case 3: hipLaunchKernelGGL(lmm_null_kernel<2>, dim3(1), dim3(64), 0, 0, a, o); break;
  case 4: hipLaunchKernelGGL(lmm_null_kernel<3>, dim3(1), dim3(64), 0, 0, a, o); break;
  case 5: hipLaunchKernelGGL(lmm_null_kernel<4>, dim3(1), dim3(64), 0, 0, a, o); break;
  default:
    if (n_cvt - 1 > (size_t)GEN_CMAX) {
      (void)hipFuncSetAttribute(reinterpret_cast<const void *>(lmm_null_wide_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)wide_lds_bytes(GEN_CMAX_WIDE));
      hipLaunchKernelGGL(lmm_null_wide_kernel, dim3(1), dim3(64), wide_lds_bytes(n_cvt - 1), 0, a, (int)n_cvt - 1, o);
    } else {
      hipLaunchKernelGGL(lmm_null_generic_kernel, dim3(1), dim3(64), 0, 0, a, (int)n_cvt - 1, o);
    }
    break;
  }
  HIPCHK(hipGetLastError());
  NullOut h;
  HIPCHK(hipMemcpy(&h, dO.p, sizeof h, hipMemcpyDeviceToHost));
  null_derive(h, trace_G, n, n_cvt, out8);
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_finish(double *time_UtX_min, double *time_opt_min) {
  NEED_INIT();
  if (!g_ctx.lmm_active) return fail(GEMMA_HIP_ESTATE, "lmm_finish before lmm_setup");
  HIPCHK(hipDeviceSynchronize());
  pipe_release(); // blocks still in flight are dropped with the state
  xp_release();
  prof_collect(GEMMA_STAGE_UTX_GEMM);
  prof_collect(GEMMA_STAGE_UTX_POST);
  prof_collect(GEMMA_STAGE_ASSOC);
  if (time_UtX_min)
    *time_UtX_min = (g_ctx.prof[GEMMA_STAGE_UTX_GEMM].acc_ms + g_ctx.prof[GEMMA_STAGE_UTX_POST].acc_ms) / 60000.0;
  if (time_opt_min) *time_opt_min = g_ctx.prof[GEMMA_STAGE_ASSOC].acc_ms / 60000.0;
  lmm_release();
  return GEMMA_HIP_OK;
}

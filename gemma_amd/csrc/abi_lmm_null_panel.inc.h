// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace).
// This part: the null fits of a whole phenotype panel (gemma_hip_lmm_null_panel / _d): what gemma_hip_lmm_null computes for one
// column of U^T Y, for every column in one launch per chunk -- one wavefront per phenotype (lmm_null_panel.hip.h).
//
// Stateless like gemma_hip_lmm_null: the buffers are the call's own, no LMM setup is needed or disturbed.  The columns are walked in
// chunks; beyond eval and UtW (and its transposed copy) the device holds a chunk of U^T Y as it came (host form only) and its
// transposed copy.

static_assert(sizeof(gemma_null_fit) == sizeof(NullFit8) && sizeof(gemma_null_fit) == 64, "gemma_null_fit is out8 of gemma_hip_lmm_null");

static const size_t NULL_PANEL_NMAX = (size_t)65535 * 32;

static int null_panel_check(size_t n, size_t n_cvt, size_t T, const void *eval, const void *UtW, const void *UtY, double l_min,
                            double l_max, size_t n_region, const void *fit, const void *beta, const void *se_beta) {
  if (T == 0 || T > (size_t)INT_MAX - 64) return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: T=%zu phenotypes", T);
  if (!eval || !UtW || !UtY || !fit) return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: null pointer");
  if ((beta == nullptr) != (se_beta == nullptr))
    return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: beta and se_beta come together (both or neither)");
  if (n_cvt == 0 || n_cvt > (size_t)GEN_CMAX_WIDE + 1)
    return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: n_cvt=%zu covariates (1..%d)", n_cvt, GEN_CMAX_WIDE + 1);
  if (n <= n_cvt) return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: n=%zu individuals for n_cvt=%zu", n, n_cvt);
  if (n > NULL_PANEL_NMAX) // the transposes run 32 individuals per workgroup along grid.y
    return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: n=%zu individuals (at most %zu)", n, NULL_PANEL_NMAX);
  if (beta && n_cvt > (size_t)NP_CMAX)
    return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: beta / se_beta with n_cvt=%zu covariates (1..%d)", n_cvt, NP_CMAX);
  if (!(l_max > l_min)) return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: l_min=%g, l_max=%g", l_min, l_max);
  if (n_region == 0 || n_region > (size_t)ASSOC_MAX_REGION)
    return fail(GEMMA_HIP_EINVAL, "lmm_null_panel: n_region=%zu (1..%d)", n_region, ASSOC_MAX_REGION);
  return GEMMA_HIP_OK;
}

// columns per chunk: GEMMA_HIP_NULL_PANEL_CHUNK, else what half of the free memory holds at bytes_per_column
static size_t null_panel_chunk(size_t T, size_t bytes_per_column) {
  const char *e = getenv("GEMMA_HIP_NULL_PANEL_CHUNK");
  if (e && *e) {
    const long long v = atoll(e);
    if (v > 0) return std::min(T, (size_t)v);
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return T;
  }
  return std::min(T, std::max<size_t>(free_b / 2 / bytes_per_column, 1));
}

// The fits of Tc columns.  Y_d: n rows of Tc columns, leading dimension ldY; Yt_d: room for Tc x n; UtWt_d: c x n; o_d: Tc fits.
static int null_panel_launch(size_t n, size_t n_cvt, size_t Tc, const double *eval_d, const double *UtWt_d, const double *Y_d,
                             size_t ldY, double *Yt_d, double l_min, double l_max, size_t n_region, NullOut *o_d, double *beta_d,
                             double *se_d, hipStream_t s) {
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((Tc + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, Y_d, (long)n,
                     (long)Tc, (long)ldY, Yt_d, (long)n);
  HIPCHK(hipGetLastError());
  AssocArgs a;
  memset(&a, 0, sizeof a);
  a.n = (int)n; a.n_region = (int)n_region; a.l_min = l_min; a.l_max = l_max;
  a.eval = eval_d; a.UtWt = UtWt_d;
  fill_lam_grid(a, l_min, l_max, n_region);
  const int T = (int)Tc, cp = (int)n_cvt - 1;
  const dim3 grid((unsigned)((Tc + NP_WAVES - 1) / NP_WAVES)), block(64 * NP_WAVES);
  switch (n_cvt) {
  case 1: hipLaunchKernelGGL(lmm_null_panel_kernel<0>, grid, block, 0, s, a, Yt_d, T, o_d); break;
  case 2: hipLaunchKernelGGL(lmm_null_panel_kernel<1>, grid, block, 0, s, a, Yt_d, T, o_d); break;
  case 3: hipLaunchKernelGGL(lmm_null_panel_kernel<2>, grid, block, 0, s, a, Yt_d, T, o_d); break;
  case 4: hipLaunchKernelGGL(lmm_null_panel_kernel<3>, grid, block, 0, s, a, Yt_d, T, o_d); break;
  case 5: hipLaunchKernelGGL(lmm_null_panel_kernel<4>, grid, block, 0, s, a, Yt_d, T, o_d); break;
  default:
    if (cp > GEN_CMAX) {
      HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(lmm_null_panel_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)wide_lds_bytes(GEN_CMAX_WIDE)));
      hipLaunchKernelGGL(lmm_null_panel_wide_kernel, dim3((unsigned)Tc), dim3(64), wide_lds_bytes(cp), s, a, cp, Yt_d, T, o_d);
    } else {
      hipLaunchKernelGGL(lmm_null_panel_generic_kernel, grid, block, 0, s, a, cp, Yt_d, T, o_d);
    }
    break;
  }
  HIPCHK(hipGetLastError());
  if (beta_d) {
    hipLaunchKernelGGL(null_panel_beta_kernel, grid, block, 0, s, (int)n, (int)n_cvt, T, eval_d, UtWt_d, Yt_d, o_d, beta_d, se_d);
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

static int null_panel_wt(size_t n, size_t c, const double *UtW_d, DevBuf &dWt, hipStream_t s) {
  if (dWt.reserve(n * c * 8)) return fail(GEMMA_HIP_ENOMEM, "lmm_null_panel: U^T W transposed (%zu bytes)", n * c * 8);
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((c + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, UtW_d, (long)n,
                     (long)c, (long)c, dWt.as<double>(), (long)n);
  HIPCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_lmm_null_panel_d(size_t n, size_t n_cvt, size_t T, const double *eval_d, const double *UtW_d,
                                          const double *UtY_d, double l_min, double l_max, size_t n_region, double trace_G,
                                          gemma_null_fit *fit_d, double *beta_d, double *se_beta_d, void *stream) {
  NEED_INIT();
  int rc = null_panel_check(n, n_cvt, T, eval_d, UtW_d, UtY_d, l_min, l_max, n_region, fit_d, beta_d, se_beta_d);
  if (rc) return rc;
  hipStream_t s = S(stream);
  ScopedBuf dWt, dYt, dO;
  auto body = [&]() -> int {
    int r = null_panel_wt(n, n_cvt, UtW_d, dWt, s);
    if (r) return r;
    const size_t per_col = n * 8 + sizeof(NullOut);
    const size_t chunk = null_panel_chunk(T, per_col);
    if (dYt.reserve(chunk * n * 8) || dO.reserve(chunk * sizeof(NullOut)))
      return fail(GEMMA_HIP_ENOMEM, "lmm_null_panel: a chunk of %zu phenotypes does not fit (%zu bytes)", chunk, chunk * per_col);
    for (size_t t0 = 0; t0 < T; t0 += chunk) {
      const size_t Tc = std::min(chunk, T - t0);
      if ((r = null_panel_launch(n, n_cvt, Tc, eval_d, dWt.as<double>(), UtY_d + t0, T, dYt.as<double>(), l_min, l_max, n_region,
                                 dO.as<NullOut>(), beta_d ? beta_d + t0 * n_cvt : nullptr,
                                 se_beta_d ? se_beta_d + t0 * n_cvt : nullptr, s)))
        return r;
      hipLaunchKernelGGL(null_panel_derive_kernel, dim3((unsigned)((Tc + 255) / 256)), dim3(256), 0, s,
                         (const NullOut *)dO.as<NullOut>(), (int)Tc, trace_G, (double)(n - n_cvt), reinterpret_cast<NullFit8 *>(fit_d + t0));
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipStreamSynchronize(s)); // the call's own buffers go with it
    return GEMMA_HIP_OK;
  };
  rc = body();
  if (rc) (void)hipStreamSynchronize(s); // before the buffers go
  return rc;
}

extern "C" int gemma_hip_lmm_null_panel(size_t n, size_t n_cvt, size_t T, const double *eval, const double *UtW, const double *UtY,
                                        double l_min, double l_max, size_t n_region, double trace_G, gemma_null_fit *fit,
                                        double *beta, double *se_beta) {
  NEED_INIT();
  int rc = null_panel_check(n, n_cvt, T, eval, UtW, UtY, l_min, l_max, n_region, fit, beta, se_beta);
  if (rc) return rc;
  ScopedBuf dE, dW, dWt, dY, dYt, dO, dB;
  auto body = [&]() -> int {
    if (dE.reserve(n * 8) || dW.reserve(n * n_cvt * 8))
      return fail(GEMMA_HIP_ENOMEM, "lmm_null_panel: eval and U^T W (%zu bytes)", n * 8 + n * n_cvt * 8);
    HIPCHK(hipMemcpy(dE.p, eval, n * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dW.p, UtW, n * n_cvt * 8, hipMemcpyHostToDevice));
    int r = null_panel_wt(n, n_cvt, dW.as<double>(), dWt, 0);
    if (r) return r;
    const size_t b_col = beta ? 2 * n_cvt * 8 : 0;
    const size_t per_col = 2 * n * 8 + sizeof(NullOut) + b_col;
    const size_t chunk = null_panel_chunk(T, per_col);
    if (dY.reserve(chunk * n * 8) || dYt.reserve(chunk * n * 8) || dO.reserve(chunk * sizeof(NullOut)) ||
        (beta && dB.reserve(chunk * b_col)))
      return fail(GEMMA_HIP_ENOMEM, "lmm_null_panel: a chunk of %zu phenotypes does not fit (%zu bytes)", chunk, chunk * per_col);
    std::vector<NullOut> h(chunk);
    for (size_t t0 = 0; t0 < T; t0 += chunk) {
      const size_t Tc = std::min(chunk, T - t0);
      HIPCHK(hipMemcpy2D(dY.p, Tc * 8, UtY + t0, T * 8, Tc * 8, n, hipMemcpyHostToDevice));
      double *b_d = beta ? dB.as<double>() : nullptr, *s_d = beta ? dB.as<double>() + Tc * n_cvt : nullptr;
      if ((r = null_panel_launch(n, n_cvt, Tc, dE.as<double>(), dWt.as<double>(), dY.as<double>(), Tc, dYt.as<double>(), l_min, l_max,
                                 n_region, dO.as<NullOut>(), b_d, s_d, 0)))
        return r;
      HIPCHK(hipMemcpy(h.data(), dO.p, Tc * sizeof(NullOut), hipMemcpyDeviceToHost));
      if (beta) {
        HIPCHK(hipMemcpy(beta + t0 * n_cvt, b_d, Tc * n_cvt * 8, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(se_beta + t0 * n_cvt, s_d, Tc * n_cvt * 8, hipMemcpyDeviceToHost));
      }
      for (size_t k = 0; k < Tc; ++k) null_derive(h[k], trace_G, n, n_cvt, reinterpret_cast<double *>(fit + t0 + k)); // a gemma_null_fit is out8
    }
    return GEMMA_HIP_OK;
  };
  rc = body();
  if (rc) (void)hipDeviceSynchronize(); // before the buffers go
  return rc;
}

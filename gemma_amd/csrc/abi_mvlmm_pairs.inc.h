// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace).
// This part: the standard errors of the multivariate null block (gemma_hip_mvlmm_null_se, over mv_null_body of abi_mvlmm.inc.h) and
// the two-trait null fits of a whole panel (gemma_hip_mvlmm_null_pairs / _d; kernels in mvlmm_kernels_pair.hip).
//
// The pair panel is stateless like gemma_hip_lmm_null_panel: the buffers are the call's own, no LMM setup is needed or disturbed.
// Flow: U^T W and U^T Y transposed once; the univariate REML starts of all T columns from ONE null-panel call (vg_remle, ve_remle:
// the diagonals MphInitial takes, src/mvlmm.cpp:2780-2797); then per chunk of pairs a gather of the two rows of every pair into a
// slab (16 n bytes per pair), one launch of mvlmm_pair_null_kernel (one wavefront per pair) and one of mvpair_finish_kernel.

static_assert(sizeof(gemma_mvpair_fit) == sizeof(MvPairFit) && sizeof(gemma_mvpair_block) == sizeof(MvPairBlock) &&
                  sizeof(gemma_mvpair_fit) == 16 + 2 * 17 * 8,
              "gemma_mvpair_fit is MvPairFit of mvlmm_pair.h");
static_assert(GEMMA_MV_DMAX == MV_DMAX && GEMMA_MV_CMAX == MV_CMAX, "the se arrays are sized by the kernels' caps");

extern "C" int gemma_hip_mvlmm_null_se(size_t n, size_t n_cvt, size_t d, const double *eval, const double *UtW, const double *UtY,
                                       double l_min, double l_max, size_t n_region, const gemma_mvlmm_opt *opt, gemma_mvlmm_null *out,
                                       gemma_mvlmm_null_se *se) {
  if (!se) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_se: null pointer");
  return mv_null_body(n, n_cvt, d, eval, UtW, UtY, l_min, l_max, n_region, opt, out, se);
}

static int mvpairs_check(size_t n, size_t n_cvt, size_t T, const void *eval, const void *UtW, const void *UtY, const void *pairs,
                         size_t m, const void *fit, const void *B, const void *VB) {
  if (!eval || !UtW || !UtY || !fit) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: null pointer");
  if ((B == nullptr) != (VB == nullptr)) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: B and VB come together (both or neither)");
  if (T < 2 || T > (size_t)INT_MAX - 64) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: T=%zu traits (at least 2)", T);
  if (n_cvt < 1 || n_cvt > (size_t)MV_PAIR_CMAX)
    return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: n_cvt=%zu covariates (1..%d: the fixed two-trait instances)", n_cvt, MV_PAIR_CMAX);
  if (n <= n_cvt + 1) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: n <= n_cvt + 1");
  if (n > (size_t)INT_MAX) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: n=%zu individuals", n);
  if (pairs && m == 0) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: an empty list of pairs");
  if (!pairs && m != 0 && m != T * (T - 1) / 2)
    return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: m=%zu without a list (0 or T (T - 1) / 2 = %zu)", m, T * (T - 1) / 2);
  if (m > (size_t)INT_MAX) return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: m=%zu pairs", m);
  return GEMMA_HIP_OK;
}

// the host copy of the list: the caller's, checked, or all i < j row by row
static int mvpairs_list(size_t T, const int *pairs, size_t m, std::vector<int> &out) {
  if (!pairs) {
    out.reserve(T * (T - 1));
    for (size_t i = 0; i < T; ++i)
      for (size_t j = i + 1; j < T; ++j) {
        out.push_back((int)i);
        out.push_back((int)j);
      }
    return GEMMA_HIP_OK;
  }
  for (size_t q = 0; q < m; ++q) {
    const long i = pairs[2 * q], j = pairs[2 * q + 1];
    if (i < 0 || i >= j || j >= (long)T)
      return fail(GEMMA_HIP_EINVAL, "mvlmm_null_pairs: pair %zu is (%ld, %ld): 0 <= i < j < T=%zu", q, i, j, T);
  }
  out.assign(pairs, pairs + 2 * m);
  return GEMMA_HIP_OK;
}

// pairs per chunk: GEMMA_HIP_MVPAIR_CHUNK, else what half of the free memory holds at bytes_per_pair
static size_t mvpairs_chunk(size_t m, size_t bytes_per_pair) {
  const char *e = getenv("GEMMA_HIP_MVPAIR_CHUNK");
  if (e && *e) {
    const long long v = atoll(e);
    if (v > 0) return std::min(m, (size_t)v);
  }
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
    (void)hipGetLastError();
    return m;
  }
  return std::min(m, std::max<size_t>(free_b / 2 / bytes_per_pair, 1));
}

// wavefronts (= pairs) per workgroup: one, unless GEMMA_HIP_MVPAIR_WAVES=4 (read at the call; scripts/pair_panel_probe.py).  A
// workgroup lives as long as its slowest pair: at 8128 pairs four per workgroup cost 632 ms against 503 ms.
static int mvpairs_waves() {
  const char *e = getenv("GEMMA_HIP_MVPAIR_WAVES");
  return (e && e[0] == '4' && !e[1]) ? 4 : 1;
}

// Everything on the device.  list: the checked host copy of the pairs.  to_host: fit / B / VB are host pointers, filled chunk by
// chunk; else device pointers written in place.
static int mvpairs_run(size_t n, size_t c, size_t T, const double *eval_d, const double *UtW_d, const double *UtY_d,
                       const std::vector<int> &list, double l_min, double l_max, size_t n_region, const gemma_mvlmm_opt *opt,
                       gemma_mvpair_fit *fit, double *B, double *VB, bool to_host, hipStream_t s) {
  const size_t m = list.size() / 2;
  gemma_mvlmm_opt o;
  mv_default_opt(o, opt);
  ScopedBuf dWt, dYt, dStart, dPairs, dYp, dRaw, dFit, dB;
  auto body = [&]() -> int {
    int r = null_panel_wt(n, c, UtW_d, dWt, s);
    if (r) return r;
    if (dYt.reserve(T * n * 8) || dStart.reserve(T * sizeof(gemma_null_fit)) || dPairs.reserve(2 * m * sizeof(int)))
      return fail(GEMMA_HIP_ENOMEM, "mvlmm_null_pairs: U^T Y transposed, the starts and the list (%zu bytes)",
                  T * n * 8 + T * sizeof(gemma_null_fit) + 2 * m * sizeof(int));
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((T + 31) / 32), (unsigned)((n + 31) / 32)), dim3(32, 8), 0, s, UtY_d, (long)n,
                       (long)T, (long)T, dYt.as<double>(), (long)n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dPairs.p, list.data(), 2 * m * sizeof(int), hipMemcpyHostToDevice, s));
    // the univariate starts of every column: one launch (synchronises s, so `list` may be a pageable vector)
    if ((r = gemma_hip_lmm_null_panel_d(n, c, T, eval_d, UtW_d, UtY_d, l_min, l_max, n_region, 1.0, dStart.as<gemma_null_fit>(), nullptr,
                                        nullptr, s)))
      return r;
    const size_t raw = (size_t)mv_pair_raw_doubles((int)c), b_pair = B ? 2 * 2 * c : 0;
    const size_t per_pair = 2 * n * 8 + raw * 8 + (to_host ? sizeof(gemma_mvpair_fit) + 2 * b_pair * 8 : 0);
    const size_t chunk = mvpairs_chunk(m, per_pair);
    if (dYp.reserve(chunk * 2 * n * 8) || dRaw.reserve(chunk * raw * 8) ||
        (to_host && (dFit.reserve(chunk * sizeof(gemma_mvpair_fit)) || (B && dB.reserve(chunk * 2 * b_pair * 8)))))
      return fail(GEMMA_HIP_ENOMEM, "mvlmm_null_pairs: a chunk of %zu pairs does not fit (%zu bytes)", chunk, chunk * per_pair);
    const int waves = mvpairs_waves();
    for (size_t q0 = 0; q0 < m; q0 += chunk) {
      const size_t mc = std::min(chunk, m - q0);
      MvPairArgs p;
      p.n = (int)n;
      p.c = (int)c;
      p.m = (long)mc;
      p.eval = eval_d;
      p.Wt = dWt.as<double>();
      p.Yp = dYp.as<double>();
      p.pairs = dPairs.as<int>() + 2 * q0;
      p.start = dStart.as<double>();
      p.em_iter = (int)o.em_iter;
      p.nr_iter = (int)o.nr_iter;
      p.em_prec = o.em_prec;
      p.nr_prec = o.nr_prec;
      p.raw = dRaw.as<double>();
      MvPairFit *f_d = reinterpret_cast<MvPairFit *>(to_host ? dFit.as<gemma_mvpair_fit>() : fit + q0);
      double *b_d = !B ? nullptr : to_host ? dB.as<double>() : B + q0 * b_pair;
      double *vb_d = !B ? nullptr : to_host ? dB.as<double>() + mc * b_pair : VB + q0 * b_pair;
      int lrc = gemma_hip_mvpair_gather_launch_(dYt.as<double>(), (long)n, p.pairs, p.m, dYp.as<double>(), s);
      if (!lrc) lrc = gemma_hip_mvpair_launch_(&p, waves, s);
      if (!lrc) lrc = gemma_hip_mvpair_finish_launch_(&p, f_d, b_d, vb_d, s);
      if (lrc) return fail(GEMMA_HIP_ERUNTIME, "mvlmm_null_pairs launch: %s", hipGetErrorString((hipError_t)lrc));
      if (to_host) {
        HIPCHK(hipMemcpyAsync(fit + q0, dFit.p, mc * sizeof(gemma_mvpair_fit), hipMemcpyDeviceToHost, s));
        if (B) {
          HIPCHK(hipMemcpyAsync(B + q0 * b_pair, b_d, mc * b_pair * 8, hipMemcpyDeviceToHost, s));
          HIPCHK(hipMemcpyAsync(VB + q0 * b_pair, vb_d, mc * b_pair * 8, hipMemcpyDeviceToHost, s));
        }
        HIPCHK(hipStreamSynchronize(s)); // the chunk buffers are reused
      }
    }
    HIPCHK(hipStreamSynchronize(s)); // the call's own buffers go with it
    return GEMMA_HIP_OK;
  };
  int rc = body();
  if (rc) (void)hipStreamSynchronize(s); // before the buffers go
  return rc;
}

extern "C" int gemma_hip_mvlmm_null_pairs_d(size_t n, size_t n_cvt, size_t T, const double *eval_d, const double *UtW_d,
                                            const double *UtY_d, const int *pairs_d, size_t m, double l_min, double l_max,
                                            size_t n_region, const gemma_mvlmm_opt *opt, gemma_mvpair_fit *fit_d, double *B_d,
                                            double *VB_d, void *stream) {
  NEED_INIT();
  int rc = mvpairs_check(n, n_cvt, T, eval_d, UtW_d, UtY_d, pairs_d, m, fit_d, B_d, VB_d);
  if (rc) return rc;
  hipStream_t s = S(stream);
  std::vector<int> host, list;
  if (pairs_d) { // the list is checked on the host: 8 bytes per pair
    host.resize(2 * m);
    HIPCHK(hipMemcpyAsync(host.data(), pairs_d, 2 * m * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if ((rc = mvpairs_list(T, pairs_d ? host.data() : nullptr, m, list))) return rc;
  return mvpairs_run(n, n_cvt, T, eval_d, UtW_d, UtY_d, list, l_min, l_max, n_region, opt, fit_d, B_d, VB_d, false, s);
}

extern "C" int gemma_hip_mvlmm_null_pairs(size_t n, size_t n_cvt, size_t T, const double *eval, const double *UtW, const double *UtY,
                                          const int *pairs, size_t m, double l_min, double l_max, size_t n_region,
                                          const gemma_mvlmm_opt *opt, gemma_mvpair_fit *fit, double *B, double *VB) {
  NEED_INIT();
  int rc = mvpairs_check(n, n_cvt, T, eval, UtW, UtY, pairs, m, fit, B, VB);
  if (rc) return rc;
  std::vector<int> list;
  if ((rc = mvpairs_list(T, pairs, m, list))) return rc;
  ScopedBuf dE, dW, dY;
  if (dE.reserve(n * 8) || dW.reserve(n * n_cvt * 8) || dY.reserve(n * T * 8))
    return fail(GEMMA_HIP_ENOMEM, "mvlmm_null_pairs: eval, U^T W and U^T Y (%zu bytes)", n * 8 + n * n_cvt * 8 + n * T * 8);
  HIPCHK(hipMemcpy(dE.p, eval, n * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dW.p, UtW, n * n_cvt * 8, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dY.p, UtY, n * T * 8, hipMemcpyHostToDevice));
  return mvpairs_run(n, n_cvt, T, dE.as<double>(), dW.as<double>(), dY.as<double>(), list, l_min, l_max, n_region, opt, fit, B, VB,
                     true, 0);
}

// ------------------------------------------------------------------------------ variance components (-vc 1 / -vc 2)
// Textual part of gemma_hip.hip: argument checks and error text around the variance-component unit (vc_tu.hip).

extern "C" int gemma_hip_spd_inverse_d(double *A_d, size_t n, size_t lda, double *logdet, long *bad_pivot, void *stream) {
  NEED_INIT();
  if (n == 0 || lda < n || !A_d) return fail(GEMMA_HIP_EINVAL, "spd_inverse: n = %zu, lda = %zu", n, lda);
  std::string msg;
  const int rc = spd_inverse_x(A_d, (long)n, (long)lda, logdet, bad_pivot, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_spd_inverse(double *A, size_t n, size_t lda, double *logdet, long *bad_pivot) {
  NEED_INIT();
  if (n == 0 || lda < n || !A) return fail(GEMMA_HIP_EINVAL, "spd_inverse: n = %zu, lda = %zu", n, lda);
  const size_t ld = (n + 1) & ~(size_t)1;
  ScopedBuf d;
  if (d.reserve(n * ld * 8)) return fail(GEMMA_HIP_ENOMEM, "spd_inverse: cannot allocate %zu bytes", n * ld * 8);
  std::string msg;
  HIPCHK(hipMemcpy2D(d.p, ld * 8, A, lda * 8, n * 8, n, hipMemcpyHostToDevice));
  if (int rc = spd_inverse_x(d.as<double>(), (long)n, (long)ld, logdet, bad_pivot, nullptr, msg)) return ret(rc, msg);
  HIPCHK(hipMemcpy2D(A, lda * 8, d.p, ld * 8, n * 8, n, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}

static bool g_vc_ready = false;
static size_t g_vc_nvc = 0;

static int vc_setup_common(size_t n, size_t n_vc, const double *const *K, size_t ldk, const double *W, size_t n_cvt, const double *y,
                           bool device) {
  NEED_INIT();
  g_vc_ready = false;
  if (n < 2 || n_vc < 1 || n_vc > 8 || n_cvt < 1 || n_cvt > 64 || n_cvt >= n || ldk < n || !K || !W || !y)
    return fail(GEMMA_HIP_EINVAL, "vc_setup: n = %zu, n_vc = %zu (1..8), n_cvt = %zu (1..64), ldk = %zu", n, n_vc, n_cvt, ldk);
  for (size_t l = 0; l < n_vc; ++l)
    if (!K[l]) return fail(GEMMA_HIP_EINVAL, "vc_setup: kinship %zu is NULL", l);
  std::string msg;
  const int rc = vc_setup_x((long)n, (int)n_vc, K, (long)ldk, device, W, (int)n_cvt, y, msg);
  if (rc) {
    vc_release_x();
    return ret(rc, msg);
  }
  g_vc_ready = true;
  g_vc_nvc = n_vc;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_vc_setup(size_t n, size_t n_vc, const double *const *K, size_t ldk, const double *W, size_t n_cvt,
                                  const double *y) {
  return vc_setup_common(n, n_vc, K, ldk, W, n_cvt, y, false);
}

extern "C" int gemma_hip_vc_setup_d(size_t n, size_t n_vc, const double *const *K_d, size_t ldk, const double *W, size_t n_cvt,
                                    const double *y) {
  return vc_setup_common(n, n_vc, K_d, ldk, W, n_cvt, y, true);
}

static void vc_copy_out(const VcResult &r, double *sigma2, double *se_sigma2, double *pve, double *se_pve, double *pve_total,
                        double *se_pve_total) {
  for (size_t i = 0; i <= g_vc_nvc; ++i) {
    if (sigma2) sigma2[i] = r.sigma2[i];
    if (se_sigma2) se_sigma2[i] = r.se_sigma2[i];
  }
  for (size_t i = 0; i < g_vc_nvc; ++i) {
    if (pve) pve[i] = r.pve[i];
    if (se_pve) se_pve[i] = r.se_pve[i];
  }
  if (pve_total) *pve_total = r.pve_total;
  if (se_pve_total) *se_pve_total = r.se_pve_total;
}

extern "C" int gemma_hip_vc_he(double *sigma2, double *se_sigma2, double *pve, double *se_pve, double *pve_total, double *se_pve_total) {
  NEED_INIT();
  if (!g_vc_ready) return fail(GEMMA_HIP_ESTATE, "vc_he before vc_setup");
  VcResult r{};
  std::string msg;
  const int rc = vc_he_x(r, msg);
  if (rc) return ret(rc, msg);
  vc_copy_out(r, sigma2, se_sigma2, pve, se_pve, pve_total, se_pve_total);
  return GEMMA_HIP_OK;
}

static double g_vc_t5[5] = {0, 0, 0, 0, 0};

extern "C" int gemma_hip_vc_reml(int noconstrain, double *sigma2, double *se_sigma2, double *pve, double *se_pve, double *pve_total,
                                 double *se_pve_total, int *iterations, int *status, long *counts, double *iter_sigma2, size_t iter_cap) {
  NEED_INIT();
  if (!g_vc_ready) return fail(GEMMA_HIP_ESTATE, "vc_reml before vc_setup");
  VcResult r{};
  std::vector<double> it;
  std::string msg;
  const int rc = vc_reml_x(noconstrain != 0, r, &it, msg);
  if (rc) return ret(rc, msg);
  vc_copy_out(r, sigma2, se_sigma2, pve, se_pve, pve_total, se_pve_total);
  if (iterations) *iterations = r.iterations;
  if (status) *status = r.status;
  if (counts) {
    counts[0] = r.evaluations;
    counts[1] = r.inverses;
  }
  if (iter_sigma2) {
    const size_t rows = std::min(iter_cap, it.size() / (g_vc_nvc + 1));
    memcpy(iter_sigma2, it.data(), rows * (g_vc_nvc + 1) * 8);
  }
  g_vc_t5[0] = r.t_asm; g_vc_t5[1] = r.t_inv; g_vc_t5[2] = r.t_pcor; g_vc_t5[3] = r.t_mv; g_vc_t5[4] = r.t_tr;
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_vc_timing(double *t5) {
  if (!t5) return fail(GEMMA_HIP_EINVAL, "vc_timing: NULL");
  for (int i = 0; i < 5; ++i) t5[i] = g_vc_t5[i];
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_vc_release(void) {
  NEED_INIT();
  vc_release_x();
  g_vc_ready = false;
  return GEMMA_HIP_OK;
}

// ------------------------------------------------------------------------------ MQS summary statistics (-gs, -vc 1 -beta)
// Textual part of gemma_hip.hip: argument checks and error text around the MQS unit (mqs_tu.hip).

extern "C" int gemma_hip_mqs_begin(size_t ni_total, const int *indicator_idv, size_t n_vc, const double *W, size_t n_cvt, int slot) {
  NEED_INIT();
  if (ni_total == 0 || ni_total > (size_t)1 << 30 || !W) return fail(GEMMA_HIP_EINVAL, "mqs_begin: ni_total = %zu", ni_total);
  if (n_vc < 1 || n_vc > 8) return fail(GEMMA_HIP_EINVAL, "mqs_begin: n_vc = %zu (1..8)", n_vc);
  if (n_cvt < 1 || n_cvt > 64) return fail(GEMMA_HIP_EINVAL, "mqs_begin: n_cvt = %zu (1..64, with the intercept)", n_cvt);
  if (slot < 0 || slot > 2) return fail(GEMMA_HIP_EINVAL, "mqs_begin: slot = %d (0: K, 1: A, 2: A on top of the kept K)", slot);
  std::string msg;
  const int rc = mqs_begin_x((long)ni_total, indicator_idv, (int)n_vc, W, (int)n_cvt, slot, msg);
  return ret(rc, msg);
}

static int mqs_add_common(int geno_kind, const void *geno, size_t l, size_t ld, const int *cat, const double *weight, bool device,
                          void *stream) {
  if (!mqs_active_x()) return fail(GEMMA_HIP_EINVAL, "mqs_add before mqs_begin");
  if (l == 0) return GEMMA_HIP_OK;
  if (!cat) return fail(GEMMA_HIP_EINVAL, "mqs_add: cat is NULL");
  int rc = mv_check_block("mqs_add", geno_kind, geno, l, ld, (size_t)mqs_ni_total_x());
  if (rc) return rc;
  std::string msg;
  rc = mqs_add_x(geno_kind, geno, (long)l, (long)ld, cat, weight, device, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_mqs_add(int geno_kind, const void *geno, size_t l, size_t ld, const int *cat, const double *weight) {
  NEED_INIT();
  return mqs_add_common(geno_kind, geno, l, ld, cat, weight, false, nullptr);
}

extern "C" int gemma_hip_mqs_add_d(int geno_kind, const void *geno_d, size_t l, size_t ld, const int *cat_d, const double *weight_d,
                                   void *stream) {
  NEED_INIT();
  return mqs_add_common(geno_kind, geno_d, l, ld, cat_d, weight_d, true, stream);
}

extern "C" int gemma_hip_mqs_end(double *S, double *ns) {
  NEED_INIT();
  if (!mqs_active_x()) return fail(GEMMA_HIP_EINVAL, "mqs_end before mqs_begin");
  std::string msg;
  const int rc = mqs_end_x(S, ns, msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_mqs_get(int slot, size_t i_vc, double *out) {
  NEED_INIT();
  if (!out || i_vc >= 8) return fail(GEMMA_HIP_EINVAL, "mqs_get: matrix %zu", i_vc);
  std::string msg;
  const int rc = mqs_get_x(slot, (int)i_vc, out, msg);
  return ret(rc, msg);
}

static int mqs_S_check(size_t n, size_t n_vc, const double *A, const double *K, size_t ld, size_t n_cvt, const double *S) {
  if (n < 3 || n_vc < 1 || n_vc > 8 || !K || !S || ld < n || n_cvt < 1 || n_cvt > 64 || n_cvt + 1 >= n || !A)
    return fail(GEMMA_HIP_EINVAL, "mqs_S: n = %zu, n_vc = %zu (1..8), ld = %zu, n_cvt = %zu (1..64)", n, n_vc, ld, n_cvt);
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_mqs_S_d(size_t n, size_t n_vc, const double *A_d, const double *K_d, size_t ld, size_t n_cvt, double *S_out,
                                 void *stream) {
  NEED_INIT();
  int rc = mqs_S_check(n, n_vc, A_d, K_d, ld, n_cvt, S_out);
  if (rc) return rc;
  std::string msg;
  rc = mqs_S_x((long)n, (int)n_vc, A_d, K_d, (long)ld, (int)n_cvt, S_out, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_mqs_S(size_t n, size_t n_vc, const double *A, const double *K, size_t ld, size_t n_cvt, double *S) {
  NEED_INIT();
  int rc = mqs_S_check(n, n_vc, A, K, ld, n_cvt, S);
  if (rc) return rc;
  const bool same = (A == K);
  const size_t ldd = (n + 1) & ~(size_t)1, per = n * ldd;
  ScopedBuf d;
  if (d.reserve((same ? 1 : 2) * n_vc * per * 8)) return fail(GEMMA_HIP_ENOMEM, "mqs_S: cannot allocate %zu bytes", (same ? 1 : 2) * n_vc * per * 8);
  double *Kd = d.as<double>(), *Ad = same ? Kd : Kd + n_vc * per;
  for (size_t i = 0; i < n_vc; ++i) {
    HIPCHK(hipMemcpy2D(Kd + i * per, ldd * 8, K + i * n * ld, ld * 8, n * 8, n, hipMemcpyHostToDevice));
    if (!same) HIPCHK(hipMemcpy2D(Ad + i * per, ldd * 8, A + i * n * ld, ld * 8, n * 8, n, hipMemcpyHostToDevice));
  }
  std::string msg;
  rc = mqs_S_x((long)n, (int)n_vc, Ad, Kd, (long)ldd, (int)n_cvt, S, nullptr, msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_mqs_release(void) {
  NEED_INIT();
  mqs_release_x();
  return GEMMA_HIP_OK;
}

// ------------------------------------------------------------------------------ MQS confidence intervals (-ci 1, -ci 2)
extern "C" int gemma_hip_ci_begin(size_t ni_total, const int *indicator_idv, size_t n_vc) {
  NEED_INIT();
  if (ni_total == 0 || ni_total > (size_t)1 << 30) return fail(GEMMA_HIP_EINVAL, "ci_begin: ni_total = %zu", ni_total);
  if (n_vc < 1 || n_vc > 8) return fail(GEMMA_HIP_EINVAL, "ci_begin: n_vc = %zu (1..8)", n_vc);
  std::string msg;
  const int rc = ci_begin_x((long)ni_total, indicator_idv, (int)n_vc, msg);
  return ret(rc, msg);
}

static int ci_xwz_common(int geno_kind, const void *geno, size_t l, size_t ld, const int *cat, const double *z, const double *w,
                         size_t *n_skipped, bool device, void *stream) {
  if (ci_pass_x() != 1) return fail(GEMMA_HIP_EINVAL, "ci_xwz outside pass 1 (after ci_begin, before ci_xwz_end)");
  if (n_skipped) *n_skipped = 0;
  if (l == 0) return GEMMA_HIP_OK;
  if (!cat || !z) return fail(GEMMA_HIP_EINVAL, "ci_xwz: cat or z is NULL");
  int rc = mv_check_block("ci_xwz", geno_kind, geno, l, ld, (size_t)ci_ni_total_x());
  if (rc) return rc;
  std::string msg;
  rc = ci_xwz_x(geno_kind, geno, (long)l, (long)ld, cat, z, w, device, S(stream), n_skipped, msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_ci_xwz(int geno_kind, const void *geno, size_t l, size_t ld, const int *cat, const double *z, const double *w,
                                size_t *n_skipped) {
  NEED_INIT();
  return ci_xwz_common(geno_kind, geno, l, ld, cat, z, w, n_skipped, false, nullptr);
}

extern "C" int gemma_hip_ci_xwz_d(int geno_kind, const void *geno_d, size_t l, size_t ld, const int *cat_d, const double *z_d,
                                  const double *w_d, size_t *n_skipped, void *stream) {
  NEED_INIT();
  return ci_xwz_common(geno_kind, geno_d, l, ld, cat_d, z_d, w_d, n_skipped, true, stream);
}

extern "C" int gemma_hip_ci_xwz_end(double *Xz, double *XWz) {
  NEED_INIT();
  if (ci_pass_x() != 1) return fail(GEMMA_HIP_EINVAL, "ci_xwz_end outside pass 1 (after ci_begin, once)");
  std::string msg;
  const int rc = ci_xwz_end_x(Xz, XWz, msg);
  return ret(rc, msg);
}

static int ci_xtxwz_common(int geno_kind, const void *geno, size_t l, size_t ld, double *XtXWz, bool device, void *stream) {
  if (ci_pass_x() != 2) return fail(GEMMA_HIP_EINVAL, "ci_xtxwz before ci_xwz_end: pass 2 needs the finished XWz of pass 1");
  if (l == 0) return GEMMA_HIP_OK;
  if (!XtXWz) return fail(GEMMA_HIP_EINVAL, "ci_xtxwz: XtXWz is NULL");
  int rc = mv_check_block("ci_xtxwz", geno_kind, geno, l, ld, (size_t)ci_ni_total_x());
  if (rc) return rc;
  std::string msg;
  rc = ci_xtxwz_x(geno_kind, geno, (long)l, (long)ld, XtXWz, device, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_ci_xtxwz(int geno_kind, const void *geno, size_t l, size_t ld, double *XtXWz) {
  NEED_INIT();
  return ci_xtxwz_common(geno_kind, geno, l, ld, XtXWz, false, nullptr);
}

extern "C" int gemma_hip_ci_xtxwz_d(int geno_kind, const void *geno_d, size_t l, size_t ld, double *XtXWz_d, void *stream) {
  NEED_INIT();
  return ci_xtxwz_common(geno_kind, geno_d, l, ld, XtXWz_d, true, stream);
}

extern "C" int gemma_hip_ci_release(void) {
  NEED_INIT();
  ci_release_x();
  return GEMMA_HIP_OK;
}

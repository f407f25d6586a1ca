// ------------------------------------------------------------------------------ MQS summary statistics (-gs, -vc 1 -beta)
// Textual part of gemma_hip.hip: argument checks and error text around the MQS unit (mqs_tu.hip).

extern "C" int gemma_hip_mqs_begin(size_t ni_total, const int *indicator_idv, size_t n_vc, const double *W, size_t n_cvt, int slot) {
  NEED_INIT();
  if (ni_total == 0 || ni_total > (size_t)1 << 30 || !W) return fail(GEMMA_HIP_EINVAL, "mqs_begin: ni_total = %zu", ni_total);
  if (n_vc < 1 || n_vc > 8) return fail(GEMMA_HIP_EINVAL, "mqs_begin: n_vc = %zu (1..8)", n_vc);
  if (n_cvt < 1 || n_cvt > 64) return fail(GEMMA_HIP_EINVAL, "mqs_begin: n_cvt = %zu (1..64, with the intercept)", n_cvt);
  if (slot != 0 && slot != 1) return fail(GEMMA_HIP_EINVAL, "mqs_begin: slot = %d (0: K, 1: A)", slot);
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
  DevBuf d;
  if (d.reserve((same ? 1 : 2) * n_vc * per * 8)) return fail(GEMMA_HIP_ENOMEM, "mqs_S: cannot allocate %zu bytes", (same ? 1 : 2) * n_vc * per * 8);
  double *Kd = d.as<double>(), *Ad = same ? Kd : Kd + n_vc * per;
  hipError_t e = hipSuccess;
  for (size_t i = 0; i < n_vc && e == hipSuccess; ++i) {
    e = hipMemcpy2D(Kd + i * per, ldd * 8, K + i * n * ld, ld * 8, n * 8, n, hipMemcpyHostToDevice);
    if (e == hipSuccess && !same) e = hipMemcpy2D(Ad + i * per, ldd * 8, A + i * n * ld, ld * 8, n * 8, n, hipMemcpyHostToDevice);
  }
  std::string msg;
  if (e == hipSuccess) rc = mqs_S_x((long)n, (int)n_vc, Ad, Kd, (long)ldd, (int)n_cvt, S, nullptr, msg);
  d.release();
  if (e != hipSuccess) return fail(GEMMA_HIP_ERUNTIME, "mqs_S: %s", hipGetErrorString(e));
  return ret(rc, msg);
}

extern "C" int gemma_hip_mqs_release(void) {
  NEED_INIT();
  mqs_release_x();
  return GEMMA_HIP_OK;
}

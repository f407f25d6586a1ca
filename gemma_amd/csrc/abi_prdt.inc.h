// ------------------------------------------------------------------------------ genomic prediction (-bslmm 2, -predict 1 / 2)
// Textual part of gemma_hip.hip: argument checks and error text around the prediction unit (prdt_tu.hip).

static int ridge_setup_common(size_t n, const double *U, size_t ldu, const double *eval, bool ue_device, const double *Uty,
                              bool uty_device, double lambda, size_t ns_test, double *bv_out, void *stream) {
  if (n == 0 || ldu < n || !U || !eval || !Uty)
    return fail(GEMMA_HIP_EINVAL, "ridge_setup: n = %zu, ldu = %zu", n, ldu);
  if (ns_test == 0) return fail(GEMMA_HIP_EINVAL, "ridge_setup: ns_test = 0 (the effects are scaled by lambda / ns_test)");
  if (!(lambda >= 0.0)) return fail(GEMMA_HIP_EINVAL, "ridge_setup: lambda = %g", lambda);
  std::string msg;
  const int rc = ridge_setup_x((long)n, U, (long)ldu, eval, ue_device, Uty, uty_device, lambda, (long)ns_test, bv_out, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_ridge_setup(size_t n, const double *U, const double *eval, const double *Uty, double lambda, size_t ns_test,
                                     double *bv_out) {
  NEED_INIT();
  return ridge_setup_common(n, U, n, eval, false, Uty, false, lambda, ns_test, bv_out, nullptr);
}

extern "C" int gemma_hip_ridge_setup_d(size_t n, const double *U_d, size_t ldu, const double *eval_d, const double *Uty_d, double lambda,
                                       size_t ns_test, double *bv_out_d, void *stream) {
  NEED_INIT();
  return ridge_setup_common(n, U_d, ldu, eval_d, true, Uty_d, true, lambda, ns_test, bv_out_d, stream);
}

extern "C" int gemma_hip_ridge_setup_kept(const double *Uty, double lambda, size_t ns_test, double *bv_out) {
  NEED_INIT();
  const size_t n = g_ctx.kept_n;
  if (n == 0 || !g_ctx.kept_UE.p) return fail(GEMMA_HIP_ESTATE, "ridge_setup_kept before eigh_kept_K / eigh_keep");
  const double *U = g_ctx.kept_UE.as<double>();
  return ridge_setup_common(n, U, n, U + n * n, true, Uty, false, lambda, ns_test, bv_out, nullptr);
}

extern "C" int gemma_hip_ridge_set_r(size_t n, const double *r, double scale) {
  NEED_INIT();
  if (n == 0 || !r) return fail(GEMMA_HIP_EINVAL, "ridge_set_r: n = %zu", n);
  std::string msg;
  const int rc = ridge_set_r_x((long)n, r, scale, msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_ridge_set_indicator(const int *indicator_idv, size_t ni_total) {
  NEED_INIT();
  if (!ridge_ready_x()) return fail(GEMMA_HIP_ESTATE, "ridge_set_indicator before ridge_setup");
  if (!indicator_idv || ni_total == 0) return fail(GEMMA_HIP_EINVAL, "ridge_set_indicator: ni_total = %zu", ni_total);
  if (ni_total < ridge_n_x())
    return fail(GEMMA_HIP_EINVAL, "ridge_set_indicator: %zu analysed individuals, ni_total = %zu", ridge_n_x(), ni_total);
  std::string msg;
  const int rc = ridge_set_indicator_x(indicator_idv, (long)ni_total, msg);
  return ret(rc, msg);
}

static int mv_check_block(const char *who, int geno_kind, const void *geno, size_t l, size_t ld, size_t ni_total) {
  if (geno_kind != GEMMA_GENO_PLINK_2BIT && geno_kind != GEMMA_GENO_F64_SNP_MAJOR)
    return fail(GEMMA_HIP_EINVAL, "%s: genotype kind %d (SNP-major fp64 or PLINK 2-bit rows)", who, geno_kind);
  const size_t need = geno_kind == GEMMA_GENO_PLINK_2BIT ? (ni_total + 3) / 4 : ni_total;
  if (!geno || ld < need) return fail(GEMMA_HIP_EINVAL, "%s: ld = %zu, a row of %zu individuals takes %zu", who, ld, ni_total, need);
  if (l > (size_t)1 << 30) return fail(GEMMA_HIP_EINVAL, "%s: l = %zu", who, l);
  return GEMMA_HIP_OK;
}

static int ridge_batch_common(int geno_kind, const void *geno, size_t l, size_t ld, bool device, double *alpha_out, void *stream) {
  if (!ridge_ready_x()) return fail(GEMMA_HIP_ESTATE, "ridge_batch before ridge_setup");
  if (l == 0) return GEMMA_HIP_OK;
  if (!alpha_out) return fail(GEMMA_HIP_EINVAL, "ridge_batch: alpha_out is NULL");
  int rc = mv_check_block("ridge_batch", geno_kind, geno, l, ld, ridge_ni_total_x());
  if (rc) return rc;
  std::string msg;
  rc = ridge_batch_x(geno_kind, geno, (long)l, (long)ld, device, alpha_out, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_ridge_batch(int geno_kind, const void *geno, size_t l, size_t ld, double *alpha_out) {
  NEED_INIT();
  return ridge_batch_common(geno_kind, geno, l, ld, false, alpha_out, nullptr);
}

extern "C" int gemma_hip_ridge_batch_d(int geno_kind, const void *geno_d, size_t l, size_t ld, double *alpha_out_d, void *stream) {
  NEED_INIT();
  return ridge_batch_common(geno_kind, geno_d, l, ld, true, alpha_out_d, stream);
}

extern "C" int gemma_hip_ridge_finish(void) {
  NEED_INIT();
  ridge_finish_x();
  return GEMMA_HIP_OK;
}

extern "C" int gemma_hip_prdt_begin(const int *indicator_idv, size_t ni_total) {
  NEED_INIT();
  if (!indicator_idv || ni_total == 0) return fail(GEMMA_HIP_EINVAL, "prdt_begin: ni_total = %zu", ni_total);
  std::string msg;
  const int rc = prdt_begin_x(indicator_idv, (long)ni_total, msg);
  return ret(rc, msg);
}

static int prdt_add_common(int geno_kind, const void *geno, size_t l, size_t ld, bool device, const double *effect, int *used_out,
                           void *stream) {
  if (!prdt_active_x()) return fail(GEMMA_HIP_ESTATE, "prdt_add before prdt_begin");
  if (l == 0) return GEMMA_HIP_OK;
  if (!effect) return fail(GEMMA_HIP_EINVAL, "prdt_add: effect is NULL");
  int rc = mv_check_block("prdt_add", geno_kind, geno, l, ld, prdt_ni_total_x());
  if (rc) return rc;
  std::string msg;
  rc = prdt_add_x(geno_kind, geno, (long)l, (long)ld, device, effect, used_out, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_prdt_add(int geno_kind, const void *geno, size_t l, size_t ld, const double *effect, int *used_out) {
  NEED_INIT();
  return prdt_add_common(geno_kind, geno, l, ld, false, effect, used_out, nullptr);
}

extern "C" int gemma_hip_prdt_add_d(int geno_kind, const void *geno_d, size_t l, size_t ld, const double *effect_d, int *used_out_d,
                                    void *stream) {
  NEED_INIT();
  return prdt_add_common(geno_kind, geno_d, l, ld, true, effect_d, used_out_d, stream);
}

static int prdt_add_bv_common(const double *G, size_t ni_total, size_t ldg, bool device, const double *u_hat, size_t n_bv, void *stream) {
  if (!prdt_active_x()) return fail(GEMMA_HIP_ESTATE, "prdt_add_bv before prdt_begin");
  if (!G || !u_hat || ldg < ni_total) return fail(GEMMA_HIP_EINVAL, "prdt_add_bv: ni_total = %zu, ldg = %zu", ni_total, ldg);
  if (ni_total != prdt_ni_total_x())
    return fail(GEMMA_HIP_EINVAL, "prdt_add_bv: G is %zu x %zu, prdt_begin counted %zu individuals", ni_total, ni_total, prdt_ni_total_x());
  if (n_bv != prdt_n_train_x())
    return fail(GEMMA_HIP_EINVAL, "prdt_add_bv: %zu breeding values, %zu training individuals", n_bv, prdt_n_train_x());
  if (n_bv > 65535 || ni_total - n_bv > 65535) return fail(GEMMA_HIP_EINVAL, "prdt_add_bv: more than 65535 individuals in a group");
  std::string msg;
  const int rc = prdt_add_bv_x(G, (long)ni_total, (long)ldg, device, u_hat, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_prdt_add_bv(const double *G, size_t ni_total, const double *u_hat, size_t n_bv) {
  NEED_INIT();
  return prdt_add_bv_common(G, ni_total, ni_total, false, u_hat, n_bv, nullptr);
}

extern "C" int gemma_hip_prdt_add_bv_d(const double *G_d, size_t ni_total, size_t ldg, const double *u_hat, size_t n_bv, void *stream) {
  NEED_INIT();
  return prdt_add_bv_common(G_d, ni_total, ldg, true, u_hat, n_bv, stream);
}

extern "C" int gemma_hip_prdt_end(double pheno_mean, int probit, double *y_prdt) {
  NEED_INIT();
  if (!prdt_active_x()) return fail(GEMMA_HIP_ESTATE, "prdt_end before prdt_begin");
  if (!y_prdt && prdt_ni_total_x() > prdt_n_train_x()) return fail(GEMMA_HIP_EINVAL, "prdt_end: y_prdt is NULL");
  std::string msg;
  const int rc = prdt_end_x(pheno_mean, probit, y_prdt, msg);
  return ret(rc, msg);
}

// Mode 43 for one phenotype (src/gemma.cpp:1732-1820, :1873-1882 with PRDT::MvnormPrdt, src/prdt.cpp:448-553): every dense step
// goes through the entry points that exist -- centring, eigensolver, U'W and U'y, the REML null fit, the SPD inverse and the GEMM.
extern "C" int gemma_hip_prdt_kin(size_t ni, const double *G_full, const int *indicator_pheno, const double *W_full, size_t n_cvt,
                                  const double *y_full, double l_min, double l_max, size_t n_region, double *y_miss, double *fit3) {
  NEED_INIT();
  if (ni == 0 || !G_full || !indicator_pheno || !W_full || !y_full || n_cvt == 0)
    return fail(GEMMA_HIP_EINVAL, "prdt_kin: ni = %zu, n_cvt = %zu", ni, n_cvt);
  std::vector<size_t> po, pm;
  for (size_t i = 0; i < ni; ++i) (indicator_pheno[i] != 0 ? po : pm).push_back(i);
  const size_t n = po.size(), m = pm.size(), c = n_cvt;
  if (n <= c) return fail(GEMMA_HIP_EINVAL, "prdt_kin: %zu observed phenotypes, %zu covariates", n, c);
  if (m > 0 && !y_miss) return fail(GEMMA_HIP_EINVAL, "prdt_kin: y_miss is NULL");
  int rc;
  // G over the observed individuals and G_full, each centred by CenterMatrix (:1772-1773)
  std::vector<double> G(n * n), Gf(G_full, G_full + ni * ni), W(n * c), y(n);
  for (size_t a = 0; a < n; ++a) {
    for (size_t b = 0; b < n; ++b) G[a * n + b] = G_full[po[a] * ni + po[b]];
    for (size_t k = 0; k < c; ++k) W[a * c + k] = W_full[po[a] * c + k];
    y[a] = y_full[po[a]];
  }
  if ((rc = gemma_hip_center(G.data(), n)) || (rc = gemma_hip_center(Gf.data(), ni))) return rc;
  // EigenDecomp_Zeroed, CalcUtX of W and y, CalcLambda 'R', CalcLmmVgVeBeta (:1779-1801)
  std::vector<double> U(n * n), ev(n), UtW(n * c), Uty(n);
  double trace_G = 0.0, null8[8];
  if ((rc = gemma_hip_eigh(G.data(), n, U.data(), ev.data(), &trace_G))) return rc;
  if ((rc = gemma_hip_calc_utx(U.data(), W.data(), n, c, UtW.data())) || (rc = gemma_hip_calc_utx(U.data(), y.data(), n, 1, Uty.data())))
    return rc;
  if ((rc = gemma_hip_lmm_null(n, c, ev.data(), UtW.data(), Uty.data(), l_min, l_max, n_region, trace_G, null8))) return rc;
  const double lambda = null8[2], vg = null8[6], ve = null8[7];
  // beta = (W' H^-1 W)^-1 W' H^-1 y in the eigenbasis (c x c, on the host: src/lmm.cpp:2208-2256)
  std::vector<double> A(c * (c + 1), 0.0), beta(c);
  for (size_t i = 0; i < n; ++i) {
    const double h = 1.0 / (lambda * ev[i] + 1.0);
    for (size_t a = 0; a < c; ++a) {
      for (size_t b = 0; b < c; ++b) A[a * (c + 1) + b] += UtW[i * c + a] * h * UtW[i * c + b];
      A[a * (c + 1) + c] += UtW[i * c + a] * h * Uty[i];
    }
  }
  for (size_t k = 0; k < c; ++k) { // Gauss-Jordan with partial pivoting
    size_t p = k;
    for (size_t i = k + 1; i < c; ++i)
      if (fabs(A[i * (c + 1) + k]) > fabs(A[p * (c + 1) + k])) p = i;
    if (A[p * (c + 1) + k] == 0.0) return fail(GEMMA_HIP_EINVAL, "prdt_kin: the covariates are collinear");
    for (size_t j = 0; j <= c; ++j) std::swap(A[k * (c + 1) + j], A[p * (c + 1) + j]);
    for (size_t i = 0; i < c; ++i) {
      if (i == k) continue;
      const double f = A[i * (c + 1) + k] / A[k * (c + 1) + k];
      for (size_t j = k; j <= c; ++j) A[i * (c + 1) + j] -= f * A[k * (c + 1) + j];
    }
  }
  for (size_t k = 0; k < c; ++k) beta[k] = A[k * (c + 1) + c] / A[k * (c + 1) + k];
  if (fit3) { fit3[0] = vg; fit3[1] = ve; fit3[2] = lambda; }
  if (m == 0) return GEMMA_HIP_OK;
  // H = ve I + vg G_full (:1813-1816); y_miss = W_miss beta + H_mo H_oo^-1 (y_obs - W_obs beta)
  std::vector<double> Hoo(n * n), Hmo(m * n), res(n), x(n);
  for (size_t a = 0; a < n; ++a) {
    for (size_t b = 0; b < n; ++b) Hoo[a * n + b] = vg * Gf[po[a] * ni + po[b]] + (a == b ? ve : 0.0);
    double f = 0.0;
    for (size_t k = 0; k < c; ++k) f += W[a * c + k] * beta[k];
    res[a] = y[a] - f;
  }
  for (size_t a = 0; a < m; ++a) {
    for (size_t b = 0; b < n; ++b) Hmo[a * n + b] = vg * Gf[pm[a] * ni + po[b]];
    double f = 0.0;
    for (size_t k = 0; k < c; ++k) f += W_full[pm[a] * c + k] * beta[k];
    y_miss[a] = f;
  }
  double logdet = 0.0;
  long bad = -1;
  if ((rc = gemma_hip_spd_inverse(Hoo.data(), n, n, &logdet, &bad))) return rc;
  if ((rc = gemma_hip_dgemm('N', 'N', n, 1, n, 1.0, Hoo.data(), n, res.data(), 1, 0.0, x.data(), 1))) return rc;
  return gemma_hip_dgemm('N', 'N', m, 1, n, 1.0, Hmo.data(), n, x.data(), 1, 1.0, y_miss, 1);
}

// Mode 43 for several phenotypes: the Kronecker system on the device (prdt_mv.hip.h), see include/gemma_hip.h
static int prdt_kin_mv_check(const char *who, size_t ni, size_t d, const double *G, size_t ldg, const int *ind, const double *W, size_t c,
                             const double *Y, size_t extra, size_t *n_miss) {
  if (ni == 0 || !G || !ind || !W || !Y || ldg < ni) return fail(GEMMA_HIP_EINVAL, "%s: ni = %zu, ldg = %zu or a null pointer", who, ni, ldg);
  if (d < 2) return fail(GEMMA_HIP_EINVAL, "%s: %zu phenotypes (2..%d)", who, d, MV_DMAX);
  int rc = mv_check_dims(who, d, c, extra);
  if (rc) return rc;
  if (ni > 65535) return fail(GEMMA_HIP_EINVAL, "%s: more than 65535 individuals", who);
  size_t m = 0;
  for (size_t k = 0; k < ni * d; ++k) m += ind[k] == 0;
  if (m == ni * d) return fail(GEMMA_HIP_EINVAL, "%s: no phenotype is observed", who);
  *n_miss = m;
  return GEMMA_HIP_OK;
}

static int prdt_kin_mv_apply_common(size_t ni, size_t d, const double *G, size_t ldg, int g_where, const int *ind, const double *W,
                                    size_t c, const double *Y, const double *Vg, const double *Ve, const double *B, double *y_miss,
                                    void *stream) {
  size_t m = 0;
  int rc = prdt_kin_mv_check("prdt_kin_mv_apply", ni, d, G, ldg, ind, W, c, Y, 0, &m);
  if (rc) return rc;
  if (!Vg || !Ve || !B) return fail(GEMMA_HIP_EINVAL, "prdt_kin_mv_apply: Vg, Ve or B is NULL");
  if (m == 0) return GEMMA_HIP_OK;
  if (!y_miss) return fail(GEMMA_HIP_EINVAL, "prdt_kin_mv_apply: y_miss is NULL");
  std::string msg;
  long bad = -1;
  rc = prdt_mv_apply_x((long)ni, (long)d, G, (long)ldg, g_where, ind, W, (long)c, Y, Vg, Ve, B, y_miss, &bad, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_prdt_kin_mv_apply(size_t ni, size_t d, const double *G_full, const int *indicator_pheno, const double *W_full,
                                           size_t n_cvt, const double *Y_full, const double *Vg, const double *Ve, const double *B,
                                           double *y_miss) {
  NEED_INIT();
  return prdt_kin_mv_apply_common(ni, d, G_full, ni, 0, indicator_pheno, W_full, n_cvt, Y_full, Vg, Ve, B, y_miss, nullptr);
}

extern "C" int gemma_hip_prdt_kin_mv_apply_d(size_t ni, size_t d, const double *G_full_d, size_t ldg, const int *indicator_pheno,
                                             const double *W_full, size_t n_cvt, const double *Y_full, const double *Vg, const double *Ve,
                                             const double *B, double *y_miss, void *stream) {
  NEED_INIT();
  return prdt_kin_mv_apply_common(ni, d, G_full_d, ldg, 1, indicator_pheno, W_full, n_cvt, Y_full, Vg, Ve, B, y_miss, stream);
}

extern "C" int gemma_hip_prdt_kin_mv(size_t ni, size_t d, const double *G_full, const int *indicator_pheno, const double *W_full,
                                     size_t n_cvt, const double *Y_full, double l_min, double l_max, size_t n_region,
                                     const gemma_mvlmm_opt *opt, double *y_miss, gemma_mvlmm_null *fit) {
  NEED_INIT();
  if (d == 1) { // the reference takes the univariate branch (src/gemma.cpp:1790-1820)
    double fit3[3] = {0.0, 0.0, 0.0};
    const int rc1 = gemma_hip_prdt_kin(ni, G_full, indicator_pheno, W_full, n_cvt, Y_full, l_min, l_max, n_region, y_miss, fit3);
    if (rc1 == GEMMA_HIP_OK && fit) {
      memset(fit, 0, sizeof *fit);
      fit->Vg_remle[0] = fit3[0];
      fit->Ve_remle[0] = fit3[1];
    }
    return rc1;
  }
  size_t m = 0;
  int rc = prdt_kin_mv_check("prdt_kin_mv", ni, d, G_full, ni, indicator_pheno, W_full, n_cvt, Y_full, 1, &m);
  if (rc) return rc;
  const size_t c = n_cvt;
  std::vector<int> pos; // the individuals with every phenotype: the null fit's (cPar.indicator_idv)
  for (size_t i = 0; i < ni; ++i) {
    bool full = true;
    for (size_t a = 0; a < d; ++a) full = full && indicator_pheno[i * d + a] != 0;
    if (full) pos.push_back((int)i);
  }
  const size_t n = pos.size();
  if (n <= c + 1) return fail(GEMMA_HIP_EINVAL, "prdt_kin_mv: %zu individuals with every phenotype, %zu covariates", n, c);
  if (m > 0 && !y_miss) return fail(GEMMA_HIP_EINVAL, "prdt_kin_mv: y_miss is NULL");
  // G_full to the device once; G of the complete individuals taken from it and centred there (:1757-1773)
  std::string msg;
  double *Gd = nullptr;
  if ((rc = prdt_mv_stage_G_x(G_full, (long)ni, (long)ni, false, &Gd, nullptr, msg))) return ret(rc, msg);
  const size_t k = c + d;
  std::vector<double> WY(n * k), UtWY(n * k), ev(n), UtW(n * c), UtY(n * d);
  { // the device buffers of the decomposition go at the end of this block, before the null fit asks for its own
    ScopedBuf sub, U, small; // small: [eval n | WY n x (c + d) | UtWY n x (c + d)]
    if (sub.reserve(n * n * 8) || U.reserve(n * n * 8) || small.reserve((n + 2 * n * k) * 8))
      return fail(GEMMA_HIP_ENOMEM, "prdt_kin_mv: cannot allocate 2 x %zu bytes", n * n * 8);
    if ((rc = prdt_mv_sub_x(Gd, (long)ni, pos.data(), (long)n, sub.as<double>(), nullptr, msg))) return ret(rc, msg);
    double *ev_d = small.as<double>(), *WY_d = ev_d + n, *UtWY_d = WY_d + n * k;
    double trace_G = 0.0;
    if ((rc = gemma_hip_center_d(sub.as<double>(), n, nullptr)) ||
        (rc = gemma_hip_eigh_d(sub.as<double>(), n, U.as<double>(), ev_d, &trace_G, nullptr)))
      return rc;
    // U'W and U'Y in one product (:1785-1786)
    for (size_t a = 0; a < n; ++a) {
      for (size_t j = 0; j < c; ++j) WY[a * k + j] = W_full[(size_t)pos[a] * c + j];
      for (size_t j = 0; j < d; ++j) WY[a * k + c + j] = Y_full[(size_t)pos[a] * d + j];
    }
    HIPCHK(hipMemcpy(WY_d, WY.data(), n * k * 8, hipMemcpyHostToDevice));
    if ((rc = gemma_hip_dgemm_d('T', 'N', n, k, n, 1.0, U.as<double>(), n, WY_d, k, 0.0, UtWY_d, k, nullptr))) return rc;
    HIPCHK(hipMemcpy(UtWY.data(), UtWY_d, n * k * 8, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ev.data(), ev_d, n * 8, hipMemcpyDeviceToHost));
  }
  for (size_t a = 0; a < n; ++a) {
    for (size_t j = 0; j < c; ++j) UtW[a * c + j] = UtWY[a * k + j];
    for (size_t j = 0; j < d; ++j) UtY[a * d + j] = UtWY[a * k + c + j];
  }
  // CalcMvLmmVgVeBeta (:1828-1830): the REMLE half of the null block
  gemma_mvlmm_null local;
  gemma_mvlmm_null *f = fit ? fit : &local;
  if ((rc = gemma_hip_mvlmm_null(n, c, d, ev.data(), UtW.data(), UtY.data(), l_min, l_max, n_region, opt, f))) return rc;
  if (m == 0) return GEMMA_HIP_OK;
  long bad = -1;
  rc = prdt_mv_apply_x((long)ni, (long)d, nullptr, (long)ni, 2, indicator_pheno, W_full, (long)c, Y_full, f->Vg_remle, f->Ve_remle,
                       f->B_remle, y_miss, &bad, nullptr, msg);
  return ret(rc, msg);
}

// tests and scripts/prdt_mv_probe.py (not in the public header): H_oo's assembled upper triangle, and the factor + solve path on a
// host or a device matrix
extern "C" int gemma_hip_dbg_prdt_mv_assemble(size_t ni, size_t d, const double *Gc, const int *indicator_pheno, const double *Vg,
                                              const double *Ve, double *H, size_t lda) {
  NEED_INIT();
  if (ni == 0 || d == 0 || d > (size_t)MV_DMAX || !Gc || !indicator_pheno || !Vg || !Ve || !H)
    return fail(GEMMA_HIP_EINVAL, "dbg_prdt_mv_assemble: ni = %zu, d = %zu", ni, d);
  size_t N = 0;
  for (size_t k = 0; k < ni * d; ++k) N += indicator_pheno[k] != 0;
  if (lda < N) return fail(GEMMA_HIP_EINVAL, "dbg_prdt_mv_assemble: lda = %zu, %zu observed entries", lda, N);
  std::string msg;
  const int rc = prdt_mv_dbg_assemble_x((long)ni, (long)d, Gc, indicator_pheno, Vg, Ve, H, (long)lda, nullptr, msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_dbg_spd_solve(const double *A, size_t n, double *x, long *bad_pivot) {
  NEED_INIT();
  if (n == 0 || !A || !x) return fail(GEMMA_HIP_EINVAL, "dbg_spd_solve: n = %zu", n);
  std::string msg;
  const int rc = prdt_mv_dbg_solve_x(const_cast<double *>(A), (long)n, (long)n, x, false, bad_pivot, nullptr, msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_dbg_spd_solve_d(double *A_d, size_t n, size_t lda, double *x_d, long *bad_pivot, void *stream) {
  NEED_INIT();
  if (n == 0 || lda < n || !A_d || !x_d) return fail(GEMMA_HIP_EINVAL, "dbg_spd_solve: n = %zu, lda = %zu", n, lda);
  std::string msg;
  const int rc = prdt_mv_dbg_solve_x(A_d, (long)n, (long)lda, x_d, true, bad_pivot, S(stream), msg);
  return ret(rc, msg);
}

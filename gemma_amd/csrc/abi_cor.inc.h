// ------------------------------------------------------------------------------ windowed SNP correlation (-calccor)
// Textual part of gemma_hip.hip: argument checks and error text around the correlation unit (cor_tu.hip).

extern "C" int gemma_hip_cor_begin(size_t ni_total, const int *indicator_idv) {
  NEED_INIT();
  if (ni_total == 0 || ni_total > (size_t)1 << 30) return fail(GEMMA_HIP_EINVAL, "cor_begin: ni_total = %zu", ni_total);
  std::string msg;
  const int rc = cor_begin_x((long)ni_total, indicator_idv, msg);
  return ret(rc, msg);
}

static int cor_block_common(int geno_kind, const void *geno, size_t l_in, size_t ld, size_t l_out, const int *n_nb, double *var,
                            double *cor, bool device, void *stream) {
  if (!cor_active_x()) return fail(GEMMA_HIP_EINVAL, "cor_block before cor_begin");
  if (l_out == 0) return GEMMA_HIP_OK;
  if (l_in < l_out) return fail(GEMMA_HIP_EINVAL, "cor_block: l_in = %zu < l_out = %zu", l_in, l_out);
  if (!n_nb || !var) return fail(GEMMA_HIP_EINVAL, "cor_block: n_nb or var is NULL");
  int rc = mv_check_block("cor_block", geno_kind, geno, l_in, ld, (size_t)cor_ni_total_x());
  if (rc) return rc;
  std::string msg;
  rc = cor_block_x(geno_kind, geno, (long)l_in, (long)ld, (long)l_out, n_nb, var, cor, device, S(stream), msg);
  return ret(rc, msg);
}

extern "C" int gemma_hip_cor_block(int geno_kind, const void *geno, size_t l_in, size_t ld, size_t l_out, const int *n_nb, double *var,
                                   double *cor) {
  NEED_INIT();
  return cor_block_common(geno_kind, geno, l_in, ld, l_out, n_nb, var, cor, false, nullptr);
}

extern "C" int gemma_hip_cor_block_d(int geno_kind, const void *geno_d, size_t l_in, size_t ld, size_t l_out, const int *n_nb_d,
                                     double *var_d, double *cor_d, void *stream) {
  NEED_INIT();
  return cor_block_common(geno_kind, geno_d, l_in, ld, l_out, n_nb_d, var_d, cor_d, true, stream);
}

extern "C" int gemma_hip_cor_release(void) {
  NEED_INIT();
  cor_release_x();
  return GEMMA_HIP_OK;
}

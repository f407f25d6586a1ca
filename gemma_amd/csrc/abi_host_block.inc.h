// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace).
// This part: a genotype block as the caller holds it -- its geometry and the argument check every block entry point makes
// (block_geom), the staging copy of a host block (stage_block) and the shape of a host-pointer entry point around its _d form
// (host_batch).  Included first: the kinship takes the geometry as well.

static size_t min_ld_for(int kind, size_t n_items_per_row, size_t l) {
  switch (kind) {
  case GEMMA_GENO_F64_SNP_MAJOR: return n_items_per_row;
  case GEMMA_GENO_PLINK_2BIT: return (n_items_per_row + 3) / 4;
  case GEMMA_GENO_F64_IDV_MAJOR: return l;
  default: return (size_t)-1;
  }
}

struct BlockGeom {
  size_t need; // items read of every row (the smallest ld)
  size_t rows; // rows in memory: SNPs, or individuals for individual-major input
  size_t esz;  // bytes per item
};

// The check of a block of l SNPs over n analysed individuals, and its geometry.  mapped: PLINK rows cover the ni_total individuals
// of lmm_set_indicator when a map is in place (the kinship has none).  out: the caller's output pointer -- geno again where the
// call has none.  g may be nullptr (the _d forms only validate).
static int block_geom(const char *who, int kind, size_t n, bool mapped, const void *geno, size_t l, size_t ld, const void *out,
                      BlockGeom *g = nullptr) {
  const size_t per_row = (mapped && kind == GEMMA_GENO_PLINK_2BIT && g_ctx.have_map) ? g_ctx.ni_total : n;
  const size_t need = min_ld_for(kind, per_row, l);
  if (need == (size_t)-1) return fail(GEMMA_HIP_EINVAL, "%s: unknown geno_kind %d", who, kind);
  if (!geno || !out || ld < need) return fail(GEMMA_HIP_EINVAL, "%s: ld=%zu < %zu", who, ld, need);
  if (g) *g = BlockGeom{need, kind == GEMMA_GENO_F64_IDV_MAJOR ? n : l, kind == GEMMA_GENO_PLINK_2BIT ? (size_t)1 : (size_t)8};
  return GEMMA_HIP_OK;
}

// A host block into g_ctx.stage_in, at the caller's ld: exactly `need` items of every row are read (the caller's last row may end
// there; what lies behind them in a wider row is not the block's) -- the same rows hipMemcpy2D of gemma_hip_dgemm copies.
static int stage_block(const char *who, const BlockGeom &g, const void *geno, size_t ld) {
  if (g_ctx.stage_in.reserve(g.rows * ld * g.esz)) return fail(GEMMA_HIP_ENOMEM, "%s: staging %zu bytes", who, g.rows * ld * g.esz);
  HIPCHK(hipMemcpy2D(g_ctx.stage_in.p, ld * g.esz, geno, ld * g.esz, g.need * g.esz, g.rows, hipMemcpyHostToDevice));
  return GEMMA_HIP_OK;
}

// A host-pointer block entry point after its state check: stage the block, run(block on the device, out_buf.p) -- the _d form on
// the null stream --, copy out_bytes back from out_buf.
template <class Run>
static int host_block(const char *who, const BlockGeom &g, const void *geno, size_t ld, DevBuf &out_buf, void *out, size_t out_bytes,
                      Run run) {
  if (out_buf.reserve(out_bytes)) return fail(GEMMA_HIP_ENOMEM, "%s: staging %zu bytes", who, out_bytes);
  int rc = stage_block(who, g, geno, ld);
  if (!rc) rc = run(g_ctx.stage_in.p, out_buf.p);
  if (rc) return rc;
  HIPCHK(hipMemcpy(out, out_buf.p, out_bytes, hipMemcpyDeviceToHost));
  return GEMMA_HIP_OK;
}
// ... of a block of `kind` over the setup's n individuals
template <class Run>
static int host_batch(const char *who, int kind, const void *geno, size_t l, size_t ld, DevBuf &out_buf, void *out, size_t out_bytes,
                      Run run) {
  BlockGeom g;
  const int rc = block_geom(who, kind, g_ctx.cfg.n, true, geno, l, ld, out, &g);
  return rc ? rc : host_block(who, g, geno, ld, out_buf, out, out_bytes, run);
}

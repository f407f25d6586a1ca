// Part of gemma_hip.hip (ONE translation unit: the parts share the context g_ctx and the helpers of its anonymous namespace, and are
// included there in this order).
// This part: U^T x launch sites: the int8-digit products (records kernel, dosage planes), digit combine, compute_utx.  Which form
// the hard-call product takes and which kernels it launches is decided in i8_plan.h; this file reserves and launches from that.

// ---- exact int8-digit U^T x (i8gemm.hip.h): buffers, the product on an already packed left factor, ingest variants
static_assert(I8_PLAN_BM_RECORDS == (size_t)S2_BM && I8_PLAN_BM_BYTES == (size_t)I8P_BM,
              "i8_plan.h pads a block to the kernels' tile heights");
// The form of a block's product with what is known at run time only: the padding of U's digit planes (i8_prepare_u), and -- form
// with `direct`, set by i8_plink_left -- the 2-bit PLINK rows the records came from (plink_records_kernel): g_ctx.i8_A holds
// nothing of the block then and the surplus kernels read the missing pattern of their rows there.  nullptr: the byte matrix
struct I8Dims : I8Form {
  size_t ldk, npad;
  const unsigned char *bed = nullptr;
  long bed_ld = 0;
};
static const int *i8_anymiss(const I8Dims &d) { return d.complete ? g_ctx.i8_rowsur.as<int>() + d.lpad : nullptr; }
// allow_epi = false: the caller needs the planes and a separate combine (the two-block pipe: its product must not write the ONE
// g_ctx.UtX while the block before it is still read from there)
// allow_direct: the caller is i8_plink_left's and can leave the block's 2-bit rows in place until its i8_post_rows has run; a form
// with `direct` does not touch g_ctx.i8_A
static int i8_begin(size_t l, I8Dims *d, hipStream_t s, bool allow_epi = true, bool allow_direct = false) {
  int rc = i8_prepare_u(s);
  if (rc) return rc;
  static_cast<I8Form &>(*d) = i8_form(g_ctx.knobs.i8, g_ctx.cfg.n, l, g_ctx.i8_digits, g_ctx.have_map, allow_epi, allow_direct);
  d->ldk = g_ctx.i8_ldk; d->npad = g_ctx.i8_npad;
  const bool with_bytes = !d->direct;
  const size_t c_elems = (size_t)d->c_planes * d->mrows * d->npad;
  const size_t a_bytes = with_bytes ? d->lpad * d->ldk : 0;
  if ((with_bytes && g_ctx.i8_A.reserve(a_bytes)) || g_ctx.i8_C.reserve(c_elems * 4) || g_ctx.i8_mean.reserve(l * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_batch: int8 product buffers (%zu bytes)", a_bytes + c_elems * 4);
  // the padding rows [l, lpad) only: every packing kernel writes every byte of the rows below l, K padding included (the whole
  // matrix was zeroed here until round 8: 406 MB per 20 000 x 20 000 block for 224 rows)
  if (with_bytes && d->lpad != l) HIPCHK(hipMemsetAsync(g_ctx.i8_A.as<int8_t>() + l * d->ldk, 0, (d->lpad - l) * d->ldk, s));
  return GEMMA_HIP_OK;
}

// The records / mask words of a block (`words` of 16 bytes) and, per padded row, the calls the mask operand dropped, with the
// block's any-missing flag behind them; what each builder zeroes of the counters is its own affair
static int i8_meta_reserve(const I8Dims &d, size_t words) {
  if (g_ctx.i8_meta.reserve(words * sizeof(uint4)) || g_ctx.i8_rowsur.reserve((d.lpad + 1) * sizeof(int)))
    return fail(GEMMA_HIP_ENOMEM, "lmm_batch: records / mask words of the sparse product");
  g_ctx.i8_flag_at = d.complete ? (long)d.lpad : -1;
  g_ctx.i8_rowsur_n = (long)d.lpad;
  return GEMMA_HIP_OK;
}

// The int8 product in three pieces, each over the SNP rows [row0, row0 + rows) of the packed block (rows, row0 multiples of the
// kernel's tile height except for the last piece of a block): mask words / records, the matrix product, the digit combine.
static int i8_meta_build(const I8Dims &d, hipStream_t s) {
  if (!d.sparse()) return GEMMA_HIP_OK;
  ProfScope ps(GEMMA_STAGE_INGEST, s);
  const size_t nk = d.ldk / I8_BK, total = d.lpad * nk * (d.records() ? 4 : 2);
  if (int rc = i8_meta_reserve(d, total)) return rc;
  HIPCHK(hipMemsetAsync(g_ctx.i8_rowsur.p, 0, (d.lpad + 1) * sizeof(int), s)); // dropped calls per row, then the block's any-missing flag
  if (d.records())
    hipLaunchKernelGGL(sparse2_meta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g_ctx.i8_A.as<int8_t>(),
                       (long)d.lpad, (long)d.ldk, g_ctx.i8_meta.as<uint4>(), g_ctx.i8_rowsur.as<int>(),
                       const_cast<int *>(i8_anymiss(d)));
  else
    hipLaunchKernelGGL(sparse_meta_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, g_ctx.i8_A.as<int8_t>(),
                       (long)d.lpad, (long)d.ldk, g_ctx.i8_meta.as<uint4>(), g_ctx.i8_rowsur.as<int>());
  HIPCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

// The raster of a launch shape: found in the cache or built into the least recently used slot.  A slot is only recycled when more
// than six shapes are alive (a block in row chunks has two); then the device is synchronised first, since a kernel on ANY stream may
// still read the map that goes.
static int raster_for(int tiles_m, int tiles_n, int rb, hipStream_t s, const int2 **map_d) {
  Ctx::RasterSlot *lru = &g_ctx.i8_raster[0];
  for (auto &r : g_ctx.i8_raster) {
    if (r.tm == tiles_m && r.tn == tiles_n && r.rb == rb && r.dev.p) {
      r.used = ++g_ctx.i8_raster_clock;
      *map_d = r.dev.as<int2>();
      return GEMMA_HIP_OK;
    }
    if (r.used < lru->used) lru = &r;
  }
  if (lru->dev.p) HIPCHK(hipDeviceSynchronize()); // recycling a map some launch may still read
  s2_build_raster(tiles_m, tiles_n, rb, lru->host);
  lru->tm = lru->tn = lru->rb = 0;
  if (lru->dev.reserve(lru->host.size() * sizeof(int2)))
    return fail(GEMMA_HIP_ENOMEM, "lmm_batch: tile raster (%zu bytes)", lru->host.size() * sizeof(int2));
  // once per launch shape, and synchronous: a later cache hit hands the same map to a launch on ANY stream, and nothing
  // would order that launch behind an upload still queued on this one
  HIPCHK(hipMemcpyAsync(lru->dev.p, lru->host.data(), lru->host.size() * sizeof(int2), hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  lru->tm = tiles_m; lru->tn = tiles_n; lru->rb = rb;
  lru->used = ++g_ctx.i8_raster_clock;
  *map_d = lru->dev.as<int2>();
  return GEMMA_HIP_OK;
}

// Dynamic LDS of the int8 product kernels, hard calls and dosages: once, at the first int8 product
static int i8_kernel_attrs() {
  static bool done = false;
  if (done) return GEMMA_HIP_OK;
  const struct { const void *f; int lds; } attrs[] = {
      {reinterpret_cast<const void *>(i8gemm_packed_kernel_t<true>), 3 * I8P_STAGE},
      {reinterpret_cast<const void *>(i8gemm_sparse_kernel), 3 * SP_STAGE},
      {reinterpret_cast<const void *>(i8gemm_sparse2_kernel), S2_NST * S2_STAGE},
      {reinterpret_cast<const void *>(i8gemm_sparse2_r16_kernel), S2_R16_LDS},
      {reinterpret_cast<const void *>(i8gemm_sparse2_r16_g_kernel), S2_R16_LDS},
      {reinterpret_cast<const void *>(i8gemm_sparse2_r16_ep_kernel), S2_R16_LDS},
      {reinterpret_cast<const void *>(i8gemm_sparse2_r16_ep_g_kernel), S2_R16_LDS},
      {reinterpret_cast<const void *>(i8gemm_packed_kernel_t<false, true>), 3 * I8P_STAGE},
      {reinterpret_cast<const void *>(i8gemm_dense16_kernel_t<true>), 3 * I8P_STAGE}};
  for (const auto &a : attrs) HIPCHK(hipFuncSetAttribute(a.f, hipFuncAttributeMaxDynamicSharedMemorySize, a.lds));
  done = true;
  return GEMMA_HIP_OK;
}

// rows_pad: padded rows of this piece (a multiple of the tile height; row0 too).  Pieces other than the whole block are taken
// by the records kernels only.
// UtX, ldx, rows (d.epi only): where the rows [row0, row0 + rows) of U^T x go -- the whole destination, as i8_post_rows takes it.
static int i8_gemm_rows(const I8Dims &d, size_t row0, size_t rows_pad, hipStream_t s, double *UtX = nullptr, size_t ldx = 0,
                        size_t rows = 0) {
  static_assert(GEMMA_UTX_KERNEL_DENSE_I8 == I8_DENSE + 1 && GEMMA_UTX_KERNEL_SPARSE_BYTES == I8_SPARSE_BYTES + 1 &&
                    GEMMA_UTX_KERNEL_RECORDS_R32 == I8_RECORDS_R32 + 1 && GEMMA_UTX_KERNEL_RECORDS_R16 == I8_RECORDS_R16 + 1,
                "the matrix kernel reported for a mode");
  if (d.epi && (!UtX || rows == 0))
    return fail(GEMMA_HIP_ESTATE, "lmm_batch: the epilogue form of the int8 product without its destination");
  g_ctx.i8_last_epi = d.epi;
  ProfScope ps(GEMMA_STAGE_UTX_GEMM, s);
  if (int rc = i8_kernel_attrs()) return rc;
  const I8Switches &k = g_ctx.knobs.i8;
  I8Launch plan[4];
  const int launches = i8_launches(d, plan);
  const int nk = (int)(d.ldk / I8_BK);
  const long strideB = (long)(d.npad * d.ldk), strideC = (long)(d.mrows * d.npad);
  if (!d.records()) {
    // the mask product on dense MFMAs (i8gemm_packed_kernel_t) or on the 2:4 sparse MFMA with byte genotypes and separate mask
    // words (i8gemm_sparse.hip.h): the whole block, every plane, one launch
    I8PackArgs g;
    g.A = g_ctx.i8_A.as<int8_t>(); g.Bt = g_ctx.i8_Bt.as<int8_t>(); g.C = g_ctx.i8_C.as<int>();
    g.ldk = (long)d.ldk; g.ldc = (long)d.npad; g.strideB = strideB; g.strideC = strideC;
    g.m_row0 = (long)d.lpad;
    g.tiles_m = (int)(d.lpad / I8P_BM); g.tiles_n = (int)(d.npad / I8_BN);
    g.nk = nk; g.gm = k.gm; g.fuse = d.fuse; g.digits = d.digits;
    const dim3 grid((unsigned)(g.tiles_m * g.tiles_n), (unsigned)plan[0].planes);
    note_utx_kernel(d.mode + 1, d.digits, d.fuse, 0);
    if (plan[0].kernel == I8K_SPARSE) {
      SparseMeta sm;
      sm.m4 = g_ctx.i8_meta.as<uint4>();
      sm.row_surplus = g_ctx.i8_rowsur.as<int>();
      sm.ntiles = (long)nk;
      hipLaunchKernelGGL(i8gemm_sparse_kernel, grid, dim3(512), 3 * SP_STAGE, s, g, sm);
    } else {
      hipLaunchKernelGGL(i8gemm_packed_kernel_t<true>, grid, dim3(512), 3 * I8P_STAGE, s, g);
    }
  } else {
    // the 2:4 sparse MFMA on records (i8gemm_sparse2*.hip.h) -- rows that lose calls to the 2-of-4 limit are completed in fp64
    // after the digits are combined
    Sparse2Args g2;
    // records: [tile_m][ktile][row % 256][chunk]; planes: G rows at row, M rows at lpad + row
    g2.AM = g_ctx.i8_meta.as<uint4>() + (row0 / S2_BM) * (size_t)nk * S2_BM * 4;
    g2.Bt = g_ctx.i8_Bt.as<int8_t>();
    // d.epi: plane 0 is never stored, plane q >= 1 lives at slot q - 1 of i8_C (the kernels address plane q at C + q * strideC)
    g2.C = g_ctx.i8_C.as<int>() + row0 * d.npad - (d.epi ? strideC : 0);
    g2.ldk = (long)d.ldk; g2.ldc = (long)d.npad; g2.strideB = strideB; g2.strideC = strideC;
    g2.m_row0 = (long)d.lpad;
    g2.tiles_m = (int)(rows_pad / S2_BM); g2.tiles_n = (int)(d.npad / S2_BN);
    g2.nk = nk; g2.gm = k.gm; g2.fuse = d.fuse; g2.digits = d.digits;
    // GEMMA_HIP_I8_RASTER: 0 = every XCD sweeps its own tile rows (round 3); 1 / 2 / 4 / 8 = row blocks of the super-patch the
    // eight XCDs share (s2_build_raster)
    if (k.raster > 0)
      if (int rc = raster_for(g2.tiles_m, g2.tiles_n, k.raster, s, &g2.tile_map)) return rc;
    g2.anymiss = i8_anymiss(d);
    if (d.epi) { // the epilogue instances read these; every other kernel ignores them (i8gemm_sparse2.h)
      g2.UtX = UtX + row0 * ldx; g2.ldx = (long)ldx; g2.l = (long)rows; g2.n = (long)d.n;
      g2.mean = g_ctx.i8_mean.as<double>() + row0; g2.qinv = g_ctx.i8_qinv.as<double>();
      g2.m_scale = 1.0; g2.nplanes = d.nplanes; g2.epi_depth = k.epi_depth;
    }
    // the 32-row kernel of rounds 3-4, or the same product on the 16-row forms (i8gemm_sparse2_r16.hip.h: same records, same
    // planes, every entry equal; 9 % faster under the power limit)
    note_utx_kernel(d.mode + 1, d.digits, d.fuse, k.raster > 0 ? k.raster : 0);
    static void (*const kernels[I8K_COUNT])(Sparse2Args) = {nullptr, nullptr, i8gemm_sparse2_kernel, i8gemm_sparse2_r16_kernel,
        i8gemm_sparse2_r16_g_kernel, i8gemm_sparse2_r16_ep_kernel, i8gemm_sparse2_r16_ep_g_kernel};
    // stream order is the dependency of the epilogue launch on the planes before it
    for (int i = 0; i < launches; ++i) {
      g2.plane0 = plan[i].plane0; g2.run_if = plan[i].run_if;
      hipLaunchKernelGGL(kernels[plan[i].kernel], dim3((unsigned)(g2.tiles_m * g2.tiles_n), (unsigned)plan[i].planes), dim3(512),
                         plan[i].kernel == I8K_SPARSE2 ? S2_NST * S2_STAGE : S2_R16_LDS, s, g2);
    }
  }
  HIPCHK(hipGetLastError());
  return GEMMA_HIP_OK;
}

// digits -> fp64 for the rows [row0, row0 + rows) of a block of l SNPs
static int i8_post_rows(size_t l, const I8Dims &d, size_t row0, size_t rows, double *UtX, size_t ldx, hipStream_t s) {
  ProfScope ps(GEMMA_STAGE_UTX_POST, s);
  // the calls the sparse mask operand dropped (groups of four with 3-4 missing calls): rows with up to SUR_MAX of them are
  // completed inside the digit combine from a short per-row list, the rare rows with more by the fp64 fix-up pass
  int *sur_cnt = nullptr, *sur_list = nullptr;
  // the missing pattern of the rows, as the surplus kernels read it: the block's 2-bit rows (direct form) or the byte matrix
  auto with_pattern = [&](auto &&launch) {
    if (d.bed) launch(SurplusPlink{d.bed + row0 * d.bed_ld, d.bed_ld, (long)d.n});
    else launch(SurplusBytes{g_ctx.i8_A.as<int8_t>() + row0 * d.ldk, (long)d.ldk});
  };
  if (d.sparse()) {
    if (g_ctx.i8_surlist.reserve(l * (SUR_MAX + 1) * sizeof(int)))
      return fail(GEMMA_HIP_ENOMEM, "lmm_batch: dropped-call lists");
    sur_cnt = g_ctx.i8_surlist.as<int>() + row0;
    sur_list = g_ctx.i8_surlist.as<int>() + l + row0 * SUR_MAX;
    with_pattern([&](auto from) {
      hipLaunchKernelGGL(i8_surplus_list_kernel<decltype(from)>, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, from,
                         (long)d.ldk, g_ctx.i8_rowsur.as<int>() + row0, (long)rows, sur_cnt, sur_list);
    });
    HIPCHK(hipGetLastError());
  }
  if (!d.epi) {
    hipLaunchKernelGGL(i8_combine_kernel, dim3((unsigned)((d.n + 1023) / 1024), (unsigned)std::min<size_t>(rows, 65535)),
                       dim3(256), 0, s,
                       g_ctx.i8_C.as<int>() + row0 * d.npad, (long)d.npad, (long)(d.mrows * d.npad), (long)d.lpad,
                       g_ctx.i8_mean.as<double>() + row0, g_ctx.i8_qinv.as<double>(), (long)rows, (long)d.n, UtX + row0 * ldx, (long)ldx,
                       1.0, d.fuse, d.digits, sur_cnt, sur_list, g_ctx.U, (long)d.n, d.mdrop, i8_anymiss(d));
    HIPCHK(hipGetLastError());
  } else {
    // the product's epilogue wrote U^T x (16-row records): only the short lists are left of the combine
    hipLaunchKernelGGL(i8_surplus_short_kernel, dim3((unsigned)rows), dim3(256), 0, s, sur_cnt, sur_list,
                       g_ctx.i8_mean.as<double>() + row0, g_ctx.U, (long)d.n, (long)d.n, (long)rows, UtX + row0 * ldx, (long)ldx);
    HIPCHK(hipGetLastError());
  }
  if (d.sparse()) {
    with_pattern([&](auto from) {
      hipLaunchKernelGGL(i8_surplus_fix_kernel<decltype(from)>, dim3((unsigned)rows), dim3(256), 0, s, from, (long)d.ldk,
                         g_ctx.i8_rowsur.as<int>() + row0, g_ctx.i8_mean.as<double>() + row0, g_ctx.U, (long)d.n, (long)d.n,
                         (long)rows, UtX + row0 * ldx, (long)ldx, SUR_MAX);
    });
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

// UtX (l x ldx) from the packed left factor in g_ctx.i8_A and the per-SNP means in g_ctx.i8_mean
static int i8_product(size_t l, const I8Dims &d, double *UtX, size_t ldx, hipStream_t s) {
  int rc = i8_meta_build(d, s);
  if (!rc) rc = i8_gemm_rows(d, 0, d.lpad, s, UtX, ldx, l);
  if (!rc) rc = i8_post_rows(l, d, 0, l, UtX, ldx, s);
  return rc;
}

// The left factor of a PLINK block, ready for i8_gemm_rows, and mean_s.  d comes from i8_begin(.., allow_direct = true) where the
// caller can leave geno as it is until the block's i8_post_rows has run: GEMMA_HIP_I8_DIRECT (default 1) then takes a block on the
// records kernels with every individual analysed from its 2-bit rows straight to the records (plink_records.hip.h) and sets d.bed.
// Every other form: the byte matrix (ingest_i8_kernel) and, for the sparse modes, the words built from it (i8_meta_build).
// after_ingest: recorded on s behind the last kernel that reads geno on the byte-matrix form.
static int i8_plink_left(const void *geno, size_t l, size_t ld, I8Dims &d, hipStream_t s, hipEvent_t after_ingest = nullptr) {
  if (!d.direct) {
    {
      ProfScope ps(GEMMA_STAGE_INGEST, s);
      IngestI8Args a;
      a.src = reinterpret_cast<const unsigned char *>(geno); a.ld = (long)ld; a.l = (long)l;
      a.idx_map = g_ctx.have_map ? g_ctx.idx_map.as<int>() : nullptr;
      a.n = (int)d.n; a.A = g_ctx.i8_A.as<int8_t>(); a.ldk = (long)d.ldk;
      a.mean = g_ctx.i8_mean.as<double>();
      hipLaunchKernelGGL(ingest_i8_kernel, dim3((unsigned)((l + 3) / 4)), dim3(256), 0, s, a);
      HIPCHK(hipGetLastError());
    }
    if (after_ingest) HIPCHK(hipEventRecord(after_ingest, s));
    return i8_meta_build(d, s);
  }
  if (after_ingest)
    return fail(GEMMA_HIP_ESTATE, "lmm_batch: records straight from the 2-bit rows on a path that needs the byte matrix");
  ProfScope ps(GEMMA_STAGE_INGEST, s);
  if (int rc = i8_meta_reserve(d, d.lpad * (d.ldk / I8_BK) * 4)) return rc;
  // the block's any-missing flag; the kernel writes every row counter itself
  HIPCHK(hipMemsetAsync(g_ctx.i8_rowsur.as<int>() + d.lpad, 0, sizeof(int), s));
  PlinkRecordsArgs a;
  a.src = reinterpret_cast<const unsigned char *>(geno); a.ld = (long)ld; a.l = (long)l; a.lpad = (long)d.lpad;
  a.n = (int)d.n; a.ldk = (long)d.ldk;
  a.AM = g_ctx.i8_meta.as<uint4>(); a.row_surplus = g_ctx.i8_rowsur.as<int>();
  a.anymiss = const_cast<int *>(i8_anymiss(d)); a.mean = g_ctx.i8_mean.as<double>();
  hipLaunchKernelGGL(plink_records_kernel, dim3((unsigned)(d.lpad / 4)), dim3(256), 0, s, a);
  HIPCHK(hipGetLastError());
  d.bed = a.src; d.bed_ld = (long)ld;
  return GEMMA_HIP_OK;
}

// PLINK 2-bit batch
static int utx_plink_i8(const void *geno, size_t l, size_t ld, double *UtX, size_t ldx, hipStream_t s) {
  I8Dims d;
  int rc = i8_begin(l, &d, s, true, true);
  if (!rc) rc = i8_plink_left(geno, l, ld, d, s);
  if (!rc) rc = i8_gemm_rows(d, 0, d.lpad, s, UtX, ldx, l);
  if (!rc) rc = i8_post_rows(l, d, 0, l, UtX, ldx, s);
  return rc;
}

// Fixed-point dosage rows (i8gemm.hip.h: pack_dosage_kernel): byte planes a0 [, a1] [, mask] x the digits of U on the dense int8
// kernel, one int32 plane per (byte plane, digit); GEMMA_HIP_UTX_DOSAGE_I8=0 keeps such batches on the fp64 GEMM.
static bool dosage_i8_enabled() { return g_ctx.knobs.dosage_i8 != 0; }
static int utx_dosage_i8(const double *src, size_t l, size_t ld, bool nan_missing, bool two, bool have_m, const I8Dims &d,
                         double *UtX, size_t ldx, hipStream_t s) {
  const int np = (two ? 2 : 1) + (have_m ? 1 : 0);
  const size_t plane_a = d.lpad * d.ldk, plane_c = d.lpad * d.npad;
  if (g_ctx.i8_A.reserve((size_t)np * plane_a) || g_ctx.i8_C.reserve((size_t)np * d.digits * plane_c * 4) ||
      g_ctx.i8_colsum.reserve(d.n * 8))
    return fail(GEMMA_HIP_ENOMEM, "lmm_batch: dosage planes (%zu bytes)", (size_t)np * (plane_a + d.digits * plane_c * 4));
  int8_t *A0 = g_ctx.i8_A.as<int8_t>();
  {
    ProfScope ps(GEMMA_STAGE_INGEST, s);
    if (d.lpad != l) HIPCHK(hipMemsetAsync(A0, 0, (size_t)np * plane_a, s)); // padding rows of every plane
    PackDosageArgs a;
    a.src = src; a.ld = (long)ld; a.l = (long)l; a.n = (int)d.n; a.nan_missing = nan_missing ? 1 : 0; a.two = two ? 1 : 0;
    a.A0 = A0; a.A1 = two ? A0 + plane_a : nullptr; a.Am = have_m ? A0 + (size_t)(np - 1) * plane_a : nullptr;
    a.ldk = (long)d.ldk; a.mean = g_ctx.i8_mean.as<double>();
    hipLaunchKernelGGL(pack_dosage_kernel, dim3((unsigned)((l + 3) / 4)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
    if (!g_ctx.i8_colsum_ready) {
      hipLaunchKernelGGL(u_digit_colsum_kernel, dim3((unsigned)((d.n + 3) / 4)), dim3(256), 0, s, g_ctx.i8_Bt.as<int8_t>(),
                         (long)d.ldk, (long)(d.npad * d.ldk), g_ctx.i8_qinv.as<double>(), (long)d.n, d.digits,
                         g_ctx.i8_colsum.as<double>());
      HIPCHK(hipGetLastError());
      g_ctx.i8_colsum_ready = true;
    }
  }
  {
    ProfScope ps(GEMMA_STAGE_UTX_GEMM, s);
    if (int rc = i8_kernel_attrs()) return rc;
    for (int a = 0; a < np; ++a) {
      I8PackArgs g;
      g.A = A0 + (size_t)a * plane_a;
      g.Bt = g_ctx.i8_Bt.as<int8_t>();
      g.C = g_ctx.i8_C.as<int>() + (size_t)a * d.digits * plane_c;
      g.ldk = (long)d.ldk; g.ldc = (long)d.npad;
      g.strideB = (long)(d.npad * d.ldk); g.strideC = (long)plane_c;
      g.m_row0 = 0;
      g.tiles_m = (int)(d.lpad / I8P_BM); g.tiles_n = (int)(d.npad / I8_BN);
      g.nk = (int)(d.ldk / I8_BK);
      g.gm = g_ctx.knobs.i8.gm;
      g.fuse = 0;
      g.digits = d.digits;
      // round 5: the byte planes on v_mfma_i32_16x16x64_i8 (i8gemm_dense16.hip.h: same tiles, same LDS images, every plane entry equal;
      // 44.5 against 46.8 ms for six planes at n = B = 20 000 under the power limit); GEMMA_HIP_DOSAGE_ROWS=32: the 32-row kernel
      if (g_ctx.knobs.dosage_rows == 32) {
        note_utx_kernel(GEMMA_UTX_KERNEL_DOSAGE_I8, d.digits, 0, 0);
        hipLaunchKernelGGL((i8gemm_packed_kernel_t<false, true>), dim3((unsigned)(g.tiles_m * g.tiles_n), (unsigned)d.digits),
                           dim3(512), 3 * I8P_STAGE, s, g);
      } else {
        note_utx_kernel(GEMMA_UTX_KERNEL_DOSAGE_I8_R16, d.digits, 0, 0);
        hipLaunchKernelGGL((i8gemm_dense16_kernel_t<true>), dim3((unsigned)(g.tiles_m * g.tiles_n), (unsigned)d.digits),
                           dim3(512), 3 * I8P_STAGE, s, g);
      }
      HIPCHK(hipGetLastError());
    }
  }
  {
    ProfScope ps(GEMMA_STAGE_UTX_POST, s);
    hipLaunchKernelGGL(i8_combine_dosage_kernel, dim3((unsigned)((d.n + 255) / 256), (unsigned)std::min<size_t>(l, 65535)),
                       dim3(256), 0, s, g_ctx.i8_C.as<int>(), (long)d.npad, (long)plane_c, g_ctx.i8_mean.as<double>(),
                       g_ctx.i8_qinv.as<double>(), g_ctx.i8_colsum.as<double>(), (long)l, (long)d.n, UtX, (long)ldx, d.digits,
                       two ? 1 : 0, have_m ? 1 : 0, two ? 1000.0 : 100.0);
    HIPCHK(hipGetLastError());
  }
  return GEMMA_HIP_OK;
}

// fp64 SNP-major rows (src: l x ld): if every row is a hard-call row (i8gemm.hip.h, pack_f64_kernel) the batch goes
// through the int8-digit product and *done = true; otherwise nothing is computed and the caller takes the fp64 GEMM.
// One stream synchronisation per batch (the verdict is read back).
static int utx_f64_try_i8(const double *src, size_t l, size_t ld, bool nan_missing, double *UtX, size_t ldx,
                          hipStream_t s, bool *done) {
  *done = false;
  I8Dims d;
  int rc = i8_begin(l, &d, s);
  if (rc) return rc;
  if (g_ctx.scratch.reserve(16)) return fail(GEMMA_HIP_ENOMEM, "lmm_batch: scratch");
  const int init[4] = {1, 1, 1, 0}; // hard calls, dosages k/1000, dosages k/100, any missing entry
  HIPCHK(hipMemcpyAsync(g_ctx.scratch.p, init, sizeof init, hipMemcpyHostToDevice, s));
  {
    ProfScope ps(GEMMA_STAGE_INGEST, s);
    PackF64Args a;
    a.src = src; a.ld = (long)ld; a.l = (long)l; a.n = (int)d.n; a.nan_missing = nan_missing ? 1 : 0;
    a.A = g_ctx.i8_A.as<int8_t>(); a.ldk = (long)d.ldk; a.mean = g_ctx.i8_mean.as<double>();
    a.all_hard = g_ctx.scratch.as<int>();
    hipLaunchKernelGGL(pack_f64_kernel, dim3((unsigned)((l + 3) / 4)), dim3(256), 0, s, a);
    HIPCHK(hipGetLastError());
  }
  int verdict[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(verdict, g_ctx.scratch.p, sizeof verdict, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (verdict[0]) {
    *done = true;
    g_ctx.last_utx_path = 1;
    return i8_product(l, d, UtX, ldx, s);
  }
  if (verdict[1] && dosage_i8_enabled()) { // fixed-point dosages: k/100 on one byte plane, k/1000 on two
    *done = true;
    g_ctx.last_utx_path = verdict[2] ? 2 : 3;
    return utx_dosage_i8(src, l, ld, nan_missing, !verdict[2], verdict[3] != 0, d, UtX, ldx, s);
  }
  return GEMMA_HIP_OK;
}

// U as the right-hand operand of the fp64 GEMM.  With an odd n the caller's U (leading dimension n) would send every tile down
// the bounds-checked kernel (the LDS-DMA path wants even leading dimensions): a copy with leading dimension n + 1 is made
// once per lmm_setup and used instead.
static int gemm_U(const double **U, long *ld, hipStream_t s) {
  const size_t n = g_ctx.cfg.n;
  *U = g_ctx.U;
  *ld = (long)n;
  if ((n & 1) == 0) return GEMMA_HIP_OK;
  if (g_ctx.U_even_of != g_ctx.U) {
    if (g_ctx.U_even.reserve(n * (n + 1) * 8)) return fail(GEMMA_HIP_ENOMEM, "lmm_batch: even-ld copy of U");
    HIPCHK(hipMemcpy2DAsync(g_ctx.U_even.p, (n + 1) * 8, g_ctx.U, n * 8, n * 8, n, hipMemcpyDeviceToDevice, s));
    g_ctx.U_even_of = g_ctx.U;
  }
  *U = g_ctx.U_even.as<double>();
  *ld = (long)n + 1;
  return GEMMA_HIP_OK;
}

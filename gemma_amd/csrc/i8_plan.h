// The form of the int8 U^T x product and the launches it takes, as a pure function of the switches and a few integers (no HIP
// include: a plain C++ program can use it, tests/cpp/i8_plan_check.cpp does).  abi_utx.inc.h reserves and launches from the result
// and decides nothing itself; DESIGN 3.7 has the table of forms.
#pragma once

#include <cstddef>

#include "../../include/gemma_hip.h"

namespace gemma_hip {

// tile heights of the left factor (static_assert in abi_utx.inc.h: S2_BM, I8P_BM)
constexpr size_t I8_PLAN_BM_RECORDS = 256, I8_PLAN_BM_BYTES = 128;

// The switches the form depends on, as Knobs::load() reads them (gemma_hip.hip).
struct I8Switches {
  int utx_i8 = 1;         // GEMMA_HIP_UTX_I8: 1 = hard-call batches through the exact int8-digit product, 0 = always the fp64 GEMM
  int sparse = 2;         // GEMMA_HIP_I8_SPARSE: 0 dense mask product, 1 sparse MFMA on byte genotypes, 2 records kernel
  int rows = 16;          // GEMMA_HIP_I8_ROWS: 32 = the records kernel on the 32-row matrix instructions
  int fuse = 1;           // GEMMA_HIP_I8_FUSE: 0 = one int32 plane per digit
  int mdrop = 0;          // GEMMA_HIP_I8_FORM=7g6m: seven digits for the genotype product, the mask product on the upper six
  int complete = 1;       // GEMMA_HIP_I8_COMPLETE: 0 = blocks without a missing call take the mask product like any other block
  int epilogue = 1;       // GEMMA_HIP_I8_EPILOGUE: 0 = every digit plane to memory and the digit combine as a pass of its own
  int epi_depth = 4;      // GEMMA_HIP_I8_EPI_DEPTH: 1 = the epilogue of the records kernel reads the planes back one step ahead
  int direct = 1;         // GEMMA_HIP_I8_DIRECT: 0 = PLINK blocks reach the records through the byte matrix
  int raster = 1;         // GEMMA_HIP_I8_RASTER: row blocks of the cross-XCD raster (unset: S2_DEFAULT_RASTER, put here by load())
  int gm = 0;             // GEMMA_HIP_I8_GM: tile rows per L2 patch of the non-rastered launch
  int overlap = 0;        // GEMMA_HIP_OVERLAP
  int chunks = 4;         // GEMMA_HIP_OVERLAP_CHUNKS
};

// left factor and mask product: dense MFMAs on bytes (i8gemm_packed_kernel_t), the 2:4 sparse MFMA on bytes + mask words
// (i8gemm_sparse.hip.h), 16-byte records of 2-bit genotypes + mask words on 256 x 128 tiles (i8gemm_sparse2*.hip.h)
enum I8Mode { I8_DENSE, I8_SPARSE_BYTES, I8_RECORDS_R32, I8_RECORDS_R16 };
inline I8Mode i8_mode(const I8Switches &k) {
  return k.sparse == 0 ? I8_DENSE : k.sparse == 1 ? I8_SPARSE_BYTES : k.rows == 32 ? I8_RECORDS_R32 : I8_RECORDS_R16;
}

struct I8Form {
  I8Mode mode;
  size_t n, lpad, mrows; // lpad: l rounded up to the tile height; planes hold G rows at row, M rows at lpad + row
  int fuse, digits, nplanes;
  int mdrop;    // 1: the 7g6m form -- plane 0 (digit 0 alone) carries the genotype product only
  int complete; // 1: the records builder flags the block's missing calls and a block without one takes the genotype product alone
                // (Sparse2Args::anymiss): same planes, same U^T x, bit for bit
  int epi;      // 1: plane 0 is launched last, in the epilogue form of the 16-row records kernel, and writes U^T x itself: no digit
                // combine, and the plane buffer holds planes 1 .. nplanes - 1 only
  int c_planes; // planes in memory: nplanes - epi
  int direct;   // 1: a PLINK block's records come straight from its 2-bit rows (plink_records_kernel), no byte matrix
  bool records() const { return mode >= I8_RECORDS_R32; }
  bool sparse() const { return mode != I8_DENSE; }
};

// allow_epi = false: the caller needs the planes and a separate combine; allow_direct = false: it needs the byte matrix (the
// two-block pipe on both counts, abi_lmm_batch.inc.h).  have_map: an indicator map selects the analysed individuals.
inline I8Form i8_form(const I8Switches &k, size_t n, size_t l, int digits, bool have_map, bool allow_epi, bool allow_direct) {
  I8Form f;
  f.mode = i8_mode(k);
  const bool r16 = f.mode == I8_RECORDS_R16;
  const size_t bm = f.records() ? I8_PLAN_BM_RECORDS : I8_PLAN_BM_BYTES;
  f.n = n; f.lpad = (l + bm - 1) / bm * bm; f.mrows = 2 * f.lpad;
  // two digits per int32 output plane while 256 * C_hi + C_lo cannot overflow: n * 2 * 128 * 257 < 2^31
  f.fuse = (k.fuse && (double)n * 2.0 * 128.0 * 257.0 < 2147483648.0) ? 1 : 0;
  f.digits = digits;
  f.nplanes = f.fuse ? (digits + 1) / 2 : digits;
  // the 7g6m form needs plane 0 to be digit 0 alone (odd count, fused planes) and the 16-row records kernel
  f.mdrop = (k.mdrop && f.fuse && digits == 7 && r16) ? 1 : 0;
  f.complete = (k.complete && r16) ? 1 : 0;
  f.epi = (allow_epi && k.epilogue && r16 && f.nplanes >= 2) ? 1 : 0;
  f.c_planes = f.nplanes - f.epi;
  f.direct = (allow_direct && k.direct && f.records() && !have_map) ? 1 : 0;
  return f;
}

enum I8Kernel { I8K_PACKED, I8K_SPARSE, I8K_SPARSE2, I8K_R16, I8K_R16_G, I8K_R16_EP, I8K_R16_EP_G, I8K_COUNT };
struct I8Launch {
  I8Kernel kernel;
  int plane0, planes; // first plane and plane count (grid.y)
  int run_if;         // Sparse2Args::run_if: 0 always, 1 / 2 only when the block has / has not a missing call
  bool writes_utx;    // an epilogue instance: plane 0, behind every other plane in stream order
};

// The launches of one product, in order.  16-row records: the planes above `first` with both products (and, complete-block form,
// once more with the genotype product alone: one of the pair returns at once), then plane 0 where it is launched on its own -- last
// as the epilogue, or (7g6m) from the genotype product alone.  Every other mode is one launch of all planes.
inline int i8_launches(const I8Form &f, I8Launch out[4]) {
  if (f.mode != I8_RECORDS_R16) {
    out[0] = {f.mode == I8_DENSE ? I8K_PACKED : f.mode == I8_SPARSE_BYTES ? I8K_SPARSE : I8K_SPARSE2, 0, f.nplanes, 0, false};
    return 1;
  }
  const int first = (f.epi || f.mdrop) ? 1 : 0, both = f.complete ? 1 : 0;
  int k = 0;
  out[k++] = {I8K_R16, first, f.nplanes - first, both, false};
  if (f.complete) out[k++] = {I8K_R16_G, first, f.nplanes - first, 2, false};
  if (f.mdrop) out[k++] = {f.epi ? I8K_R16_EP_G : I8K_R16_G, 0, 1, 0, f.epi != 0};
  else if (f.epi) {
    out[k++] = {I8K_R16_EP, 0, 1, both, true};
    if (f.complete) out[k++] = {I8K_R16_EP_G, 0, 1, 2, true};
  }
  return k;
}

// Row chunks of a PLINK block on two streams (GEMMA_HIP_OVERLAP, lmm_batch_plink_chunked): at least two tile rows per chunk
inline int i8_chunks(const I8Switches &k, size_t l) {
  if (!k.overlap || k.utx_i8 != 1 || i8_mode(k) < I8_RECORDS_R32) return 1;
  int q = k.chunks < 1 ? 1 : k.chunks > 16 ? 16 : k.chunks;
  while (q > 1 && l < (size_t)q * 2 * I8_PLAN_BM_RECORDS) --q;
  return q;
}

// the two-block pipe (gemma_hip_lmm_batch_pipe_d) has something to pipeline: PLINK blocks on the records kernel
inline bool i8_pipe_eligible(const I8Switches &k, int kind) {
  return kind == GEMMA_GENO_PLINK_2BIT && k.utx_i8 == 1 && i8_mode(k) >= I8_RECORDS_R32;
}

} // namespace gemma_hip

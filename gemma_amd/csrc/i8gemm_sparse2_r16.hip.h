// The records kernel (i8gemm_sparse2.hip.h: same records, same digit planes, same int32 planes out, same LDS stages and LDS-DMA
// pipeline, wavefronts 8 x 1) on the 16-ROW matrix instructions: genotype product on v_mfma_i32_16x16x64_i8, mask product on
// v_smfmac_i32_16x16x128_i8.  The shipped form since the end of round 4 (GEMMA_HIP_I8_ROWS=32 selects the 32-row kernel).
//
// Why: the kernel is power-limited, and how much clock the chip gives up depends on the instruction and on the VALUES it multiplies
// (DESIGN.md 3.1c).  With operands in registers and nothing else running v_mfma_i32_32x32x32_i8 sustains 3.70 POP/s on full-range
// digit values and the 16x16x64 form 4.72 (profiles/r04_mfma_power_probe.txt); this kernel needs 40.8 ms of schedule (all-zero
// digits; the 32-row kernel 38.7) and 49.8 ms with real digits where the 32-row kernel needs 54.6 on the same box
// (profiles/r04_i8_g16s_prototype.txt).  Every entry of every plane equals the 32-row kernel's on ten shapes -- 2 454 061 056 entries
// at n = 20 000, odd digit counts, unfused planes, K loops of 1 - 3 tiles, ragged tiles (profiles/r04_i8_r16_full_compare.txt,
// scripts/i8_kernel_bench.hip variant 7 with FULLCMP=1).
//
// Layouts (profiles/r04_mfma16_layout_probe.txt, r04_smfmac16_layout_probe.txt).  Lane l = (r16 = l % 16, q = l / 16).
//   dense 16x16x64, pair P of K-steps: lane q multiplies the 16 K bytes 64 P + 16 q .. of row / column r16 -- K-step 2 P + (q >> 1),
//     half q & 1: left operand = word q >> 1 of the record chunk 2 P + (q & 1) of the row, right operand F[P] = chunk 4 P + q of the
//     digit row;
//   sparse 16x16x128, the whole K-tile: lane quarter q of the left operand covers the 32 logical K bytes of K-step q (kept slots
//     0..7 its first 16, 8..15 its second 16) = index word and kept bits of the record chunk q of the row -- which the records
//     already hold; its right operand in lane (c16, qb) is (F[0], F[1]) of the SAME lane: chunk beta of quarter qb multiplies
//     quarter qa = (qb >> 1) + 2 beta, slots 8 (qb & 1) ..: K bytes 64 beta + 16 qb .. = F[beta] of lane qb.  So one 8-register
//     tuple per 16-column sub-block serves two dense and one sparse instruction per group of 16 rows: no lane exchange, no second
//     set of LDS reads.
// Per K-tile and wavefront: 4 record reads + 16 digit reads (ds_read_b128), 32 dense + 16 sparse instructions, 4 LDS-DMA pieces, one
// counted s_waitcnt vmcnt(8) + one s_barrier; tests/test_isa_schedule.py holds the built loop to that.
#pragma once
#include <type_traits>
#include "i8gemm_sparse2.hip.h"
#include "i8gemm_sparse2_r16.h"

#ifndef S2_R16_PREP_SPREAD
#define S2_R16_PREP_SPREAD 0
#endif
// timing experiments only (scripts/i8_kernel_bench.hip, round 6 power table): the sparse (mask) / the dense (genotype) matrix
// instructions compiled out -- results wrong, everything else of the loop (LDS reads, LDS-DMA, operand preparation) unchanged
#ifndef S2_R16_ABL_NO_S
#define S2_R16_ABL_NO_S 0
#endif
#ifndef S2_R16_ABL_NO_D
#define S2_R16_ABL_NO_D 0
#endif

namespace gemma_hip {

// WITH_S = false: the genotype product alone (round 6, the "7g6m" form: the lowest of seven digits is multiplied with the genotypes
// only -- its mask term is below the rounding of the other six): no sparse instruction, no mask accumulators, no M rows
// written.  The same loop otherwise; one source so that the two cannot drift apart.
//
// COMBINE = true: the launch of plane 0 (the lowest digit or digit pair), queued on the stream behind the launch of planes
// nplanes - 1 .. 1.  Its workgroups keep plane 0 in their accumulators, read the other planes of their tile back, run the digit
// combine (i8gemm.hip.h: i8_combine_kernel -- the same operations in the same order, so the same doubles) and store U^T x
// themselves: plane 0 never goes to memory and the separate pass over the planes is not run.  The K loop is the same source.
template <bool WITH_S, bool COMBINE = false>
__device__ __forceinline__ void s2_r16_body(const Sparse2Args &g) {
  extern __shared__ __attribute__((aligned(1024))) int8_t i8lds[];
  constexpr bool NO_S = !WITH_S || S2_R16_ABL_NO_S;
  if (g.run_if) { // Sparse2Args::anymiss: the form that is not this block's returns before it touches anything
    const int any = __builtin_amdgcn_readfirstlane(*g.anymiss);
    if ((g.run_if == 1) != (any != 0)) return;
  }
  int tm, tn;
  if (g.tile_map) {
    const int2 t2 = g.tile_map[blockIdx.x];
    tm = __builtin_amdgcn_readfirstlane(t2.x);
    tn = __builtin_amdgcn_readfirstlane(t2.y);
  } else {
    const int nwg = gridDim.x, b = blockIdx.x;
    const int q_ = nwg >> 3, r = nwg & 7, x = b & 7, o = b >> 3;
    const int L = (x < r ? x * (q_ + 1) : r * (q_ + 1) + (x - r) * q_) + o;
    const int GM = g.gm > 0 ? g.gm : 8;
    const int per_group = GM * g.tiles_n;
    const int grp = L / per_group;
    const int first_m = grp * GM;
    const int gsz = min(g.tiles_m - first_m, GM);
    const int in = L - grp * per_group;
    tm = first_m + in % gsz;
    tn = in / gsz;
  }
  const int plane = blockIdx.y + g.plane0;
  const int odd = g.digits & 1;
  const int d_first = g.fuse ? (odd ? (plane == 0 ? 0 : 2 * plane) : 2 * plane + 1) : plane;
  const int nd = (g.fuse && !(odd && plane == 0)) ? 2 : 1;
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r16 = lane & 15, q = lane >> 4;

  const uint4 *asrc[2];
  const int8_t *bsrc[2];
  int adst[2], bdst[2];
#define GS_INIT_SRC(DIGIT)                                                                                        \
  do {                                                                                                            \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) {                                                               \
      const int qp = 2 * wave + j;                                                                                \
      const int row = 16 * qp + (lane >> 2);                                                                      \
      asrc[j] = g.AM + ((long)tm * g.nk * S2_BM + row) * 4 + ((lane & 3) ^ ((row >> 2) & 3));                     \
      adst[j] = qp * 1024;                                                                                        \
      const int col = 8 * qp + (lane >> 3);                                                                       \
      bsrc[j] = g.Bt + (long)(DIGIT) * g.strideB + ((long)tn * S2_BN + col) * g.ldk + 16 * ((lane & 7) ^ ((col >> 1) & 7)); \
      bdst[j] = S2_AMB + qp * 1024;                                                                               \
    }                                                                                                             \
  } while (0)
  // byte offsets inside a stage: record chunk (q & 1) + 2 P of row wave * 32 + r16 (second row group: + 1024), digit chunk 4 P + q of
  // column r16 (sub-block sb: + 2048 sb; the swizzles do not change with either)
  int ro[2], fo[2];
  {
    const int row = wave * 32 + r16;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      ro[p] = row * 64 + (((2 * p + (q & 1)) ^ ((row >> 2) & 3)) << 4);
      fo[p] = S2_AMB + r16 * 128 + (((4 * p + q) ^ ((r16 >> 1) & 7)) << 4);
    }
  }

  i32x4 accg[2][8], accm[2][8];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) { accg[i][j] = (i32x4){0, 0, 0, 0}; accm[i][j] = (i32x4){0, 0, 0, 0}; }

  i32x4 rec[2][2];  // records of the NEXT K-tile [row group][pair]: chunk 2 P + (q & 1)
  i32x4 ga[2][2];   // genotype operands [row group][pair]
  i32x4 ms[2];      // kept values of K-step q [row group]
  int ix[2];        // index words of K-step q [row group]
  i32x8 T[4];       // digit fragments (F[0], F[1]) of four sub-blocks in flight (ring: slot = sub-block % 4, the same in every K-tile)

#define GS_DMA_A(j, SOFF)                                                                                         \
  do {                                                                                                            \
    __builtin_amdgcn_global_load_lds((gemma_gptr_t)asrc[j], (gemma_lptr_t)(i8lds + (SOFF) + adst[j]), 16, 0, 0);  \
    asrc[j] += S2_BM * 4;                                                                                         \
  } while (0)
#define GS_DMA_B(j, SOFF)                                                                                         \
  do {                                                                                                            \
    __builtin_amdgcn_global_load_lds((gemma_gptr_t)bsrc[j], (gemma_lptr_t)(i8lds + (SOFF) + bdst[j]), 16, 0, 0);  \
    bsrc[j] += I8_BK;                                                                                             \
  } while (0)
#define GS_RREC(SOFF, i, P) rec[i][P] = *reinterpret_cast<const i32x4 *>(i8lds + (SOFF) + ro[P] + (i) * 1024)
// sub-block SB of the stage into ring slot SL
#define GS_RT(SOFF, SB, SL)                                                                                       \
  do {                                                                                                            \
    const i32x4 x_ = *reinterpret_cast<const i32x4 *>(i8lds + (SOFF) + fo[0] + (SB) * 2048);                      \
    const i32x4 y_ = *reinterpret_cast<const i32x4 *>(i8lds + (SOFF) + fo[1] + (SB) * 2048);                      \
    T[SL] = __builtin_shufflevector(x_, y_, 0, 1, 2, 3, 4, 5, 6, 7);                                              \
  } while (0)
// operands of a K-tile from its records: genotype word q >> 1 of (pair P, half q & 1); index word and kept bits of K-step q = the
// record of pair q >> 1 (its half is q & 1 by construction)
#define GS_PREP(i)                                                                                                \
  do {                                                                                                            \
    ga[i][0] = s2_unpack_g((q >> 1) ? rec[i][0][1] : rec[i][0][0]);                                               \
    ga[i][1] = s2_unpack_g((q >> 1) ? rec[i][1][1] : rec[i][1][0]);                                               \
    ix[i] = (q >> 1) ? rec[i][1][2] : rec[i][0][2];                                                               \
    ms[i] = s2_expand((q >> 1) ? rec[i][1][3] : rec[i][0][3]);                                                    \
    asm volatile("" ::"v"(rec[i][0]), "v"(rec[i][1]));                                                            \
  } while (0)
// the same in pieces (S2_R16_PREP_SPREAD): each operand register is rebuilt right behind the LAST matrix instruction of the K-tile
// that reads it (step 7: D(0,P0) D(1,P0) D(0,P1) D(1,P1) S(0) S(1)), so the 66 VALU instructions of the preparation sit between
// the step's matrix instructions instead of behind them
#define GS_PREP_G(i, P) ga[i][P] = s2_unpack_g((q >> 1) ? rec[i][P][1] : rec[i][P][0])
#define GS_PREP_M(i)                                                                                              \
  do {                                                                                                            \
    ix[i] = (q >> 1) ? rec[i][1][2] : rec[i][0][2];                                                               \
    ms[i] = s2_expand((q >> 1) ? rec[i][1][3] : rec[i][0][3]);                                                    \
    asm volatile("" ::"v"(rec[i][0]), "v"(rec[i][1]));                                                            \
  } while (0)
#define GS_D(i, SB, P, SL)                                                                                        \
  do {                                                                                                            \
    if (!S2_R16_ABL_NO_D)                                                                                         \
      asm volatile("s_nop 1\n\tv_mfma_i32_16x16x64_i8 %0, %1, %2, %0"                                             \
                   : "+v"(accg[i][SB])                                                                            \
                   : "v"(ga[i][P]), "v"(__builtin_shufflevector(T[SL], T[SL], 4 * (P), 4 * (P) + 1, 4 * (P) + 2, 4 * (P) + 3))); \
  } while (0)
#define GS_S(i, SB, SL)                                                                                           \
  do {                                                                                                            \
    if (!NO_S)                                                                                                    \
      asm volatile("s_nop 1\n\tv_smfmac_i32_16x16x128_i8 %0, %1, %2, %3" : "+v"(accm[i][SB]) : "v"(ms[i]), "v"(T[SL]), "v"(ix[i])); \
  } while (0)
// the six matrix instructions of sub-block SB (ring slot SL); X: statements issued behind the first two
#define GS_STEP(SB, SL, X)                                                                                        \
  do {                                                                                                            \
    GS_D(0, SB, 0, SL); GEMMA_SB();                                                                               \
    GS_D(1, SB, 0, SL); X; GEMMA_SB();                                                                            \
    GS_D(0, SB, 1, SL); GEMMA_SB();                                                                               \
    GS_D(1, SB, 1, SL); GEMMA_SB();                                                                               \
    GS_S(0, SB, SL); GEMMA_SB();                                                                                  \
    GS_S(1, SB, SL); GEMMA_SB();                                                                                  \
  } while (0)
// One K-tile from stage SC; at entry sub-blocks 0, 1, 2 are in ring slots 0, 1, 2 and the operands of this tile are prepared.
// Sub-block s + 3 is requested behind the first instructions of step s (its slot was freed by step s - 1).  The reads of stage SC
// end in step 4; the rendezvous for tile t + 1 follows step 4; steps 5, 6, 7 request its records and its first three sub-blocks.
#define GS_KTILE(SC, SN, SD, MORE, LOAD3, VMW)                                                                    \
  do {                                                                                                            \
    GS_STEP(0, 0, { GS_RT(SC, 3, 3); if (LOAD3) GS_DMA_A(0, SD); });                                               \
    GS_STEP(1, 1, { GS_RT(SC, 4, 0); if (LOAD3) GS_DMA_A(1, SD); });                                               \
    GS_STEP(2, 2, { GS_RT(SC, 5, 1); if (LOAD3) GS_DMA_B(0, SD); });                                               \
    GS_STEP(3, 3, { GS_RT(SC, 6, 2); if (LOAD3) GS_DMA_B(1, SD); });                                               \
    GS_STEP(4, 0, { GS_RT(SC, 7, 3); });                                                                           \
    asm volatile("s_waitcnt vmcnt(" #VMW ")" ::: "memory");                                                       \
    __builtin_amdgcn_s_barrier();                                                                                 \
    GEMMA_SB();                                                                                                   \
    GS_STEP(5, 1, { if (MORE) { GS_RREC(SN, 0, 0); GS_RREC(SN, 0, 1); GS_RREC(SN, 1, 0); GS_RREC(SN, 1, 1);       \
                                GS_RT(SN, 0, 0); } });                                                             \
    GS_STEP(6, 2, { if (MORE) { GS_RT(SN, 1, 1); } });                                                             \
    if (S2_R16_PREP_SPREAD && (MORE)) {                                                                           \
      GS_D(0, 7, 0, 3); GEMMA_SB();                                                                               \
      GS_D(1, 7, 0, 3); { GS_RT(SN, 2, 2); GS_PREP_G(0, 0); } GEMMA_SB();                                          \
      GS_D(0, 7, 1, 3); { GS_PREP_G(1, 0); } GEMMA_SB();                                                           \
      GS_D(1, 7, 1, 3); { GS_PREP_G(0, 1); } GEMMA_SB();                                                           \
      GS_S(0, 7, 3); { GS_PREP_G(1, 1); } GEMMA_SB();                                                              \
      GS_S(1, 7, 3); { GS_PREP_M(0); } GEMMA_SB();                                                                 \
      { GS_PREP_M(1); } GEMMA_SB();                                                                                \
    } else {                                                                                                      \
      GS_STEP(7, 3, { if (MORE) { GS_RT(SN, 2, 2); } });                                                           \
      if (MORE) { GS_PREP(0); GS_PREP(1); }                                                                       \
      GEMMA_SB();                                                                                                 \
    }                                                                                                             \
  } while (0)

  if (wave >= 4) __builtin_amdgcn_s_setprio(1);
  const int nk = g.nk;
  for (int dd = 0; dd < nd; ++dd) {
    if (dd > 0) {
      asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            accg[i][j][r] <<= 8;
            if (WITH_S) accm[i][j][r] <<= 8;
          }
    }
    GS_INIT_SRC(d_first - dd);
    // prologue: tiles 0 .. NST - 2 in flight, tile 0 landed
#pragma unroll
    for (int j = 0; j < 2; ++j) { GS_DMA_A(j, 0); GS_DMA_B(j, 0); }
    if (nk > 1) {
#pragma unroll
      for (int j = 0; j < 2; ++j) { GS_DMA_A(j, S2_STAGE); GS_DMA_B(j, S2_STAGE); }
    }
    if (nk > 2) {
#pragma unroll
      for (int j = 0; j < 2; ++j) { GS_DMA_A(j, 2 * S2_STAGE); GS_DMA_B(j, 2 * S2_STAGE); }
    }
    if (S2_R16_NST == 5 && nk > 3) {
#pragma unroll
      for (int j = 0; j < 2; ++j) { GS_DMA_A(j, 3 * S2_STAGE); GS_DMA_B(j, 3 * S2_STAGE); }
      asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    } else if (nk > 2) {
      asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else if (nk > 1) {
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    GEMMA_SB();
    GS_RT(0, 0, 0);
    GS_RT(0, 1, 1);
    GS_RT(0, 2, 2);
    GS_RREC(0, 0, 0); GS_RREC(0, 0, 1); GS_RREC(0, 1, 0); GS_RREC(0, 1, 1);
    GS_PREP(0);
    GS_PREP(1);
    GEMMA_SB();

    // stage byte offsets: tile t, t + 1, ..., the LDS-DMA target (the stage tile t - 1 was read from)
    int sc = 0, sn = S2_STAGE, s2 = 2 * S2_STAGE, s3 = 3 * S2_STAGE, sd = (S2_R16_NST - 1) * S2_STAGE;
#define GS_ROTATE()                                                                                               \
  do {                                                                                                            \
    const int tmp = sc;                                                                                           \
    sc = sn; sn = s2;                                                                                             \
    if (S2_R16_NST == 5) { s2 = s3; s3 = sd; } else { s2 = sd; }                                                  \
    sd = tmp;                                                                                                     \
  } while (0)
    int kt = 0;
    if (S2_R16_NST == 5) {
      for (; kt + 4 < nk; ++kt) {
        GS_KTILE(sc, sn, sd, true, true, 12);
        GS_ROTATE();
      }
      if (nk >= 4) {
        GS_KTILE(sc, sn, sd, true, false, 8);
        GS_ROTATE();
      }
    } else {
      for (; kt + 3 < nk; ++kt) {
        GS_KTILE(sc, sn, sd, true, true, 8);
        GS_ROTATE();
      }
    }
    if (nk >= 3) {
      GS_KTILE(sc, sn, sd, true, false, 4);
      GS_ROTATE();
    }
    if (nk >= 2) {
      GS_KTILE(sc, sn, sd, true, false, 0);
      GS_ROTATE();
    }
    GS_KTILE(sc, sn, sd, false, false, 0);
#undef GS_ROTATE
  }

  asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
  if constexpr (COMBINE) {
    // Entry (i, sb, r) of this lane: row tm * 256 + wave * 32 + 16 i + 4 q + r, column tn * 128 + 16 sb + r16.  A batch is the 8
    // entries (i, sb = 2 h, 2 h + 1, r); per batch and plane 8 G + 8 M dwords are requested ahead of the Horner step that uses them:
    // four steps ahead in the bodies for three and four planes (ep_fixed), one step in the generic body (16 - 32 loads per
    // wavefront in flight; 16 entries a batch spill).  Every load is issued behind the last K-tile: the counted waits of the loop
    // never see one.
    const int np = g.nplanes;
    const bool load_m = !(g.anymiss && __builtin_amdgcn_readfirstlane(*g.anymiss) == 0); // complete block: no M row was written
    const double w_hi = g.fuse ? 65536.0 : 256.0;          // planes above plane 0 sit two digits apart when fused
    const double w0 = (g.fuse && !odd) ? 65536.0 : 256.0;  // an odd digit count leaves plane 0 one digit wide
    // addresses: a uniform base per (plane, row, sub-block) in scalar registers + ONE 32-bit lane offset per array, so that the
    // epilogue's addresses take no vector registers beside the accumulators (4 q rows + r16 columns: far below 2^32 bytes)
    const long row_w = (long)tm * S2_BM + wave * 32, col_w = (long)tn * S2_BN;
    const long row_l = row_w + 4 * q, col_l = col_w + r16; // of this lane: + 16 i + r, + 16 sb
    const unsigned lo_c = (unsigned)((4 * q * g.ldc + r16) * 4), lo_x = (unsigned)((4 * q * g.ldx + r16) * 8);
#define EP_AT(T, BASE, LO) (*(T *)((const char *)(BASE) + (LO)))
#define EP_LOAD(DG, DM, I, H, P)                                                                                  \
  do {                                                                                                            \
    const int *cp_ = g.C + (long)(P) * g.strideC + (row_w + 16 * (I)) * g.ldc + col_w + 32 * (H);                 \
    _Pragma("unroll") for (int k_ = 0; k_ < 2; ++k_) _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {           \
      DG[4 * k_ + r_] = EP_AT(const int, cp_ + r_ * g.ldc + 16 * k_, lo_c);                                       \
      DM[4 * k_ + r_] = load_m ? EP_AT(const int, cp_ + (g.m_row0 + r_) * g.ldc + 16 * k_, lo_c) : 0;             \
    }                                                                                                             \
  } while (0)
    // The fused forms (three planes: six digits, the headline shape; four: seven digits) with the plane read-back EP_DEPTH steps
    // ahead (round 8, Sparse2Args::epi_depth).  A workgroup's 16 (np = 3) dependent round trips of ~1.6 us were the whole 26 us of
    // this epilogue; the 768 KiB they move take 5 us.  Room for 64 dwords in flight: the mask accumulators -- 64 registers x 512
    // lanes x 4 B = the 128 KiB of LDS, which hold nothing behind the K loop -- are parked in a lane-private LDS slot (slot j of
    // lane t at (512 j + t) * 16: consecutive lanes 16 bytes apart, conflict-free 16-byte accesses) and read back batch by batch.
    // The Horner steps, the last step and their order are the ones of the generic body below: only when the loads are issued differs.
    constexpr int EP_DEPTH = 4;
    if constexpr (WITH_S) {
      // every wavefront is behind its last read of the K loop's stages (their last reads sit before the loop's last barrier; this
      // one costs nothing and does not depend on that).  The generic body reads its mask accumulators from there as well: with
      // them in registers it had five registers to spare, and a second body in the kernel made it spill.
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 16; ++j) *reinterpret_cast<i32x4 *>(i8lds + ((j * 512 + t) << 4)) = accm[j >> 3][j & 7];
      GEMMA_SB();
    }
    // LM: the planes have M rows (load_m) -- a template parameter here: a run-time choice per load is a branch and a full wait per load
    // Addresses: per step two uniform bases (G rows, M rows) that the compiler must keep in scalar registers -- through
    // readfirstlane, or it folds them into per-load 64-bit vector addresses: 66 registers -- plus one of four 32-bit lane offsets
    // (row r of the lane's four; 3 ldc ints + the lane's own stay far below 2^32 bytes: fused planes mean n < 32 640)
    // (the integer round trip drops the address space: named again, or the loads become FLAT ones that count on lgkmcnt as well)
    typedef const __attribute__((address_space(1))) int *ep_gint_t;
    typedef const __attribute__((address_space(1))) char *ep_gchar_t;
#define EP_UNI(PTR)                                                                                               \
  ((ep_gint_t)(((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned long)(PTR) >> 32)) << 32) | \
               (unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned long)(PTR))))
#define EP_ATG(BASE, LO) (*(ep_gint_t)((ep_gchar_t)(BASE) + (LO)))
#define EP_LOADF(DG, DM, I, H, P)                                                                                 \
  do {                                                                                                            \
    const int *cp_ = g.C + (long)(P) * g.strideC + (row_w + 16 * (I)) * g.ldc + col_w + 32 * (H);                 \
    const ep_gint_t cg_ = EP_UNI(cp_), cm_ = EP_UNI(cp_ + g.m_row0 * g.ldc);                                      \
    _Pragma("unroll") for (int k_ = 0; k_ < 2; ++k_) _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {           \
      DG[4 * k_ + r_] = EP_ATG(cg_ + 16 * k_, lo_r[r_]);                                                          \
      if constexpr (LM) DM[4 * k_ + r_] = EP_ATG(cm_ + 16 * k_, lo_r[r_]);                                        \
      else DM[4 * k_ + r_] = 0;                                                                                   \
    }                                                                                                             \
  } while (0)
    auto ep_fixed = [&](auto np_tag, auto lm_tag) {
      constexpr int NP = decltype(np_tag)::value, SPB = NP - 1, NS = 8 * SPB; // plane steps per batch, steps
      constexpr bool LM = decltype(lm_tag)::value;
      // the lane's own offsets once more, from laundered lane coordinates: as common subexpressions of this body and the generic
      // one the compiler computes them in front of the branch and keeps them across the generic body, which has no register to spare
      int qf = q, cf = r16;
      asm volatile("" : "+v"(qf), "+v"(cf));
      const long row_lf = row_w + 4 * qf, col_lf = col_w + cf;
      // rows / columns of the block from the lane's first on (<= 0: none), as ints: the bounds checks of the 64 entries compare
      // constants with these two registers instead of keeping sixteen 64-bit indices
      const int rows_left = (int)min(g.l - row_lf, 64L), cols_left = (int)min(g.n - col_lf, 256L);
      const unsigned lo_xf = (unsigned)((4 * qf * g.ldx + cf) * 8);
      unsigned lo_r[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) lo_r[r] = (unsigned)(((4 * qf + r) * g.ldc + cf) * 4);
      // mean_s of the lane's 8 rows and 1 / q_j of its 8 columns first: a load in a batch's last step would be the youngest of
      // everything in flight, and waiting for it is waiting for all the planes requested ahead
      double msv[2][4], qv[8];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          msv[i][r] = g.mean[row_lf + min(16 * i + r, rows_left - 1)]; // clamped (to l - 1, n - 1), not guarded: sixteen loads back
#pragma unroll                                                           // to back, one wait; what is outside is never stored
      for (int sb = 0; sb < 8; ++sb) qv[sb] = g.qinv[col_lf + min(16 * sb, cols_left - 1)];
      // The body is straight-line code: without the scheduling barriers the compiler moves the loads of later steps up as far as
      // their addresses allow and spills what they hold (555 scratch accesses in the first build).  The order is the source order.
      GEMMA_SB();
      int lg[EP_DEPTH][8], lm[EP_DEPTH][8]; // step s = SPB b + j (batch b, plane NP - 1 - j) lands in slot s % EP_DEPTH
#pragma unroll
      for (int s = 0; s < EP_DEPTH; ++s) {
        EP_LOADF(lg[s], lm[s], (s / SPB) >> 2, (s / SPB) & 3, NP - 1 - s % SPB);
        GEMMA_SB();
      }
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const int i = b >> 2, h = b & 3;
        double tg[8], tk[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) tg[e] = tk[e] = 0.0;
#pragma unroll
        for (int j = 0; j < SPB; ++j) {
          const int s = SPB * b + j, sl = s % EP_DEPTH, s2 = s + EP_DEPTH;
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            tg[e] = tg[e] * w_hi + (double)lg[sl][e];
            tk[e] = tk[e] * w_hi + (double)lm[sl][e];
          }
          GEMMA_SB();
          if (s2 < NS) EP_LOADF(lg[sl], lm[sl], (s2 / SPB) >> 2, (s2 / SPB) & 3, NP - 1 - s2 % SPB);
          GEMMA_SB();
        }
        i32x4 mk[2] = {(i32x4){0, 0, 0, 0}, (i32x4){0, 0, 0, 0}};
        if constexpr (WITH_S) {
#pragma unroll
          for (int k = 0; k < 2; ++k) mk[k] = *reinterpret_cast<const i32x4 *>(i8lds + (((8 * i + 2 * h + k) * 512 + t) << 4));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const bool row_in = 16 * i + r < rows_left;
          const double ms = msv[i][r] * g.m_scale;
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int e = 4 * k + r, sb = 2 * h + k;
            tg[e] = tg[e] * w0 + (double)accg[i][sb][r];
            tk[e] = tk[e] * w0 + (double)mk[k][r];
            if (row_in && 16 * sb < cols_left)
              EP_AT(double, g.UtX + (row_w + 16 * i + r) * g.ldx + col_w + 16 * sb, lo_xf) =
                  fma(ms, tk[e], tg[e]) * qv[sb];
          }
        }
        GEMMA_SB();
      }
    };
    if (g.epi_depth > 1 && np == 3) {
      if (load_m) ep_fixed(std::integral_constant<int, 3>(), std::true_type());
      else ep_fixed(std::integral_constant<int, 3>(), std::false_type());
    } else if (g.epi_depth > 1 && np == 4) {
      if (load_m) ep_fixed(std::integral_constant<int, 4>(), std::true_type());
      else ep_fixed(std::integral_constant<int, 4>(), std::false_type());
    } else {
    // every other plane count (unfused planes, n = 50 000) and GEMMA_HIP_I8_EPI_DEPTH=1: the schedule of round 7, one step ahead
    int cg[8], cm[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cg[e] = cm[e] = 0;
    if (np > 1) EP_LOAD(cg, cm, 0, 0, np - 1);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int i = b >> 2, h = b & 3;
      double tg[8], tk[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) tg[e] = tk[e] = 0.0;
      for (int p = np - 1; p >= 1; --p) {
        int ng[8], nm[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) ng[e] = nm[e] = 0;
        if (p > 1) EP_LOAD(ng, nm, i, h, p - 1);
        else if (b < 7) EP_LOAD(ng, nm, (b + 1) >> 2, (b + 1) & 3, np - 1);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          tg[e] = tg[e] * w_hi + (double)cg[e];
          tk[e] = tk[e] * w_hi + (double)cm[e];
          cg[e] = ng[e];
          cm[e] = nm[e];
        }
      }
      i32x4 mk[2] = {(i32x4){0, 0, 0, 0}, (i32x4){0, 0, 0, 0}};
      if constexpr (WITH_S) {
#pragma unroll
        for (int k = 0; k < 2; ++k) mk[k] = *reinterpret_cast<const i32x4 *>(i8lds + (((8 * i + 2 * h + k) * 512 + t) << 4));
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool row_in = row_l + 16 * i + r < g.l;
        const double ms = row_in ? EP_AT(const double, g.mean + row_w + 16 * i + r, (unsigned)(32 * q)) * g.m_scale : 0.0;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int e = 4 * k + r, sb = 2 * h + k;
          const int m0 = mk[k][r];
          tg[e] = tg[e] * w0 + (double)accg[i][sb][r];
          tk[e] = tk[e] * w0 + (double)m0;
          if (row_in && col_l + 16 * sb < g.n)
            EP_AT(double, g.UtX + (row_w + 16 * i + r) * g.ldx + col_w + 16 * sb, lo_x) =
                fma(ms, tk[e], tg[e]) * EP_AT(const double, g.qinv + col_w + 16 * sb, (unsigned)(8 * r16));
        }
      }
    }
    }
#undef EP_AT
#undef EP_LOAD
#undef EP_LOADF
#undef EP_UNI
#undef EP_ATG
  } else {
    int *Cg = g.C + (long)plane * g.strideC;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int sb = 0; sb < 8; ++sb) {
        const long col = (long)tn * S2_BN + 16 * sb + r16;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const long row = (long)tm * S2_BM + wave * 32 + 16 * i + 4 * q + r;
          Cg[row * g.ldc + col] = accg[i][sb][r];
          if (WITH_S) Cg[(g.m_row0 + row) * g.ldc + col] = accm[i][sb][r];
        }
      }
  }
#undef GS_INIT_SRC
#undef GS_DMA_A
#undef GS_DMA_B
#undef GS_RREC
#undef GS_RT
#undef GS_PREP
#undef GS_PREP_G
#undef GS_PREP_M
#undef GS_D
#undef GS_S
#undef GS_STEP
#undef GS_KTILE
}

__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_kernel(Sparse2Args g) { s2_r16_body<true>(g); }
// the genotype product alone (plane 0 of the 7g6m form)
__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_g_kernel(Sparse2Args g) { s2_r16_body<false>(g); }
// plane 0 with the digit combine as its epilogue (Sparse2Args::UtX): both products / the genotype product alone
__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_ep_kernel(Sparse2Args g) { s2_r16_body<true, true>(g); }
__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_r16_ep_g_kernel(Sparse2Args g) { s2_r16_body<false, true>(g); }

} // namespace gemma_hip

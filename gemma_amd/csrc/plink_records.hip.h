// PLINK 2-bit rows -> the 16-byte records of the records kernel (i8gemm_sparse2.hip.h) in ONE pass, without the byte matrix.
//
// ingest_i8_kernel writes one byte g | m << 4 per call (402 MB per 20 000 x 20 000 block) and sparse2_meta_kernel reads them back
// to write 203 MB of records; nothing else on the records path needs the bytes except the surplus kernels on the few rows that
// dropped a call (i8gemm_sparse.hip.h: they read the 2-bit rows instead, SurplusPlink).  Here a wavefront takes one SNP row and a
// lane one record chunk at a time: 100 MB of 2-bit rows in, 203 MB of records out.
//
// The records are sparse2_meta_kernel's byte for byte, padding included: rows l .. lpad, individuals n .. ldk and the calls
// behind a ragged last byte give genotype 0, kept bits 0 and the index word 0xCCCCCCCC (p0 = 0, p1 = 3 in every nibble) -- what
// the zero bytes of the packed matrix give.  The row sums are integers, so mean_s = tot / (n - miss) is the double
// ingest_i8_kernel writes.  Lane 0 writes the row's dropped-call count: no atomics, no memset of the counters.
//
// The word arithmetic (pr_*) is host code as well: tests/host/plink_records_harness.cpp holds it to a call-by-call restatement
// of the two kernels it replaces (tests/test_plink_records_words.py; as a program of its own, over every byte pattern).
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include "i8gemm_sparse2.hip.h"
#include "plink_records.h"
#define PR_HD __host__ __device__ __forceinline__
#else
#define PR_HD inline
#endif

namespace gemma_hip {

PR_HD int pr_popc(unsigned v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popc(v);
#else
  return __builtin_popcount(v);
#endif
}

// 16 calls of a .bed word (call q at bits 2 q; code 0 -> 2, 1 -> missing, 2 -> 1, 3 -> 0; the first nvalid calls exist):
// *val = the 2-bit values at bits 2 q (0 for a missing call), *miss = bit 2 q set for a missing call
PR_HD void pr_decode(unsigned w, int nvalid, unsigned *val, unsigned *miss) {
  const unsigned valid = nvalid >= 16 ? 0x55555555u : (nvalid <= 0 ? 0u : ((1u << (2 * nvalid)) - 1u) & 0x55555555u);
  const unsigned lo = w & 0x55555555u, hi = (w >> 1) & 0x55555555u;
  const unsigned one = hi & ~lo & valid, two = ~(lo | hi) & valid;
  *val = one | (two << 1);
  *miss = lo & ~hi & valid;
}
// sum of the 16 values of pr_decode's *val
PR_HD int pr_valsum(unsigned val) { return pr_popc(val & 0x55555555u) + 2 * pr_popc(val & 0xAAAAAAAAu); }

// genotype word of a record: individual 4 i + j of the lane's 16 at bits 8 j + 2 i -- the 4 x 4 transpose of the 2-bit fields of
// the source order (individual 4 i + j at bits 8 i + 2 j), as two delta swaps
PR_HD unsigned pr_genoword(unsigned val) {
  unsigned t = ((val >> 6) ^ val) & 0x00CC00CCu;
  val ^= t ^ (t << 6);
  t = ((val >> 12) ^ val) & 0x0000F0F0u;
  val ^= t ^ (t << 12);
  return val;
}

// The mask word of 32 individuals from the missing bits of their two .bed words (m[j]: individuals 16 j .. 16 j + 15, bit 2 q):
// index nibbles and kept bits as sparse2_meta_kernel writes them, the four groups of a word side by side (one bit per byte).
// Returns the calls the 2-of-4 operand drops.
PR_HD int pr_maskword(unsigned m0, unsigned m1, unsigned *idx_out, unsigned *bits_out) {
  const unsigned K = 0x01010101u;
  unsigned idx = 0, bits = 0;
  int surplus = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 2; ++j) {
    const unsigned m = j ? m1 : m0;
    const unsigned a = m & K, b = (m >> 2) & K, c = (m >> 4) & K, d = (m >> 6) & K; // call 0 .. 3 of group 4 j + k at bit 8 k
    const unsigned na = a ^ K, nb = b ^ K, nc = c ^ K;
    const unsigned ab = a & b, axb = a ^ b, cd = c & d;
    // first missing call: 0 if a, else 1 if b, else 2 if c, else 3 if d, else 0
    const unsigned p0b0 = na & (b | (nc & d)), p0b1 = na & nb & (c | d);
    // the second missing call sits at 1 / 2 / 3
    const unsigned s1 = ab, s2 = axb & c, s3 = d & (axb ^ c) & ((ab & c) ^ K);
    const unsigned ge1 = a | b | c | d, ge2 = s1 | s2 | s3, nge2 = ge2 ^ K;
    const unsigned only_d = d & na & nb & nc;
    // second index: that call, or with fewer than two 3 (2 when the first is 3)
    const unsigned p1b0 = s1 | s3 | (nge2 & (only_d ^ K)), p1b1 = s2 | s3 | nge2;
    const unsigned nib = p0b0 | (p0b1 << 1) | (p1b0 << 2) | (p1b1 << 3);
    idx |= ((nib & 0xFu) | ((nib >> 4) & 0xF0u) | ((nib >> 8) & 0xF00u) | ((nib >> 12) & 0xF000u)) << (16 * j);
    // kept element 2 gq + e of group gq = 4 j + k -> bit 16 (k & 1) + 8 e + 2 j + (k >> 1)
    const unsigned k1 = (ge1 & 1u) | ((ge1 >> 8) & 1u) << 16 | ((ge1 >> 16) & 1u) << 1 | ((ge1 >> 24) & 1u) << 17;
    const unsigned k2 = (ge2 & 1u) | ((ge2 >> 8) & 1u) << 16 | ((ge2 >> 16) & 1u) << 1 | ((ge2 >> 24) & 1u) << 17;
    bits |= (k1 | (k2 << 8)) << (2 * j);
    surplus += pr_popc((ab & (c | d)) | (cd & (a | b))) + pr_popc(ab & cd); // three missing calls drop one, four drop two
  }
  *idx_out = idx;
  *bits_out = bits;
  return surplus;
}

// The record of chunk c = 2 p + h of K-tile kt of a row of n calls; word(k) is the .bed word of calls 16 k .. 16 k + 15 (anything
// where no call exists).  The K-tile's words are 8 kt + 0 .. 7.  Genotypes: steps 2 p and 2 p + 1, half h = words 4 p + h and
// 4 p + 2 + h; mask: the 32 individuals of step 2 p + h = words 4 p + 2 h and 4 p + 2 h + 1 -- three different words.  Over the
// four chunks every call is in the genotype words of exactly one record and in the mask words of exactly one: *tot and *miss
// add up to the row's sums.  Returns the dropped calls.
template <class Word>
PR_HD int pr_record(Word word, long kt, int c, long n, unsigned w[4], int *tot, int *miss) {
  const int p = c >> 1, h = c & 1;
  const long kb = 8 * kt + 4 * p;
  const long ka = kb + h, kc = kb + 2 + h, km = kb + 1 + h;
  const long ra = n - 16 * ka, rc = n - 16 * kc, rm = n - 16 * km;
  unsigned va, vc, vm, ma, mc, mm;
  pr_decode(ra > 0 ? word(ka) : 0u, (int)(ra < 16 ? ra : 16), &va, &ma);
  pr_decode(rc > 0 ? word(kc) : 0u, (int)(rc < 16 ? rc : 16), &vc, &mc);
  pr_decode(rm > 0 ? word(km) : 0u, (int)(rm < 16 ? rm : 16), &vm, &mm);
  const unsigned m0 = h ? mm : ma, m1 = h ? mc : mm;
  w[0] = pr_genoword(va);
  w[1] = pr_genoword(vc);
  *tot += pr_valsum(va) + pr_valsum(vc);
  *miss += pr_popc(m0 | (m1 << 1));
  return pr_maskword(m0, m1, &w[2], &w[3]);
}

#if defined(__HIPCC__)
// the .bed word of calls 16 k .. 16 k + 15 of a row of nbytes bytes; bytes behind the row read as 0
__device__ __forceinline__ unsigned pr_load(const unsigned char *bs, long k, long nbytes, bool aligned) {
  const long o = 4 * k;
  if (aligned && o + 4 <= nbytes) return *reinterpret_cast<const unsigned *>(bs + o);
  unsigned w = 0u;
#pragma unroll
  for (int b = 0; b < 4; ++b)
    if (o + b < nbytes) w |= (unsigned)bs[o + b] << (8 * b);
  return w;
}

// one wavefront per SNP row (four rows a workgroup: their records of a K-tile are 256 contiguous bytes), a lane per record
__global__ __launch_bounds__(256) void plink_records_kernel(PlinkRecordsArgs g) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= g.lpad) return;
  const long nk = g.ldk / I8_BK, items = nk * 4;
  uint4 *out = g.AM + ((row / S2_BM) * nk * S2_BM + (row % S2_BM)) * 4; // + ktile * S2_BM * 4 + chunk
  if (row >= g.l) { // a padding row
    for (long id = lane; id < items; id += 64) out[(id >> 2) * (S2_BM * 4) + (id & 3)] = make_uint4(0u, 0u, 0xCCCCCCCCu, 0u);
    if (lane == 0) g.row_surplus[row] = 0;
    return;
  }
  const unsigned char *bs = g.src + row * g.ld;
  const bool aligned = (reinterpret_cast<uintptr_t>(bs) & 3) == 0;
  const long nbytes = ((long)g.n + 3) / 4;
  int itot = 0, imiss = 0, isur = 0;
  unsigned anybits = 0;
  for (long id = lane; id < items; id += 64) {
    const long kt = id >> 2;
    const int c = (int)(id & 3);
    unsigned w[4];
    isur += pr_record([&](long k) { return pr_load(bs, k, nbytes, aligned); }, kt, c, (long)g.n, w, &itot, &imiss);
    anybits |= w[3];
    out[kt * (S2_BM * 4) + c] = make_uint4(w[0], w[1], w[2], w[3]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    itot += __shfl_xor(itot, o, 64);
    imiss += __shfl_xor(imiss, o, 64);
    isur += __shfl_xor(isur, o, 64);
  }
  if (lane == 0) {
    g.mean[row] = (double)itot / (double)(g.n - imiss); // x_total / (ni_test - n_miss): the integers of ingest_i8_kernel
    g.row_surplus[row] = isur;
  }
  // as sparse2_meta_kernel: every writer stores the same value, and only while the flag still reads 0
  if (g.anymiss && anybits != 0 && *reinterpret_cast<volatile int *>(g.anymiss) == 0) *reinterpret_cast<volatile int *>(g.anymiss) = 1;
}
#endif

} // namespace gemma_hip

// Host build of the word arithmetic of gemma_amd/csrc/plink_records.hip.h (2-bit PLINK rows -> the records of the records kernel)
// beside a call-by-call restatement of the two kernels it replaces: ingest_i8_kernel (code -> byte g | m << 4) followed by
// sparse2_meta_kernel (bytes -> records).  tests/test_plink_records_words.py loads it as a shared library; with
// -DPR_STANDALONE it is a program of its own (every byte pattern, ragged rows), meant for -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../gemma_amd/csrc/plink_records.hip.h"

using namespace gemma_hip;

namespace {
constexpr long BK = 128; // I8_BK: individuals of a K-tile

// ingest_i8_kernel: the packed bytes of one row, K padding 0
std::vector<uint8_t> packed_row(const uint8_t *bed, long n, long ldk, int *tot, int *miss) {
  std::vector<uint8_t> row((size_t)ldk, 0);
  *tot = *miss = 0;
  for (long i = 0; i < n; ++i) {
    const unsigned c = (bed[i >> 2] >> (2 * (i & 3))) & 3u;
    const unsigned byte = (0x00011002u >> (8 * c)) & 0xFFu; // 0 -> 2, 1 -> 16 (missing), 2 -> 1, 3 -> 0
    row[(size_t)i] = (uint8_t)byte;
    *tot += (int)(byte & 3u);
    *miss += (int)(byte >> 4);
  }
  return row;
}

// sparse2_meta_kernel: the record of chunk c of K-tile kt from the packed bytes
int ref_record(const uint8_t *row, long kt, int c, unsigned w[4]) {
  const int p = c >> 1, h = c & 1;
  const uint8_t *base = row + kt * BK;
  for (int e = 0; e < 2; ++e) {
    const uint8_t *src = base + 32 * (2 * p + e) + 16 * h;
    unsigned g2 = 0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) g2 |= (unsigned)(src[4 * i + j] & 3u) << (8 * j + 2 * i);
    w[e] = g2;
  }
  const uint8_t *src = base + 32 * (2 * p + h);
  unsigned idx = 0, bits = 0;
  int surplus = 0;
  for (int gq = 0; gq < 8; ++gq) {
    unsigned pat = 0;
    for (int q = 0; q < 4; ++q) pat |= (unsigned)((src[4 * gq + q] >> 4) & 1u) << q;
    const int cnt = __builtin_popcount(pat);
    const int p0 = cnt >= 1 ? __builtin_ffs((int)pat) - 1 : 0;
    const unsigned rest = pat & (pat - 1);
    const int p1 = cnt >= 2 ? __builtin_ffs((int)rest) - 1 : (p0 == 3 ? 2 : 3);
    idx |= (unsigned)(p0 | (p1 << 2)) << (4 * gq);
    const int e0 = 2 * gq, e1 = 2 * gq + 1;
    bits |= (unsigned)(cnt >= 1) << (8 * (e0 & 3) + (e0 >> 2));
    bits |= (unsigned)(cnt >= 2) << (8 * (e1 & 3) + (e1 >> 2));
    surplus += cnt > 2 ? cnt - 2 : 0;
  }
  w[2] = idx;
  w[3] = bits;
  return surplus;
}

// what plink_records_kernel does for one row, item by item; the .bed word is assembled from the row's own bytes only
int new_row(const uint8_t *bed, long n, long ldk, uint32_t *out, int *tot, int *miss) {
  const long nbytes = (n + 3) / 4, nk = ldk / BK;
  int sur = 0;
  *tot = *miss = 0;
  auto word = [&](long k) {
    unsigned w = 0;
    for (int b = 0; b < 4; ++b)
      if (4 * k + b < nbytes) w |= (unsigned)bed[4 * k + b] << (8 * b);
    return w;
  };
  for (long id = 0; id < nk * 4; ++id) {
    unsigned w[4];
    sur += pr_record(word, id >> 2, (int)(id & 3), n, w, tot, miss);
    for (int q = 0; q < 4; ++q) out[id * 4 + q] = w[q];
  }
  return sur;
}
} // namespace

// records of one row ([ktile][chunk][4 words]) by the new arithmetic / by the restated kernels; both return the dropped calls
extern "C" int pr_row_new(const uint8_t *bed, long n, long ldk, uint32_t *out, int *tot, int *miss) {
  return new_row(bed, n, ldk, out, tot, miss);
}
extern "C" int pr_row_ref(const uint8_t *bed, long n, long ldk, uint32_t *out, int *tot, int *miss) {
  const std::vector<uint8_t> row = packed_row(bed, n, ldk, tot, miss);
  int sur = 0;
  for (long id = 0; id < ldk / BK * 4; ++id) {
    unsigned w[4];
    sur += ref_record(row.data(), id >> 2, (int)(id & 3), w);
    for (int q = 0; q < 4; ++q) out[id * 4 + q] = w[q];
  }
  return sur;
}

#ifdef PR_STANDALONE
static int compare(const std::vector<uint8_t> &bed, long n, const char *what) {
  const long ldk = (n + BK - 1) / BK * BK + BK; // one all-padding K-tile behind the data
  std::vector<uint32_t> a((size_t)(ldk / BK * 16)), b(a.size());
  int ta, ma, tb, mb;
  const int sa = pr_row_new(bed.data(), n, ldk, a.data(), &ta, &ma), sb = pr_row_ref(bed.data(), n, ldk, b.data(), &tb, &mb);
  if (a != b || sa != sb || ta != tb || ma != mb) {
    std::printf("MISMATCH %s n=%ld: surplus %d/%d tot %d/%d miss %d/%d\n", what, n, sa, sb, ta, tb, ma, mb);
    return 1;
  }
  return 0;
}
int main() {
  int bad = 0;
  // every pattern of a group of four calls at every byte of a K-tile's first 32-individual step, beside a fixed neighbourhood
  for (int pos = 0; pos < 40; ++pos)
    for (int v = 0; v < 256; ++v) {
      std::vector<uint8_t> bed(40, 0x1B); // codes 3, 2, 1, 0 in every other byte
      bed[(size_t)pos] = (uint8_t)v;
      bad += compare(bed, 160, "byte pattern");
    }
  // ragged rows: every n up to three K-tiles, random codes, exactly (n + 3) / 4 bytes allocated
  std::srand(5);
  for (long n = 1; n <= 3 * BK + 5; ++n)
    for (int rep = 0; rep < 4; ++rep) {
      std::vector<uint8_t> bed((size_t)((n + 3) / 4));
      for (auto &x : bed) x = (uint8_t)(rep == 3 ? 0x55 : std::rand()); // rep 3: every call missing
      bad += compare(bed, n, "ragged");
    }
  std::printf(bad ? "plink_records: %d mismatches\n" : "plink_records: ok\n", bad);
  return bad ? 1 : 0;
}
#endif

// First-pass SNP QC statistics on device: what ReadFile_geno (GEMMA src/gemma_io.cpp:753-853) and
// ReadFile_bed (:942-1049) compute per SNP over the ANALYSED individuals before any kinship / LMM work:
// n_miss, maf = sum g / (2 (n - n_miss)), genotype class counts, polymorphism, and -- for the r2 filter --
// W^T x and x^T x with missing calls replaced by 2*maf.  One wavefront per SNP, two streaming passes.
// The threshold logic itself (order of filters, HWE exact test, r2 = x^T W (W^T W)^-1 W^T x / x^T x) is
// O(c^2) scalar work per SNP and runs on the host in snp_qc_finish().
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <vector>

#include "ingest.hip.h"
#define GEMMA_HIP_KERNEL_BODIES // a unit that includes this file instantiates what it launches: qc.h leaves out its extern templates
#include "qc.h"

namespace gemma_hip {

template <bool PLINK>
__global__ __launch_bounds__(256) void snp_qc_kernel(QcArgs g) {
  const int lane = threadIdx.x & 63;
  const long s = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (s >= g.l) return;
  const int n = g.n;
  const double *xs = reinterpret_cast<const double *>(g.src) + s * g.ld;
  const unsigned char *bs = reinterpret_cast<const unsigned char *>(g.src) + s * g.ld;
  double n_miss = 0.0, sum = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0, mn = INFINITY, mx = -INFINITY;
  for (int i = lane; i < n; i += 64) {
    const int p = g.idx_map ? g.idx_map[i] : i;
    double v;
    bool miss;
    if (PLINK) {
      v = plink_value((bs[p >> 2] >> (2 * (p & 3))) & 3u, miss);
    } else {
      v = xs[p];
      miss = isnan(v);
    }
    if (miss) {
      n_miss += 1.0;
    } else {
      sum += v;
      if (v >= 0 && v <= 0.5) n0 += 1.0;           // src/gemma_io.cpp:767-775
      if (v > 0.5 && v < 1.5) n1 += 1.0;
      if (v >= 1.5 && v <= 2.0) n2 += 1.0;
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    }
  }
  n_miss = wsum(n_miss); sum = wsum(sum); n0 = wsum(n0); n1 = wsum(n1); n2 = wsum(n2);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    mn = fmin(mn, __shfl_xor(mn, off, 64));
    mx = fmax(mx, __shfl_xor(mx, off, 64));
  }
  const double maf = sum / (2.0 * ((double)n - n_miss));
  const double fill = maf * 2.0; // :835, :1029
  double vx = 0.0;
  double *o = g.out + s * (QC_NSTAT + g.c);
  for (int a = 0; a < g.c; ++a) {
    double acc = 0.0;
    for (int i = lane; i < n; i += 64) {
      const int p = g.idx_map ? g.idx_map[i] : i;
      double v;
      bool miss;
      if (PLINK) {
        v = plink_value((bs[p >> 2] >> (2 * (p & 3))) & 3u, miss);
      } else {
        v = xs[p];
        miss = isnan(v);
      }
      v = miss ? fill : v;
      acc += g.Wt[(long)a * n + i] * v;
      if (a == 0) vx += v * v;
    }
    acc = wsum(acc);
    if (lane == 0) o[QC_NSTAT + a] = acc;
  }
  vx = wsum(vx);
  if (lane == 0) {
    o[0] = n_miss; o[1] = sum; o[2] = n0; o[3] = n1; o[4] = n2; o[5] = mn; o[6] = mx; o[7] = vx;
  }
}

} // namespace gemma_hip

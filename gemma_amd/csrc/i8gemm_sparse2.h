// What the host side of i8gemm_sparse2.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in i8gemm_sparse2.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>
#include "i8gemm_sparse.h"

namespace gemma_hip {

constexpr int S2_BM = 256, S2_BN = 128;
constexpr int S2_AMB = 16384;   // records of a K-tile: 256 rows x 4 chunks x 16 B
constexpr int S2_STAGE = 32768; // + digit tile 128 columns x 128 B
constexpr int S2_NST = 4;

struct Sparse2Args {
  const uint4 *AM;  // [tile_m][ktile][row % 256][chunk 2 p + h]: {g2(step 2p, h), g2(step 2p+1, h), idx(step 2p+h), kept bits}
  const int8_t *Bt; // digit d: N x ldk
  int *C;           // plane q: (2 lpad) x ldc; rows [0, lpad) = G products, [lpad, 2 lpad) = M products
  long ldk, ldc, strideB, strideC, m_row0;
  int tiles_m, tiles_n, nk, gm, fuse, digits;
  int plane0 = 0; // first plane of this launch (i8gemm_sparse2_r16.hip.h: the 7g6m form launches plane 0 and planes 1.. separately)
  const int2 *tile_map = nullptr; // (tile_m, tile_n) of workgroup blockIdx.x: the cross-XCD raster of s2_build_raster; nullptr:
                                  // the per-XCD ranges of round 3 (every XCD sweeps its own tile rows)
  // Blocks without a missing call (round 6): sparse2_meta_kernel leaves *anymiss = 0 for them and the mask product is identically
  // zero.  The launch site then queues BOTH forms of the 16-row kernel and each one returns at once unless the flag is its own
  // (run_if 1: only when *anymiss != 0, 2: only when *anymiss == 0, 0: always) -- the choice is made on the device, so the
  // asynchronous pipeline needs no read-back, and neither K loop changes.
  const int *anymiss = nullptr;
  int run_if = 0;
  // The epilogue instances of the 16-row kernel (i8gemm_sparse2_r16.hip.h, COMBINE) only: the launch is plane 0, planes
  // nplanes - 1 .. 1 are complete in C, and U^T x = qinv_j * sum_planes (G + mean_s * m_scale * M) goes to UtX (l x ldx, the
  // first n columns) instead of plane 0 to C.  Every other kernel ignores these.
  double *UtX = nullptr;
  long ldx = 0, l = 0, n = 0;
  const double *mean = nullptr, *qinv = nullptr;
  double m_scale = 1.0;
  int nplanes = 0;
  int epi_depth = 1; // GEMMA_HIP_I8_EPI_DEPTH: > 1 = the fused forms (nplanes 3, 4) read the planes back four steps ahead, 1 = one step
};

__global__ __launch_bounds__(256) void sparse2_meta_kernel(const int8_t *__restrict__ A, long lpad, long ldk,
                                                           uint4 *__restrict__ AM, int *__restrict__ row_surplus,
                                                           int *anymiss = nullptr /* set to 1 when the block holds a missing call */);

// Cross-XCD raster (round 4).  Workgroup b runs on XCD b % 8 and an XCD takes its workgroups in order, 32 at a time (one per
// CU: 128 KiB of LDS each).  Round 3 gave every XCD its own contiguous range of tiles -- eight disjoint sweeps: each record
// panel (2.56 MB per tile row) comes from HBM once per 4-column step of its XCD (39 times per plane) and each digit panel once per
// 8-row group (10 times), 71 GB per launch behind the L2s.  Here the eight XCDs work on ONE super-patch of rb x 8 tile rows by
// (8 / rb) x 4 tile columns at a time (XCD x: row block x % rb, column block x / rb; its 32 tiles rows inside, columns outside as
// before, so the per-XCD L2 patch is unchanged) and the super-patches sweep the columns of a band of rb x 8 tile rows before the
// next band starts: the band's record panels (rb x 20 MB at n = 20 000) stay in the 256 MiB Infinity Cache for the whole
// sweep and a digit panel is fetched from HBM once per band and shared by the rb XCDs that need it at the same time.  HBM reads
// per launch: records once per plane (1.2 GB), digits once per band (24 / rb GB) instead of 71 GB; what the L2s request is
// unchanged.  Ragged bands / column steps give the XCDs sequences of different lengths: tiles are moved from the tails of the
// long ones to the short ones until every XCD has exactly the number of workgroups the hardware will hand it.
static inline void s2_build_raster(int tiles_m, int tiles_n, int rb, std::vector<int2> &map, int PR = 8) {
  const int NX = 8, PC = 32 / PR; // PR x PC = the 32 tiles an XCD works on at a time (8 x 4 unless an experiment says otherwise)
  if (rb != 1 && rb != 2 && rb != 4 && rb != 8) rb = 2;
  const int cbs = NX / rb; // column blocks per super-patch
  std::vector<std::vector<int2>> seq(NX);
  for (int band0 = 0, band = 0; band0 < tiles_m; band0 += rb * PR, ++band)
    for (int col0 = 0; col0 < tiles_n; col0 += cbs * PC)
      for (int xx = 0; xx < NX; ++xx) {
        const int x = (xx + band) % NX; // the XCDs that get the short blocks of a ragged last column step change from band to band
        const int r0 = band0 + (xx % rb) * PR, c0 = col0 + (xx / rb) * PC;
        const int nr = std::min(PR, std::min(tiles_m, band0 + rb * PR) - r0), nc = std::min(PC, std::min(tiles_n, col0 + cbs * PC) - c0);
        if (nr <= 0 || nc <= 0) continue;
        for (int c = 0; c < nc; ++c)
          for (int r = 0; r < nr; ++r) seq[x].push_back(make_int2(r0 + r, c0 + c));
      }
  const int total = tiles_m * tiles_n;
  std::vector<int> want(NX);
  for (int x = 0; x < NX; ++x) want[x] = total / NX + (x < total % NX ? 1 : 0);
  std::vector<int2> spare;
  for (int x = 0; x < NX; ++x)
    while ((int)seq[x].size() > want[x]) {
      spare.push_back(seq[x].back());
      seq[x].pop_back();
    }
  for (int x = 0; x < NX; ++x)
    while ((int)seq[x].size() < want[x]) {
      seq[x].push_back(spare.back());
      spare.pop_back();
    }
  map.assign((size_t)total, make_int2(0, 0));
  for (int x = 0; x < NX; ++x)
    for (int o = 0; o < want[x]; ++o) map[(size_t)o * NX + x] = seq[x][o];
}

template <int NI>
__global__ __launch_bounds__(512, 2) void i8gemm_sparse2_kernel_t(Sparse2Args g);

// the shipped form: wavefronts 8 x 1 (54.4-55.0 ms against 56.5 for 4 x 2 in the same session, profiles/r03_i8_sparse_ablation.txt)
#ifndef S2_DEFAULT_RASTER
#define S2_DEFAULT_RASTER 1 // row blocks of the cross-XCD super-patch (0: the per-XCD ranges of round 3)
#endif
#ifndef S2_DEFAULT_NI
#define S2_DEFAULT_NI 1
#endif
static constexpr auto i8gemm_sparse2_kernel = i8gemm_sparse2_kernel_t<S2_DEFAULT_NI>;

// every instance of the kernel templates above that the library launches: declared here, instantiated by the kernel unit
#define I8GEMM_SPARSE2_INSTANCES(T) \
  T void i8gemm_sparse2_kernel_t<1>(Sparse2Args);
#ifndef GEMMA_HIP_KERNEL_BODIES
I8GEMM_SPARSE2_INSTANCES(extern template __global__)
#endif

} // namespace gemma_hip

// What the host side of plink_records.hip.h needs: the argument struct and the kernel's declaration.  The word arithmetic and the
// kernel body are in plink_records.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include "i8gemm_sparse2.h"

namespace gemma_hip {

struct PlinkRecordsArgs {
  const unsigned char *src; // l rows of ld bytes, four calls a byte
  long ld, l, lpad;         // lpad: a multiple of S2_BM; rows l .. lpad are written as padding
  int n;
  long ldk;                 // a multiple of I8_BK
  uint4 *AM;                // [tile_m][ktile][row % 256][chunk]
  int *row_surplus;         // lpad counters, each written here
  int *anymiss;             // nullptr, or the block's any-missing flag (zeroed by the caller)
  double *mean;             // l
};

// one wavefront per SNP row (four rows a workgroup), a lane per record
__global__ __launch_bounds__(256) void plink_records_kernel(PlinkRecordsArgs g);

} // namespace gemma_hip

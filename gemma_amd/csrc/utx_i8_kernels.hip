// The kernels of the exact int8-digit U^T x: digit planes and packing (i8gemm), the dense and 2:4-sparse products, the records
// kernels and the records straight from PLINK rows.  The host side (abi_utx.inc.h) sees only the .h of each pair.
#include "i8gemm.hip.h"
#include "i8gemm_sparse.hip.h"
#include "i8gemm_sparse2.hip.h"
#include "i8gemm_sparse2_r16.hip.h"
#include "plink_records.hip.h"
#include "i8gemm_dense16.hip.h"

namespace gemma_hip {
I8GEMM_INSTANCES(template __global__)
I8GEMM_SPARSE_INSTANCES(template __global__)
I8GEMM_SPARSE2_INSTANCES(template __global__)
I8GEMM_DENSE16_INSTANCES(template __global__)
} // namespace gemma_hip

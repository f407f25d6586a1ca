// The kernels of the first pass over the genotypes: ingest (and the small kinship / eigenvalue helpers beside it) and SNP QC.
// The exact-integer kinship (kin_i8.hip.h) is compiled in lmm_kernels.hip: see there.
#include "ingest.hip.h"
#include "qc.hip.h"

namespace gemma_hip {
INGEST_INSTANCES(template __global__)
QC_INSTANCES(template __global__)
} // namespace gemma_hip

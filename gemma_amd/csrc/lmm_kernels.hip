// The kernels of the per-SNP stage: -lm, the -lmm tests with their gene-expression and GXE forms and null fits, the fixed-lambda
// and Chebyshev tables, the score panel, the null fits of a panel and the Wald / LRT refinement of the score panel's hit pairs.
//
// The exact-integer kinship (kin_i8.hip.h) is compiled here too, although it belongs to the first pass: kin_i8_corr2_kernel and
// score_panel_kernel both call the HIP headers' 64-bit __shfl, the compiler specialises that shared function per code object, and
// on its own kin_i8_corr2_kernel comes out 32 bytes shorter with another schedule (profiles/kernel_identity_units.txt).  Kernels
// stay byte for byte what they were; the units are cut to that rule.
#include "lm_assoc.hip.h"
#include "lmm_assoc.hip.h"
#include "lmm_grid.hip.h"
#include "lmm_score_panel.hip.h"
#include "lmm_null_panel.hip.h"
#include "lmm_pair.hip.h"
#include "kin_i8.hip.h"

namespace gemma_hip {
LMM_ASSOC_INSTANCES(template __global__)
LMM_GRID_INSTANCES(template __global__)
LMM_SCORE_PANEL_INSTANCES(template __global__)
LMM_NULL_PANEL_INSTANCES(template __global__)
LMM_PAIR_INSTANCES(template __global__)
KIN_I8_INSTANCES(template __global__)
} // namespace gemma_hip

// What the host side of lm_assoc.hip.h needs: argument structs, constants, host helpers, kernel declarations.  The device
// functions and kernel bodies are in lm_assoc.hip.h, which includes this file.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "lmm_assoc.h"

namespace gemma_hip {

constexpr int LM_CMAX = 16;

struct LmArgs {
  const double *X; // l x ld, SNP-major, imputed
  long ld, l;
  const double *Wt;   // c x n
  const double *y;    // n
  const double *WtWi; // c x c
  const double *Wty;  // c
  double yPwy;
  int n, c, test_mode; // test_mode = a_mode - 50
  double lnbeta_half_df;
  SumStat *out;
};

__global__ __launch_bounds__(256) void lm_assoc_kernel(LmArgs g);

} // namespace gemma_hip

// Entry points of the windowed-correlation translation unit (cor_tu.hip = cor.hip.h + its own instance of the fp64 MFMA GEMM + the
// tile-pair list of the band).  Separate object file, as mqs_tu.h: C++ linkage, hidden behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>

namespace gemma_hip {

// indicator (ni_total ints, may be nullptr: all analysed), host
int cor_begin_x(long ni_total, const int *indicator, std::string &msg);
bool cor_active_x();
long cor_ni_total_x();
// geno, n_nb, var, cor on the host or (device == true) on the device; l_in >= l_out rows, the windows of the first l_out stay
// inside them (checked here: GEMMA_HIP_EINVAL)
int cor_block_x(int geno_kind, const void *geno, long l_in, long ld, long l_out, const int *n_nb, double *var, double *cor, bool device,
                hipStream_t s, std::string &msg);
void cor_release_x();
void cor_tu_shutdown();

} // namespace gemma_hip

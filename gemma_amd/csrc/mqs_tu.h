// Entry points of the MQS translation unit (mqs_tu.hip = mqs.hip.h + its own instance of the fp64 MFMA SYRK + the host finishing
// step of compAKtoS / JackknifeAKtoS).  Separate object file, as vc_tu.h / prdt_tu.h: C++ linkage, hidden behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>

namespace gemma_hip {

// indicator (ni_total ints, may be nullptr: all analysed), W (n x c, host).  slot 0 fills K (and A = K); slot 1 fills A beside a kept K.
int mqs_begin_x(long ni_total, const int *indicator, int n_vc, const double *W, int c, int slot, std::string &msg);
bool mqs_active_x();
long mqs_ni_total_x();
// cat / weight on the host or (device == true) on the device, like geno; weight may be nullptr
int mqs_add_x(int geno_kind, const void *geno, long l, long ld, const int *cat, const double *weight, bool device, hipStream_t s,
              std::string &msg);
int mqs_end_x(double *S, double *ns, std::string &msg);
int mqs_get_x(int slot, int i_vc, double *out, std::string &msg);
// S (2 n_vc x n_vc: S then Svar) from centred + scaled matrices on the device: matrix i at A + i n ld (A == K allowed)
int mqs_S_x(long n, int n_vc, const double *A, const double *K, long ld, int c, double *S, hipStream_t s, std::string &msg);
void mqs_release_x();
void mqs_tu_shutdown();

} // namespace gemma_hip

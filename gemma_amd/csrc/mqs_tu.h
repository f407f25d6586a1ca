// Entry points of the MQS translation unit (mqs_tu.hip = mqs.hip.h + its own instance of the fp64 MFMA SYRK + the host finishing
// step of compAKtoS / JackknifeAKtoS).  Separate object file, as vc_tu.h / prdt_tu.h: C++ linkage, hidden behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>

namespace gemma_hip {

// indicator (ni_total ints, may be nullptr: all analysed), W (n x c, host).  slot 0 fills K (and A = K); slot 1 fills A beside a kept K;
// slot 2 does the same with A starting from the kept (centred + scaled) K, as the reference's second CalcS leaves it.
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

// -ci 1 / -ci 2: the two genotype passes (ci.hip.h).  ci_pass_x: 0 none, 1 pass 1 open, 2 XWz finished and pass 2 open.
int ci_begin_x(long ni_total, const int *indicator, int n_vc, std::string &msg);
int ci_pass_x();
long ci_ni_total_x();
// cat / z / w on the host or (device == true) on the device, like geno; w may be nullptr (-ci 1); *n_skipped on the host
int ci_xwz_x(int geno_kind, const void *geno, long l, long ld, const int *cat, const double *z, const double *w, bool device,
             hipStream_t s, size_t *n_skipped, std::string &msg);
int ci_xwz_end_x(double *Xz, double *XWz, std::string &msg);
// out (l x n_vc) on the host or (device == true) on the device
int ci_xtxwz_x(int geno_kind, const void *geno, long l, long ld, double *out, bool device, hipStream_t s, std::string &msg);
void ci_release_x();

} // namespace gemma_hip

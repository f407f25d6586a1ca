// Entry points of the variance-component translation unit (vc_tu.hip = spd_inv.hip.h + vc.hip.h + its own instance of the fp64
// MFMA GEMM + the host solver).  Separate object file, as the eigensolver's (eigh_tu.h): C++ linkage, hidden behind the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <string>
#include <vector>

namespace gemma_hip {

struct VcResult {
  double sigma2[9], se_sigma2[9], pve[8], se_pve[8], pve_total, se_pve_total;
  int iterations, status;
  long evaluations, inverses;
  double t_asm, t_inv, t_pcor, t_mv, t_tr; // seconds summed over the evaluations (HIP events)
};

// SPD inverse in place with log det (spd_inv.hip.h); A on the device, any lda >= n.  7 = ENOTPD with *bad_pivot.
int spd_inverse_x(double *A, long n, long lda, double *logdet, long *bad_pivot, hipStream_t s, std::string &msg);
// K[l] (n x n, ldk): host pointers (copied) or device pointers (kept, not owned); W (n x c) and y (n) on the host
int vc_setup_x(long n, int n_vc, const double *const *K, long ldk, bool device, const double *W, int c, const double *y,
               std::string &msg);
int vc_he_x(VcResult &r, std::string &msg);
// iters: sigma2 per iteration (row 0 = the HE start), appended
int vc_reml_x(bool noconstrain, VcResult &r, std::vector<double> *iters, std::string &msg);
void vc_release_x();
void vc_tu_shutdown();

} // namespace gemma_hip

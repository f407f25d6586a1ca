// TEST INFRASTRUCTURE: runs the pair body of gemma_amd/csrc/mvlmm_pair.hip.h (mv_pair_fit + mv_pair_finish) and mv_null_fit with its
// variance epilogue (MvNullSe) on one CPU "lane", so that the new outputs can be compared with the oracle's primitives where no GPU
// exists.  Not part of the shipped library.
#include <cstddef>
#include <cstring>
#include <vector>
#define MV_HD inline
#define MV_OUTLINE
#include "../../gemma_amd/csrc/mvlmm_pair.hip.h"
using namespace gemma_hip;

struct HostLanes {
  static constexpr int N = 1;
  static int lane() { return 0; }
  static double sum(double v) { return v; }
};

template <int C> static void run_pairs(const MvPairArgs &p, MvPairFit *fit, double *B, double *VB) {
  static double scratch[MvNrScratch<2, C>::DOUBLES];
  for (long q = 0; q < p.m; ++q) {
    mv_pair_fit<C, HostLanes>(p, q, scratch);
    mv_pair_finish(p, q, fit, B, VB);
  }
}

// every pair of p (p->Yp gathered by the caller, p->raw: m x mv_pair_raw_doubles(c)); 1: no instance for p->c
extern "C" int mvp_pairs(const MvPairArgs *p, MvPairFit *fit, double *B, double *VB) {
#define CASE(CC) if (p->c == CC) { run_pairs<CC>(*p, fit, B, VB); return 0; }
  CASE(1) CASE(2) CASE(3) CASE(4) CASE(5) CASE(6)
#undef CASE
  return 1;
}

// the null fit of the run-time instance with the epilogue: se holds 2 x mvp_null_se_doubles(d, c)
extern "C" int mvp_null_se_rt(const MvNullArgs *a, double *se_out) {
  std::vector<double> scratch((size_t)MvNrLayout(a->g.d, a->g.c).DOUBLES);
  MvNullSe se;
  se.p = se_out;
  mv_null_fit<0, 0, HostLanes>(*a, scratch.data(), se);
  return 0;
}
// the same fit without it: the defaulted argument leaves `out` as it was
extern "C" int mvp_null_rt(const MvNullArgs *a) {
  std::vector<double> scratch((size_t)MvNrLayout(a->g.d, a->g.c).DOUBLES);
  mv_null_fit<0, 0, HostLanes>(*a, scratch.data());
  return 0;
}
extern "C" int mvp_null_se_doubles(int d, int c) { return mv_null_se_doubles(d, c); }
extern "C" int mvp_raw_doubles(int c) { return mv_pair_raw_doubles(c); }
extern "C" size_t mvp_pair_args_size(void) { return sizeof(MvPairArgs); }
extern "C" size_t mvp_pair_fit_size(void) { return sizeof(MvPairFit); }
extern "C" size_t mvp_null_args_size(void) { return sizeof(MvNullArgs); }

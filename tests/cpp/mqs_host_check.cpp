// The host side of -vc 1 -beta through include/gemma_io_host.hpp, without the device: ReadFile_cat, ReadFile_snps_header,
// ObtainWeight, UpdateSNP, ReadFile_beta, Calcq and CalcVCss, with S and the SNP counts read from files (the reference's, in
// tests/test_mqs_cpu.py).  Nothing here calls the C ABI, so the program links without the library (and runs under a sanitizer).
//
//   mqs_host_check <bim> <analysed snps, one per line> <cat file | -> <beta file> <S.txt> <size.txt> <n_block> <out prefix>
//
// prints q, Vq, size and the estimates with 17 significant digits; writes <out prefix>.S.txt / .Vq.txt / .q.txt / .size.txt.
#include <cstdio>
#include <fstream>
#include <sstream>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

static void print_vec(const char *name, const std::vector<double> &v) {
  printf("%s", name);
  for (size_t i = 0; i < v.size(); ++i) printf(" %.17g", v[i]);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: mqs_host_check bim snps cat beta S size n_block out\n");
    return 2;
  }
  std::vector<SNPINFO> snpInfo;
  if (!ReadFile_bim(argv[1], snpInfo)) return 1;
  std::set<std::string> analysed;
  if (!ReadFile_snps(argv[2], analysed)) return 1;
  std::vector<int> indicator_snp(snpInfo.size(), 0);
  for (size_t t = 0; t < snpInfo.size(); ++t) indicator_snp[t] = analysed.count(snpInfo[t].rs_number) ? 1 : 0;
  std::map<std::string, size_t> mapRS2cat;
  size_t n_vc = 1;
  if (std::string(argv[3]) != "-" && !ReadFile_cat(argv[3], mapRS2cat, n_vc)) return 1;
  // src/gemma.cpp:2110-2116
  std::set<std::string> setSnps_beta;
  if (!ReadFile_snps_header(argv[4], setSnps_beta)) return 1;
  std::map<std::string, double> mapRS2wK;
  ObtainWeight(snpInfo, indicator_snp, setSnps_beta, mapRS2cat, mapRS2wK);
  UpdateSNP(snpInfo, indicator_snp, mapRS2wK);
  std::vector<size_t> vec_cat, vec_ni;
  std::vector<double> vec_weight, vec_z2;
  size_t ni_study = 0, ns_study = 0, ns_test = 0;
  ReadFile_beta(argv[4], mapRS2cat, mapRS2wK, vec_cat, vec_ni, vec_weight, vec_z2, ni_study, ns_study, ns_test);
  std::vector<double> S(2 * n_vc * n_vc), Vq(n_vc * n_vc), q(n_vc), s(n_vc + 1);
  {
    std::ifstream f(argv[5]);
    for (double &v : S)
      if (!(f >> v)) return 1;
    std::ifstream g(argv[6]);
    std::vector<double> size(n_vc + 1);
    for (double &v : size)
      if (!(g >> v)) return 1;
    Matrix Vm = matrix_view(Vq.data(), n_vc, n_vc);
    Vector qv = vector_view(q.data(), n_vc), sv = vector_view(s.data(), n_vc);
    Calcq((size_t)atol(argv[7]), vec_cat, vec_ni, vec_weight, vec_z2, &Vm, &qv, &sv);
    print_vec("s_calcq", std::vector<double>(s.begin(), s.begin() + n_vc));
    s = size; // CalcS overwrites s with the SNP counts of the kinship pass (src/gemma.cpp:2166), then s[n_vc] = ni_test (:2215)
  }
  Matrix Sm = matrix_view(S.data(), n_vc, n_vc), Sv = matrix_view(S.data() + n_vc * n_vc, n_vc, n_vc), Vm = matrix_view(Vq.data(), n_vc, n_vc);
  Vector qv = vector_view(q.data(), n_vc), sv = vector_view(s.data(), n_vc);
  std::vector<double> pve, se_pve, sigma2, se_sigma2, enrich, se_enrich;
  double pve_total = 0, se_pve_total = 0;
  CalcVCss(&Vm, &Sm, &Sv, &qv, &sv, (double)ni_study, pve, se_pve, pve_total, se_pve_total, sigma2, se_sigma2, enrich, se_enrich);
  printf("n_vc %zu ni_study %zu ns_study %zu ns_test %zu\n", n_vc, ni_study, ns_study, ns_test);
  print_vec("q", q);
  print_vec("Vq", Vq);
  print_vec("size", s);
  print_vec("pve estimates", pve);
  print_vec("se(pve)", se_pve);
  print_vec("total pve", std::vector<double>(1, pve_total));
  print_vec("se(total pve)", std::vector<double>(1, se_pve_total));
  print_vec("sigma2 estimates", sigma2);
  print_vec("se(sigma2)", se_sigma2);
  print_vec("enrichment", enrich);
  print_vec("se(enrichment)", se_enrich);
  Matrix Sfull = matrix_view(S.data(), 2 * n_vc, n_vc);
  Vector size_v = vector_view(s.data(), n_vc + 1);
  return WriteMQS(argv[8], &Sfull, &Vm, &qv, &size_v) ? 0 : 1;
}

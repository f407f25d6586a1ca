// The host side of -ci 1 / -ci 2 and of the second round of -vc 2 -beta through include/gemma_io_host.hpp, without the device:
// ReadFile_wsnp (-wcat), ObtainWeight, UpdateWeight, ReadFile_beta (signed z), UpdateSNPnZ, ReadFile_ref and CalcCIss with the
// matrices of the two genotype passes read from files; ReadFile_beta, Calcq and CalcVCss of both -vc 2 rounds with S read from
// files (tests/test_ci_cpu.py).  Nothing here calls the C ABI, so the program links without the library.
//
//   ci_host_check ci  <bim> <snps> <cat> <wcat | -> <beta> <ref prefix> <1 | 2> <ni_test> <Xz> <XWz> <XtXWz> <pve> ...
//   ci_host_check wz  ... the same up to <ni_test> <pve> ...: prints w, z and vec_cat only (what the passes take)
//   ci_host_check study <study prefix> <ref prefix>: -study -ref without genotypes (CalcVCssStudy)
//   ci_host_check vc2 <bim> <snps> <cat> <wcat> <beta> <S.txt round 1> <S.txt round 2> <size.txt> <n_block>
//
// prints vectors with 17 significant digits.
#include <cstdio>
#include <fstream>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

static void print_vec(const char *name, const std::vector<double> &v) {
  printf("%s", name);
  for (size_t i = 0; i < v.size(); ++i) printf(" %.17g", v[i]);
  printf("\n");
}

static void print_est(const VCEST &e) {
  print_vec("pve estimates", e.v_pve);
  print_vec("se(pve)", e.v_se_pve);
  print_vec("total pve", std::vector<double>(1, e.pve_total));
  print_vec("se(total pve)", std::vector<double>(1, e.se_pve_total));
  print_vec("sigma2", e.v_sigma2);
  print_vec("se(sigma2)", e.v_se_sigma2);
  print_vec("enrichment", e.v_enrich);
  print_vec("se(enrichment)", e.v_se_enrich);
}

static bool read_all(const char *path, std::vector<double> &v, size_t want) {
  std::ifstream f(path);
  v.clear();
  double d;
  while (f >> d) v.push_back(d);
  return v.size() == want;
}

int main(int argc, char **argv) {
  if (argc == 4 && std::string(argv[1]) == "study") { // src/gemma.cpp:2231-2330
    VCEST e;
    std::vector<double> size;
    if (!CalcVCssStudy(argv[2], argv[3], e, &size)) return 1;
    print_est(e);
    print_vec("size", size);
    return 0;
  }
  if (argc < 10) {
    fprintf(stderr, "usage: ci_host_check ci|wz|vc2 ...\n");
    return 2;
  }
  const std::string mode = argv[1];
  std::vector<SNPINFO> snpInfo;
  if (!ReadFile_bim(argv[2], snpInfo)) return 1;
  std::set<std::string> analysed;
  if (!ReadFile_snps(argv[3], analysed)) return 1;
  std::vector<int> indicator_snp(snpInfo.size(), 0);
  for (size_t t = 0; t < snpInfo.size(); ++t) indicator_snp[t] = analysed.count(snpInfo[t].rs_number) ? 1 : 0;
  std::map<std::string, size_t> mapRS2cat;
  size_t n_vc = 1;
  if (!ReadFile_cat(argv[4], mapRS2cat, n_vc)) return 1;
  std::map<std::string, std::vector<double>> mapRS2wcat;
  if (std::string(argv[5]) != "-" && !ReadFile_wsnp(argv[5], n_vc, mapRS2wcat)) return 1;
  const char *file_beta = argv[6];
  std::set<std::string> setSnps_beta;
  if (!ReadFile_snps_header(file_beta, setSnps_beta)) return 1;
  std::map<std::string, double> mapRS2wK, mapRS2wA;
  ObtainWeight(snpInfo, indicator_snp, setSnps_beta, mapRS2wcat, mapRS2cat, mapRS2wK);

  if (mode == "ci" || mode == "wz") { // src/gemma.cpp:2400-2554
    const int a = mode == "ci" ? 13 : 10; // first pve
    if (argc != a + (int)n_vc) return 2;
    std::vector<double> S, Svar, s_ref, v_pve;
    size_t ni_ref = 0;
    if (!ReadFile_ref(argv[7], S, Svar, s_ref, ni_ref) || s_ref.size() != n_vc) return 1;
    const bool ci2 = atoi(argv[8]) == 2;
    const size_t ni_test = (size_t)atol(argv[9]);
    for (size_t i = 0; i < n_vc; ++i) v_pve.push_back(atof(argv[a + i]));
    std::vector<double> sv(n_vc, 0.0);
    for (const auto &it : mapRS2wK) sv[mapRS2cat.at(it.first)]++;
    Vector s_vec = vector_view(sv.data(), n_vc);
    if (!ci2) {
      for (const auto &it : mapRS2wK) mapRS2wA[it.first] = 1;
    } else {
      UpdateWeight(0, mapRS2wK, ni_test, &s_vec, v_pve, mapRS2wcat, mapRS2cat, mapRS2wA);
    }
    std::map<std::string, std::string> mapRS2A1;
    std::map<std::string, double> mapRS2z;
    ReadFile_beta(file_beta, mapRS2wA, mapRS2A1, mapRS2z);
    std::vector<double> w, z;
    std::vector<size_t> vec_cat;
    UpdateSNPnZ(snpInfo, indicator_snp, mapRS2wA, mapRS2A1, mapRS2z, mapRS2cat, w, z, vec_cat);
    printf("n_vc %zu ni_ref %zu ns_test %zu\n", n_vc, ni_ref, w.size());
    print_vec("s_vec", sv);
    print_vec("w", w);
    print_vec("z", z);
    print_vec("vec_cat", std::vector<double>(vec_cat.begin(), vec_cat.end()));
    if (mode == "wz") return 0;
    std::vector<double> Xz, XWz, XtXWz;
    if (!read_all(argv[10], Xz, ni_test * n_vc) || !read_all(argv[11], XWz, ni_test * n_vc) || !read_all(argv[12], XtXWz, w.size() * n_vc))
      return 1;
    Matrix Xzm = matrix_view(Xz.data(), ni_test, n_vc), XWzm = matrix_view(XWz.data(), ni_test, n_vc),
           Xtm = matrix_view(XtXWz.data(), w.size(), n_vc), Sm = matrix_view(S.data(), n_vc, n_vc), Sv = matrix_view(Svar.data(), n_vc, n_vc);
    VCEST e;
    e.v_pve = v_pve;
    CalcCIss(&Xzm, &XWzm, &Xtm, &Sm, &Sv, w, z, &s_vec, vec_cat, v_pve, e.v_se_pve, e.pve_total, e.se_pve_total, e.v_sigma2,
             e.v_se_sigma2, e.v_enrich, e.v_se_enrich);
    print_est(e);
    return 0;
  }
  if (mode != "vc2" || argc != 11) return 2;
  // src/gemma.cpp:2110-2212 with S of either round read from files
  UpdateSNP(snpInfo, indicator_snp, mapRS2wK);
  std::vector<double> S1, S2, size;
  if (!read_all(argv[7], S1, 2 * n_vc * n_vc) || !read_all(argv[8], S2, 2 * n_vc * n_vc) || !read_all(argv[9], size, n_vc + 1)) return 1;
  const size_t n_block = (size_t)atol(argv[10]);
  std::vector<size_t> vec_cat, vec_ni;
  std::vector<double> vec_weight, vec_z2, Vq(n_vc * n_vc), q(n_vc), s(n_vc);
  size_t ni_study = 0, ns_study = 0, ns_test = 0;
  Matrix Vm = matrix_view(Vq.data(), n_vc, n_vc);
  Vector qv = vector_view(q.data(), n_vc), sv = vector_view(s.data(), n_vc), nsv = vector_view(size.data(), n_vc);
  VCEST e;
  for (int round = 0; round < 2; ++round) {
    ReadFile_beta(file_beta, mapRS2cat, round == 0 ? mapRS2wK : mapRS2wA, vec_cat, vec_ni, vec_weight, vec_z2, ni_study, ns_study, ns_test);
    Calcq(n_block, vec_cat, vec_ni, vec_weight, vec_z2, &Vm, &qv, &sv);
    std::vector<double> &S = round == 0 ? S1 : S2;
    Matrix Sm = matrix_view(S.data(), n_vc, n_vc), Sv = matrix_view(S.data() + n_vc * n_vc, n_vc, n_vc);
    CalcVCss(&Vm, &Sm, &Sv, &qv, &nsv, (double)ni_study, e.v_pve, e.v_se_pve, e.pve_total, e.se_pve_total, e.v_sigma2, e.v_se_sigma2,
             e.v_enrich, e.v_se_enrich);
    if (round == 0) UpdateWeight(1, mapRS2wK, ni_study, &nsv, e.v_pve, mapRS2wcat, mapRS2cat, mapRS2wA);
  }
  print_vec("q", q);
  print_vec("Vq", Vq);
  print_est(e);
  return 0;
}

// File driver of the kinship-only prediction for several phenotypes (a_mode 43 with n_ph > 1), the way src/gemma.cpp:1732-1897 runs:
//   prdt_mv_driver -g geno -p pheno -n a b c -k kinship [-c covariates] -predict 1 [-o prefix] [-outdir dir]
// reads the phenotype, covariate and kinship files with the host readers (include/gemma_io_host.hpp), calls the C++ mirror's
// PRDT::MvnormPrdt (include/gemma_host.hpp) and writes <dir>/<prefix>.prdt.txt through the mirror's writer.  The genotype file is
// named as on the reference's command line but not read: this mode takes nothing from it.
// Exit status: 0; 2 usage; 1 a file or check error (message on stdout / stderr).
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include "gemma_host.hpp"
#include "gemma_io_host.hpp"

using namespace gemma_amd;

int main(int argc, char **argv) {
  std::string file_geno, file_pheno, file_kin, file_cvt, file_out = "result", path_out = "./output";
  std::vector<size_t> p_column;
  int predict = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-n") {
      while (i + 1 < argc && argv[i + 1][0] != '-') p_column.push_back((size_t)atol(argv[++i]));
      continue;
    }
    if (i + 1 >= argc) return 2;
    const std::string v = argv[++i];
    if (a == "-g") file_geno = v;
    else if (a == "-p") file_pheno = v;
    else if (a == "-k") file_kin = v;
    else if (a == "-c") file_cvt = v;
    else if (a == "-predict") predict = atoi(v.c_str());
    else if (a == "-o") file_out = v;
    else if (a == "-outdir") path_out = v;
    else return 2;
  }
  if (file_pheno.empty() || file_kin.empty() || predict != 1 || p_column.size() < 2) {
    std::cerr << "usage: prdt_mv_driver -g geno -p pheno -n a b [c ...] -k kinship [-c covariates] -predict 1 [-o prefix] [-outdir dir]"
              << std::endl;
    return 2;
  }
  try {
    CvtPhen cp;
    if (!ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, p_column)) return 1;
    if (!file_cvt.empty() && !ReadFile_cvt(file_cvt, cp.indicator_cvt, cp.cvt, cp.n_cvt)) return 1;
    if (!cp.indicator_cvt.empty() && cp.indicator_cvt.size() != cp.indicator_pheno.size()) {
      std::cout << "error! number of rows in the covariates file do not match the number of individuals." << std::endl;
      return 1;
    }
    cp.ProcessCvtPhen();
    if (cp.error) return 1;
    // CopyCvtPhen(W_full, Y_full, 1), src/param.cpp:2146-2198: the individuals with covariates
    const size_t n_ph = p_column.size(), c = cp.n_cvt;
    std::vector<double> W, Y;
    for (size_t i = 0; i < cp.indicator_cvt.size(); ++i) {
      if (cp.indicator_cvt[i] == 0) continue;
      for (size_t j = 0; j < n_ph; ++j) Y.push_back(cp.pheno[i][j]);
      for (size_t j = 0; j < c; ++j) W.push_back(cp.cvt[i][j]);
    }
    const size_t ni = Y.size() / n_ph;
    std::vector<double> G(ni * ni);
    Matrix Gm = matrix_view(G.data(), ni, ni), Wm = matrix_view(W.data(), ni, c), Ym = matrix_view(Y.data(), ni, n_ph);
    bool error = false;
    ReadFile_kin(file_kin, cp.indicator_cvt, error, &Gm);
    if (error) {
      std::cout << "error! fail to read kinship/relatedness file. " << std::endl;
      return 1;
    }
    gemma_mvlmm_null fit;
    PRDT::MvnormPrdt(&Gm, cp.indicator_pheno, cp.indicator_cvt, &Wm, &Ym, &fit);
    for (int which = 0; which < 2; ++which) { // the two triangles the reference prints (:1832-1845)
      const double *V = which == 0 ? fit.Vg_remle : fit.Ve_remle;
      std::cout << "REMLE estimate for " << (which == 0 ? "Vg" : "Ve") << " in the null model: " << std::endl;
      for (size_t i = 0; i < n_ph; i++) {
        for (size_t j = 0; j <= i; j++) std::cout << (j ? "\t" : "") << V[i * n_ph + j];
        std::cout << std::endl;
      }
    }
    PRDT::WriteFiles(path_out + "/" + file_out + ".prdt.txt", cp.indicator_cvt, &Ym);
  } catch (const std::exception &e) {
    std::cerr << e.what() << std::endl;
    return 1;
  }
  return 0;
}

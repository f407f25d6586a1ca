// File-driven null fits of a phenotype panel: the null model of EVERY column of a phenotype file in one call (test harness for
// CalcLambdaNullPanel / LMM::CalcNullMulti of include/gemma_host.hpp over the readers of include/gemma_io_host.hpp; NOT a replacement
// of GEMMA's CLI):
//
//   null_panel_file_driver (-p pheno (T columns) | -bfile prefix) [-c cvt] (-k kin | -d eval -u U) [-o name] [-outdir dir]
//
// writes  dir/name.null.txt   one line per phenotype column, six significant digits:
//                             pheno l_mle_null logl_mle_H0 l_remle_null logl_remle_H0 pve se_pve vg ve beta_1 se_1 ... beta_c se_c
//                             -- what the reference's `-lmm 4 -n t` writes to its log for column t (src/gemma.cpp:3402-3427), and the
//                             null lambdas the panel scans (multi_file_driver.cpp, score_panel_file_driver.cpp) are handed
// Without -p the phenotype is column 6 of prefix.fam.  The genotypes are not read: the null model has none.  The analysed
// individuals are those with EVERY phenotype column and every covariate present, as the reference selects them for `-n a b c`
// (ProcessCvtPhen, src/param.cpp:2090-2160).  Follows score_panel_file_driver.cpp: kinship file (or -d / -u) -> U^T W, U^T Y -> the fits.
#include <cstdlib>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

// the number of columns of the first line of a phenotype file
static size_t count_columns(const std::string &path) {
  TextFile f(path);
  std::string line;
  if (!f.ok() || !f.getline(line)) return 0;
  const char *p = line.data(), *end = p + line.size(), *b, *e;
  size_t k = 0;
  while (detail::next_token(p, end, b, e)) ++k;
  return k;
}

int main(int argc, char **argv) {
  std::string file_pheno, file_bfile, file_cvt, file_kin, file_kd, file_ku, file_out = "result", path_out = "./output";
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const bool has = i + 1 < argc && argv[i + 1][0] != '-';
    if (a == "-p" && has) file_pheno = argv[++i];
    else if (a == "-bfile" && has) file_bfile = argv[++i];
    else if (a == "-c" && has) file_cvt = argv[++i];
    else if (a == "-k" && has) file_kin = argv[++i];
    else if (a == "-d" && has) file_kd = argv[++i];
    else if (a == "-u" && has) file_ku = argv[++i];
    else if (a == "-o" && has) file_out = argv[++i];
    else if (a == "-outdir" && has) path_out = argv[++i];
    else {
      std::cerr << "unknown or incomplete option " << a << std::endl;
      return 2;
    }
  }
  if ((file_kin.empty() && (file_kd.empty() || file_ku.empty())) || (file_pheno.empty() && file_bfile.empty())) {
    std::cerr << "need -k kin or -d eval -u U, and -p pheno or -bfile prefix" << std::endl;
    return 2;
  }
  try {
    enforce_hip(gemma_hip_init(0, 0), "init");
    CvtPhen cp;
    std::map<std::string, int> mapID2num;
    std::vector<size_t> cols;
    const size_t n_cols = file_pheno.empty() ? 1 : count_columns(file_pheno);
    if (n_cols == 0) {
      std::cout << "error! no phenotype column in " << file_pheno << std::endl;
      return 3;
    }
    for (size_t t = 0; t < n_cols; ++t) cols.push_back(t + 1);
    if (!file_cvt.empty() && !ReadFile_cvt(file_cvt, cp.indicator_cvt, cp.cvt, cp.n_cvt)) return 3;
    if (cp.indicator_cvt.empty()) cp.n_cvt = 1;
    if (!(file_pheno.empty() ? ReadFile_fam(file_bfile + ".fam", cp.indicator_pheno, cp.pheno, mapID2num, cols)
                             : ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)))
      return 3;
    cp.ProcessCvtPhen(); // an individual is analysed when EVERY phenotype column and every covariate is present
    if (cp.error) return 3;
    const size_t ni_total = cp.indicator_idv.size(), ni_test = cp.ni_test, n_cvt = cp.n_cvt, n_ph = cols.size();
    if (ni_test == 0) {
      std::cout << "no individual has all " << n_ph << " phenotypes (and covariates): nothing to analyse" << std::endl;
      return 3;
    }
    std::vector<double> Wb, Yb;
    cp.CopyCvtPhen(Wb, Yb);
    Matrix W = matrix_view(Wb.data(), ni_test, n_cvt);
    std::cout << "ni_total=" << ni_total << " ni_test=" << ni_test << " n_cvt=" << n_cvt << " n_ph=" << n_ph;
    // ---- eigen pairs: from -k (centre + decompose) or from -d / -u (score_panel_file_driver.cpp) ----------------------------------
    std::vector<double> Ub(ni_test * ni_test), evalb(ni_test);
    Matrix U = matrix_view(Ub.data(), ni_test, ni_test);
    Vector eval = vector_view(evalb.data(), ni_test);
    bool error = false;
    double trace_G = 0.0;
    if (!file_kin.empty()) {
      std::vector<double> Gb(ni_test * ni_test);
      Matrix G = matrix_view(Gb.data(), ni_test, ni_test);
      ReadFile_kin_threaded(file_kin, cp.indicator_idv, error, &G);
      if (error) return 5;
      CenterMatrix(&G);
      trace_G = EigenDecomp_Zeroed(&G, &U, &eval, 0);
    } else {
      ReadFile_eigenU_threaded(file_ku, error, &U);
      ReadFile_eigenD(file_kd, error, &eval);
      if (error) return 5;
      for (size_t i = 0; i < ni_test; ++i) { // src/gemma.cpp:2640-2647
        if (evalb[i] < 1e-10) evalb[i] = 0;
        trace_G += evalb[i];
      }
      trace_G /= (double)ni_test;
    }
    std::cout << " trace_G=" << std::setprecision(12) << trace_G;
    std::vector<double> UtWb(ni_test * n_cvt), UtYb(ni_test * n_ph);
    Matrix Y = matrix_view(Yb.data(), ni_test, n_ph), UtW = matrix_view(UtWb.data(), ni_test, n_cvt),
           UtY = matrix_view(UtYb.data(), ni_test, n_ph);
    CalcUtX(&U, &W, &UtW);
    CalcUtX(&U, &Y, &UtY);
    // ---- the null models of all columns (one call), with the covariate effects ------------------------------------------------------
    LMM cLmm;
    std::vector<double> betab(n_ph * n_cvt), seb(n_ph * n_cvt);
    Matrix Beta = matrix_view(betab.data(), n_ph, n_cvt), SeBeta = matrix_view(seb.data(), n_ph, n_cvt);
    const std::vector<NullModel> nulls = cLmm.CalcNullMulti(&eval, &UtW, &UtY, trace_G, &Beta, &SeBeta);
    const std::string stem = path_out + "/" + file_out;
    std::ofstream null_file((stem + ".null.txt").c_str());
    if (!null_file) {
      std::cout << "error writing file: " << stem << ".null.txt" << std::endl;
      return 6;
    }
    null_file << "pheno\tl_mle_null\tlogl_mle_H0\tl_remle_null\tlogl_remle_H0\tpve\tse_pve\tvg\tve";
    for (size_t a = 0; a < n_cvt; ++a) null_file << "\tbeta_" << a + 1 << "\tse_" << a + 1;
    null_file << "\n" << std::setprecision(6);
    for (size_t t = 0; t < n_ph; ++t) {
      const NullModel &f = nulls[t];
      null_file << cols[t] << "\t" << f.l_mle_null << "\t" << f.logl_mle_H0 << "\t" << f.l_remle_null << "\t" << f.logl_remle_H0 << "\t"
                << f.pve_null << "\t" << f.pve_se_null << "\t" << f.vg_remle_null << "\t" << f.ve_remle_null;
      for (size_t a = 0; a < n_cvt; ++a) null_file << "\t" << betab[t * n_cvt + a] << "\t" << seb[t * n_cvt + a];
      null_file << "\n";
    }
    std::cout << " fits=" << cLmm.l_mle_null_multi.size() << std::endl;
    gemma_hip_shutdown();
  } catch (const std::exception &e) {
    std::cerr << "null_panel_file_driver: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}

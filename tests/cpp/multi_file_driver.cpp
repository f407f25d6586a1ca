// File-driven univariate LMM scan of SEVERAL phenotype columns over one pass of the genotypes (test harness for
// LMM::AnalyzePlinkMulti / AnalyzeBimbamMulti of include/gemma_host.hpp + include/gemma_io_host.hpp; NOT a replacement of GEMMA's CLI):
//
//   multi_file_driver (-bfile prefix | -g geno[.gz] -p pheno [-a anno]) [-c cvt] -k kin -lmm [1|2|3|4|9] -nsep col [col ...]
//                     [-maf x] [-miss x] [-hwe x] [-r2 x] [-o name] [-outdir dir]
//
// writes dir/name.<col>.assoc.txt for every column, each the file `gemma_file_driver ... -n <col> -o name.<col>` writes when the
// column's individuals are the analysed ones.  The reference has no such mode (`-n a b c` is the multivariate LMM); what it shares
// with `-n a b c` is the selection: the analysed individuals are those with EVERY selected phenotype and every covariate present
// (ProcessCvtPhen, src/param.cpp:2090-2160) -- per-phenotype missingness is not supported, the scan runs on one set of individuals.
// Follows gemma_file_driver.cpp's -k / -lmm path: first pass (device QC) -> kinship file -> centre -> eigendecomposition -> U^T W,
// U^T Y -> one null model per column -> the scan -> one .assoc.txt per column.  One line of key=value pairs on stdout is the log.
#include <cstdlib>
#include <iostream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

int main(int argc, char **argv) {
  std::string file_geno, file_pheno, file_anno, file_bfile, file_cvt, file_kin, file_out = "result", path_out = "./output";
  std::vector<size_t> cols;
  int a_mode = 0;
  QcLevels qc;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const bool has = i + 1 < argc && argv[i + 1][0] != '-';
    if (a == "-g" && has) file_geno = argv[++i];
    else if (a == "-p" && has) file_pheno = argv[++i];
    else if (a == "-a" && has) file_anno = argv[++i];
    else if (a == "-bfile" && has) file_bfile = argv[++i];
    else if (a == "-c" && has) file_cvt = argv[++i];
    else if (a == "-k" && has) file_kin = argv[++i];
    else if (a == "-nsep" && has) {
      while (i + 1 < argc && argv[i + 1][0] != '-') cols.push_back(strtoul(argv[++i], nullptr, 10));
    }
    else if (a == "-o" && has) file_out = argv[++i];
    else if (a == "-outdir" && has) path_out = argv[++i];
    else if (a == "-lmm") a_mode = has ? atoi(argv[++i]) : 1;
    else if (a == "-maf" && has) qc.maf_level = atof(argv[++i]);
    else if (a == "-miss" && has) qc.miss_level = atof(argv[++i]);
    else if (a == "-hwe" && has) qc.hwe_level = atof(argv[++i]);
    else if (a == "-r2" && has) qc.r2_level = atof(argv[++i]);
    else {
      std::cerr << "unknown or incomplete option " << a << std::endl;
      return 2;
    }
  }
  if (!a_mode || cols.empty() || file_kin.empty() || (file_bfile.empty() && (file_geno.empty() || file_pheno.empty()))) {
    std::cerr << "need -lmm m, -nsep col [col ...], -k kin and -bfile or -g/-p" << std::endl;
    return 2;
  }
  if (cols.size() > (size_t)GEMMA_LMM_MULTI_MAX) {
    std::cerr << "-nsep takes at most " << GEMMA_LMM_MULTI_MAX << " columns" << std::endl;
    return 2;
  }
  try {
    enforce_hip(gemma_hip_init(0, 0), "init");
    CvtPhen cp;
    std::vector<SNPINFO> snpInfo;
    std::vector<int> indicator_snp;
    std::map<std::string, int> mapID2num;
    std::map<std::string, std::string> mapRS2chr;
    std::map<std::string, long int> mapRS2bp;
    std::map<std::string, double> mapRS2cM;
    const std::set<std::string> setSnps;
    if (!file_cvt.empty() && !ReadFile_cvt(file_cvt, cp.indicator_cvt, cp.cvt, cp.n_cvt)) return 3;
    if (cp.indicator_cvt.empty()) cp.n_cvt = 1;
    if (!file_bfile.empty()) {
      if (!ReadFile_bim(file_bfile + ".bim", snpInfo)) return 3;
      if (!(file_pheno.empty() ? ReadFile_fam(file_bfile + ".fam", cp.indicator_pheno, cp.pheno, mapID2num, cols)
                               : ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)))
        return 3;
    } else {
      if (!file_anno.empty() && !ReadFile_anno(file_anno, mapRS2chr, mapRS2bp, mapRS2cM)) return 3;
      if (!ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)) return 3;
    }
    cp.ProcessCvtPhen(); // an individual is analysed when EVERY selected phenotype and every covariate is present
    if (cp.error) return 3;
    const size_t ni_total = cp.indicator_idv.size(), ni_test = cp.ni_test, n_cvt = cp.n_cvt, n_ph = cols.size();
    if (ni_test == 0) {
      std::cout << "no individual has all " << n_ph << " phenotypes (and covariates): nothing to analyse" << std::endl;
      return 3;
    }
    std::vector<double> Wb, Yb;
    cp.CopyCvtPhen(Wb, Yb);
    Matrix W = matrix_view(Wb.data(), ni_test, n_cvt);
    size_t ns_test = 0;
    if (!file_bfile.empty()) {
      if (!ReadFile_bed(file_bfile + ".bed", setSnps, &W, cp.indicator_idv, indicator_snp, snpInfo, qc.maf_level, qc.miss_level,
                        qc.hwe_level, qc.r2_level, ns_test))
        return 3;
    } else {
      if (!ReadFile_geno(file_geno, setSnps, &W, cp.indicator_idv, indicator_snp, qc.maf_level, qc.miss_level, qc.hwe_level,
                         qc.r2_level, mapRS2chr, mapRS2bp, mapRS2cM, snpInfo, ns_test))
        return 3;
    }
    std::cout << "ni_total=" << ni_total << " ni_test=" << ni_test << " n_cvt=" << n_cvt << " n_ph=" << n_ph
              << " ns_total=" << indicator_snp.size() << " ns_test=" << ns_test;
    // ---- kinship file -> centre -> eigendecomposition (gemma_file_driver.cpp's -k path) ----------------------------------------
    std::vector<double> Ub(ni_test * ni_test), evalb(ni_test), Gb(ni_test * ni_test);
    Matrix U = matrix_view(Ub.data(), ni_test, ni_test), G = matrix_view(Gb.data(), ni_test, ni_test);
    Vector eval = vector_view(evalb.data(), ni_test);
    bool error = false;
    ReadFile_kin_threaded(file_kin, cp.indicator_idv, error, &G);
    if (error) return 5;
    CenterMatrix(&G);
    const double trace_G = EigenDecomp_Zeroed(&G, &U, &eval, 0);
    std::cout << " trace_G=" << std::setprecision(12) << trace_G;
    std::vector<double> UtWb(ni_test * n_cvt), UtYb(ni_test * n_ph);
    Matrix Y = matrix_view(Yb.data(), ni_test, n_ph), UtW = matrix_view(UtWb.data(), ni_test, n_cvt),
           UtY = matrix_view(UtYb.data(), ni_test, n_ph);
    CalcUtX(&U, &W, &UtW);
    CalcUtX(&U, &Y, &UtY);
    // ---- one null model per column (src/gemma.cpp:2711-2750), then the scan ------------------------------------------------------
    LMM cLmm;
    cLmm.a_mode = a_mode;
    cLmm.file_bfile = file_bfile;
    cLmm.file_geno = file_geno;
    cLmm.path_out = path_out;
    cLmm.ni_total = ni_total;
    cLmm.indicator_idv = cp.indicator_idv;
    cLmm.indicator_snp = indicator_snp;
    cLmm.snpInfo = std::move(snpInfo);
    std::vector<double> col(ni_test);
    std::vector<std::string> names;
    for (size_t t = 0; t < n_ph; ++t) {
      for (size_t i = 0; i < ni_test; ++i) col[i] = UtYb[i * n_ph + t];
      Vector Uty = vector_view(col.data(), ni_test);
      const NullModel nm = CalcLambdaNull(&eval, &UtW, &Uty, 1e-5, 1e5, 10, trace_G);
      cLmm.l_mle_null_multi.push_back(nm.l_mle_null);
      cLmm.logl_mle_H0_multi.push_back(nm.logl_mle_H0);
      names.push_back(file_out + "." + std::to_string(cols[t]));
      std::cout << " l_mle_null." << cols[t] << "=" << nm.l_mle_null << " pve." << cols[t] << "=" << nm.pve_null;
    }
    if (!file_bfile.empty()) cLmm.AnalyzePlinkMulti(&U, &eval, &UtW, &UtY);
    else AnalyzeBimbamMulti(cLmm, &U, &eval, &UtW, &UtY);
    cLmm.WriteFilesMulti(names);
    std::cout << " snps=" << (cLmm.sumStatMulti.empty() ? 0 : cLmm.sumStatMulti[0].size()) << std::endl;
    gemma_hip_shutdown();
  } catch (const std::exception &e) {
    std::cerr << "multi_file_driver: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}

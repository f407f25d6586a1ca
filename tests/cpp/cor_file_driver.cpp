// File-driven `-calccor` run, the way `gemma` is invoked (test harness for VARCOV of include/gemma_host.hpp +
// include/gemma_io_host.hpp; NOT a replacement of GEMMA's CLI):
//
//   cor_file_driver (-bfile prefix | -g geno[.gz] -p pheno -a anno) -calccor [-windowbp n] [-windowcm x] [-windowns n]
//                   [-maf x] [-miss x] [-hwe x] [-r2 x] [-o name] [-outdir dir]
//
// following PARAM::ReadFiles (src/param.cpp:115-300: first pass over the genotypes, device QC), PARAM::CheckParam's default window
// (src/param.cpp:629-630) and BatchRun's a_mode 71 (src/gemma.cpp:2046-2059): CalcNB, the blocks, WriteCov -> dir/name.cor.txt.
// One line of key=value pairs on stdout is the log.
#include <cstdlib>
#include <iostream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

int main(int argc, char **argv) {
  std::string file_geno, file_pheno, file_anno, file_bfile, file_out = "result", path_out = "./output";
  bool calccor = false;
  VARCOV cVarcov;
  QcLevels qc;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const bool has = i + 1 < argc && argv[i + 1][0] != '-';
    if (a == "-g" && has) file_geno = argv[++i];
    else if (a == "-p" && has) file_pheno = argv[++i];
    else if (a == "-a" && has) file_anno = argv[++i];
    else if (a == "-bfile" && has) file_bfile = argv[++i];
    else if (a == "-o" && has) file_out = argv[++i];
    else if (a == "-outdir" && has) path_out = argv[++i];
    else if (a == "-calccor") calccor = true;
    else if (a == "-windowbp" && has) cVarcov.window_bp = strtoul(argv[++i], nullptr, 10); // src/gemma.cpp:1576-1599
    else if (a == "-windowcm" && has) cVarcov.window_cm = atof(argv[++i]);
    else if (a == "-windowns" && has) cVarcov.window_ns = strtoul(argv[++i], nullptr, 10);
    else if (a == "-maf" && has) qc.maf_level = atof(argv[++i]);
    else if (a == "-miss" && has) qc.miss_level = atof(argv[++i]);
    else if (a == "-hwe" && has) qc.hwe_level = atof(argv[++i]);
    else if (a == "-r2" && has) qc.r2_level = atof(argv[++i]);
    else {
      std::cerr << "unknown or incomplete option " << a << std::endl;
      return 2;
    }
  }
  if (!calccor || (file_bfile.empty() && (file_geno.empty() || file_pheno.empty()))) {
    std::cerr << "need -calccor and -bfile or -g/-p[/-a]" << std::endl;
    return 2;
  }
  if (cVarcov.window_cm == 0 && cVarcov.window_bp == 0 && cVarcov.window_ns == 0) cVarcov.window_bp = 1000000; // src/param.cpp:629-630
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
    const std::vector<size_t> cols(1, 1);
    cp.n_cvt = 1;
    if (!file_bfile.empty()) {
      if (!ReadFile_bim(file_bfile + ".bim", snpInfo)) return 3;
      if (!(file_pheno.empty() ? ReadFile_fam(file_bfile + ".fam", cp.indicator_pheno, cp.pheno, mapID2num, cols)
                               : ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)))
        return 3;
    } else {
      if (!file_anno.empty() && !ReadFile_anno(file_anno, mapRS2chr, mapRS2bp, mapRS2cM)) return 3;
      if (!ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)) return 3;
    }
    cp.ProcessCvtPhen();
    if (cp.error) return 3;
    std::vector<double> Wb, Yb;
    cp.CopyCvtPhen(Wb, Yb);
    Matrix W = matrix_view(Wb.data(), cp.ni_test, cp.n_cvt);
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
    // ---- a_mode 71, src/gemma.cpp:2046-2059: CopyFromParam, then AnalyzePlink or AnalyzeBimbam ---------------------------------
    cVarcov.file_out = file_out;
    cVarcov.path_out = path_out;
    cVarcov.file_geno = file_geno;
    cVarcov.file_bfile = file_bfile;
    cVarcov.indicator_idv = cp.indicator_idv;
    cVarcov.indicator_snp = indicator_snp;
    cVarcov.snpInfo = snpInfo;
    if (!file_bfile.empty()) cVarcov.AnalyzePlink();
    else cVarcov.AnalyzeBimbam();
    if (cVarcov.error) { // a genotype file that cannot be opened or ends early: no success line
      gemma_hip_shutdown();
      return 3;
    }
    std::cout << "ni_total=" << cp.indicator_idv.size() << " ni_test=" << cp.ni_test << " ns_total=" << indicator_snp.size()
              << " ns_test=" << ns_test << " out=" << path_out << "/" << file_out << ".cor.txt" << std::endl;
    gemma_hip_shutdown();
  } catch (const std::exception &e) {
    std::cerr << "cor_file_driver: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}

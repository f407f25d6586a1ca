// File-driven MQS runs, the way `gemma` is invoked (test harness for the MQS functions of include/gemma_io_host.hpp; NOT a
// replacement of GEMMA's CLI):
//
//   mqs_file_driver (-bfile prefix | -g geno[.gz] -p pheno [-a anno]) [-p pheno] [-c covariates] [-cat file] [-wcat file]
//                   [-beta file] [-o name] [-outdir dir] (-gs | -vc 1 | -vc 2 | -ref prefix -pve x ... -ci 1|2)
//
// -g runs -ci only: the mirror has no CalcS on a BIMBAM file.
//
// following PARAM::ReadFiles (src/param.cpp:115-300: first pass over the genotypes, device QC) and BatchRun's a_mode 25 (-gs,
// src/gemma.cpp:1960-2000), 61 / 62 with -beta (:2102-2230) and 66 / 67 (:2400-2554).  Writes dir/name.S.txt / .Vq.txt / .q.txt /
// .size.txt (WriteMQS) and the estimate lines of dir/name.log.txt in the reference's wording and six-digit format.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

static void log_vec(std::ostream &o, const char *name, const std::vector<double> &v) { // src/param.cpp / gemma.cpp WriteLog
  o << "## " << name << " = ";
  for (size_t i = 0; i < v.size(); i++) o << "  " << v[i];
  o << std::endl;
}

int main(int argc, char **argv) {
  std::string file_geno, file_anno, file_pheno, file_cvt, file_bfile, file_cat, file_wcat, file_beta, file_ref, file_out = "result", path_out = "./output";
  bool gs = false;
  int vc = 0, ci = 0;
  std::vector<double> v_pve;
  QcLevels qc;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    const bool has = i + 1 < argc && argv[i + 1][0] != '-';
    if (a == "-p" && has) file_pheno = argv[++i];
    else if (a == "-c" && has) file_cvt = argv[++i];
    else if (a == "-bfile" && has) file_bfile = argv[++i];
    else if (a == "-g" && has) file_geno = argv[++i];
    else if (a == "-a" && has) file_anno = argv[++i];
    else if (a == "-cat" && has) file_cat = argv[++i];
    else if (a == "-wcat" && has) file_wcat = argv[++i];
    else if (a == "-beta" && has) file_beta = argv[++i];
    else if (a == "-ref" && has) file_ref = argv[++i];
    else if (a == "-o" && has) file_out = argv[++i];
    else if (a == "-outdir" && has) path_out = argv[++i];
    else if (a == "-gs") gs = true;
    else if (a == "-vc" && has) vc = atoi(argv[++i]);
    else if (a == "-ci" && has) ci = atoi(argv[++i]);
    else if (a == "-pve") {
      while (i + 1 < argc && (argv[i + 1][0] != '-' || (argv[i + 1][1] >= '0' && argv[i + 1][1] <= '9') || argv[i + 1][1] == '.'))
        v_pve.push_back(atof(argv[++i]));
    } else {
      std::cerr << "unknown or incomplete option " << a << std::endl;
      return 2;
    }
  }
  const int modes = (gs ? 1 : 0) + (vc != 0 ? 1 : 0) + (ci != 0 ? 1 : 0);
  if ((file_bfile.empty() && (file_geno.empty() || file_pheno.empty() || ci == 0)) || modes != 1 || (vc != 0 && (file_beta.empty() || vc < 1 || vc > 2)) ||
      (ci != 0 && (file_beta.empty() || file_ref.empty() || v_pve.empty() || ci < 1 || ci > 2)) || (vc == 2 && file_wcat.empty()) ||
      (ci == 2 && file_wcat.empty())) {
    std::cerr << "need -bfile (or -g -p with -ci) and one of -gs, -vc 1|2 -beta, -ref -pve -ci 1|2 -beta (-wcat for -vc 2 and -ci 2)" << std::endl;
    return 2;
  }
  try {
    enforce_hip(gemma_hip_init(0, 0), "init");
    CvtPhen cp;
    std::vector<SNPINFO> snpInfo;
    std::vector<int> indicator_snp;
    std::map<std::string, int> mapID2num;
    const std::set<std::string> setSnps;
    const std::vector<size_t> cols(1, 1);
    std::map<std::string, std::string> mapRS2chr;
    std::map<std::string, long int> mapRS2bp;
    std::map<std::string, double> mapRS2cM;
    if (!file_bfile.empty()) {
      if (!ReadFile_bim(file_bfile + ".bim", snpInfo)) return 3;
      if (!(file_pheno.empty() ? ReadFile_fam(file_bfile + ".fam", cp.indicator_pheno, cp.pheno, mapID2num, cols)
                               : ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)))
        return 3;
    } else {
      if (!file_anno.empty() && !ReadFile_anno(file_anno, mapRS2chr, mapRS2bp, mapRS2cM)) return 3;
      if (!ReadFile_pheno(file_pheno, cp.indicator_pheno, cp.pheno, cols)) return 3;
    }
    if (!file_cvt.empty() && !ReadFile_cvt(file_cvt, cp.indicator_cvt, cp.cvt, cp.n_cvt)) return 3;
    if (cp.indicator_cvt.empty()) cp.n_cvt = 1;
    cp.ProcessCvtPhen();
    if (cp.error) return 3;
    std::vector<double> Wb, Yb;
    cp.CopyCvtPhen(Wb, Yb);
    const size_t ni_test = cp.ni_test;
    Matrix W = matrix_view(Wb.data(), ni_test, cp.n_cvt);
    size_t ns_test = 0;
    if (!file_bfile.empty()) {
      if (!ReadFile_bed(file_bfile + ".bed", setSnps, &W, cp.indicator_idv, indicator_snp, snpInfo, qc.maf_level, qc.miss_level,
                        qc.hwe_level, qc.r2_level, ns_test))
        return 3;
    } else {
      if (!ReadFile_geno(file_geno, setSnps, &W, cp.indicator_idv, indicator_snp, qc.maf_level, qc.miss_level, qc.hwe_level, qc.r2_level,
                         mapRS2chr, mapRS2bp, mapRS2cM, snpInfo, ns_test))
        return 3;
    }
    std::map<std::string, size_t> mapRS2cat;
    size_t n_vc = 1;
    if (!file_cat.empty() && !ReadFile_cat(file_cat, mapRS2cat, n_vc)) return 3;
    std::map<std::string, std::vector<double>> mapRS2wcat;
    if (!file_wcat.empty() && !ReadFile_wsnp(file_wcat, n_vc, mapRS2wcat)) return 3;
    const std::string prefix = path_out + "/" + file_out, file_bed = file_bfile + ".bed";
    std::ofstream log((prefix + ".log.txt").c_str());
    if (!log) {
      std::cerr << "cannot write " << prefix << ".log.txt" << std::endl;
      return 4;
    }
    log << "## number of total individuals in the sample = " << cp.indicator_idv.size() << std::endl;
    VCEST est;
    std::vector<double> Sb(2 * n_vc * n_vc, 0.0), Vqb(n_vc * n_vc, 0.0), qb(n_vc, 0.0), sb(n_vc + 1, 0.0);
    Matrix S = matrix_view(Sb.data(), 2 * n_vc, n_vc), Vq = matrix_view(Vqb.data(), n_vc, n_vc);
    Vector q = vector_view(qb.data(), n_vc), s = vector_view(sb.data(), n_vc + 1);
    if (gs) { // a_mode 25
      const std::set<std::string> none;
      std::map<std::string, double> mapRS2wK;
      ObtainWeight(snpInfo, indicator_snp, none, mapRS2wcat, mapRS2cat, mapRS2wK);
      Vector s_vec = vector_view(sb.data(), n_vc);
      if (!CalcS(file_bed, cp.indicator_idv, indicator_snp, mapRS2wK, mapRS2cat, snpInfo, &W, n_vc, &S, &s_vec, 0)) return 3;
      sb[n_vc] = (double)ni_test;
      if (!WriteMQS(prefix, &S, nullptr, nullptr, &s)) return 4;
    } else if (vc != 0) { // a_mode 61 / 62 with -beta
      size_t ni_study = 0, ns_study = 0, ns_beta = 0;
      if (!CalcVCssBeta(file_bed, file_beta, cp.indicator_idv, indicator_snp, snpInfo, mapRS2cat, mapRS2wcat, &W, n_vc, 200, vc == 2, &S, &Vq,
                        &q, &s, ni_study, ns_study, ns_beta, est))
        return 3;
      if (!WriteMQS(prefix, &S, &Vq, &q, &s)) return 4;
      log << "## number of total individuals in the study = " << ni_study << std::endl;
      log << "## number of variance components = " << n_vc << std::endl;
      log_vec(log, "pve estimates", est.v_pve);
      log_vec(log, "se(pve)", est.v_se_pve);
      log << "## total pve = " << est.pve_total << std::endl << "## se(total pve) = " << est.se_pve_total << std::endl;
      log_vec(log, "sigma2 estimates", est.v_sigma2);
      log_vec(log, "se(sigma2)", est.v_se_sigma2);
      log_vec(log, "enrichment", est.v_enrich);
      log_vec(log, "se(enrichment)", est.v_se_enrich);
    } else { // a_mode 66 / 67
      if (v_pve.size() != n_vc) {
        std::cerr << "-pve takes one value per category" << std::endl;
        return 2;
      }
      std::vector<double> Sr, Svr, s_ref;
      size_t ni_ref = 0;
      if (!ReadFile_ref(file_ref, Sr, Svr, s_ref, ni_ref) || s_ref.size() != n_vc) return 3;
      std::set<std::string> setSnps_beta;
      if (!ReadFile_snps_header(file_beta, setSnps_beta)) return 3;
      std::map<std::string, double> mapRS2wK, mapRS2wA, mapRS2z;
      std::map<std::string, std::string> mapRS2A1;
      ObtainWeight(snpInfo, indicator_snp, setSnps_beta, mapRS2wcat, mapRS2cat, mapRS2wK);
      std::vector<double> svb(n_vc, 0.0);
      for (const auto &it : mapRS2wK) svb[mapRS2cat.size() == 0 ? 0 : mapRS2cat.at(it.first)]++;
      Vector s_vec = vector_view(svb.data(), n_vc);
      if (ci == 1) {
        for (const auto &it : mapRS2wK) mapRS2wA[it.first] = 1;
      } else {
        UpdateWeight(0, mapRS2wK, ni_test, &s_vec, v_pve, mapRS2wcat, mapRS2cat, mapRS2wA);
      }
      ReadFile_beta(file_beta, mapRS2wA, mapRS2A1, mapRS2z);
      std::vector<double> w, z;
      std::vector<size_t> vec_cat;
      UpdateSNPnZ(snpInfo, indicator_snp, mapRS2wA, mapRS2A1, mapRS2z, mapRS2cat, w, z, vec_cat);
      std::vector<double> Xzb(ni_test * n_vc), XWzb(ni_test * n_vc), Xtb(w.size() * n_vc);
      Matrix Xz = matrix_view(Xzb.data(), ni_test, n_vc), XWz = matrix_view(XWzb.data(), ni_test, n_vc), XtXWz = matrix_view(Xtb.data(), w.size(), n_vc);
      size_t n_skipped = 0;
      if (!file_bfile.empty()) {
        if (!PlinkXwz(file_bed, cp.indicator_idv, indicator_snp, vec_cat, ci == 1 ? nullptr : &w, z, n_vc, &Xz, &XWz, &n_skipped)) return 3;
        if (!PlinkXtXwz(file_bed, cp.indicator_idv, indicator_snp, n_vc, &XtXWz)) return 3;
      } else {
        if (!BimbamXwz(file_geno, cp.indicator_idv, indicator_snp, vec_cat, ci == 1 ? nullptr : &w, z, n_vc, &Xz, &XWz, &n_skipped)) return 3;
        if (!BimbamXtXwz(file_geno, cp.indicator_idv, indicator_snp, n_vc, &XtXWz)) return 3;
      }
      enforce_hip(gemma_hip_ci_release(), "ci_release");
      Matrix Sm = matrix_view(Sr.data(), n_vc, n_vc), Svm = matrix_view(Svr.data(), n_vc, n_vc);
      est.v_pve = v_pve;
      CalcCIss(&Xz, &XWz, &XtXWz, &Sm, &Svm, w, z, &s_vec, vec_cat, v_pve, est.v_se_pve, est.pve_total, est.se_pve_total, est.v_sigma2,
               est.v_se_sigma2, est.v_enrich, est.v_se_enrich);
      log << "## number of total individuals in the reference = " << ni_ref << std::endl;
      log << "## number of analyzed SNPs/var = " << ns_test << std::endl; // of the first pass, as the reference prints it
      log << "## number of SNPs/var with a weight = " << w.size() << std::endl;
      log << "## number of skipped SNPs/var = " << n_skipped << std::endl;
      log << "## number of variance components = " << n_vc << std::endl;
      log_vec(log, "pve estimates", est.v_pve);
      log_vec(log, "se(pve)", est.v_se_pve);
      log << "## total pve = " << est.pve_total << std::endl << "## se(total pve) = " << est.se_pve_total << std::endl;
      log_vec(log, "sigma2 per snp", est.v_sigma2);
      log_vec(log, "se(sigma2 per snp)", est.v_se_sigma2);
      log_vec(log, "enrichment", est.v_enrich);
      log_vec(log, "se(enrichment)", est.v_se_enrich);
    }
    std::cout << "ni_total=" << cp.indicator_idv.size() << " ni_test=" << ni_test << " ns_total=" << indicator_snp.size() << " n_vc=" << n_vc
              << " out=" << prefix << std::endl;
    gemma_hip_shutdown();
  } catch (const std::exception &e) {
    std::cerr << "mqs_file_driver: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}

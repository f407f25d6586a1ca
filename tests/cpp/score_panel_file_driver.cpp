// File-driven score-test panel: `-lmm 3` of EVERY column of a phenotype file over one pass of the genotypes, written as the pairs
// with p_score <= -pmax and the best SNP of every phenotype (test harness for LMM::AnalyzePlinkScorePanelHits /
// AnalyzeFeedScorePanelHits of include/gemma_host.hpp over the readers of include/gemma_io_host.hpp; NOT a replacement of GEMMA's CLI):
//
//   score_panel_file_driver (-bfile prefix | -g geno[.gz] [-a anno]) -p pheno (T columns) [-c cvt] (-k kin | -d eval -u U)
//                           -lmm 3 -pmax x [-maf x] [-miss x] [-hwe x] [-r2 x] [-o name] [-outdir dir]
//
// writes  dir/name.hits.txt   chr rs ps n_miss allele1 allele0 af phenotype beta se p_score -- the SNP columns and the number formats
//                             of LMM::WriteFiles, phenotype the 1-based column; sorted by phenotype, then by the SNP order of the file
//         dir/name.best.txt   phenotype rs ps beta se p_score, one line per phenotype (NA / -9 / nan: no SNP with a statistic)
//         dir/name.log.txt    the null lambda of every phenotype and the number of hits
// The analysed individuals are those with EVERY phenotype column and every covariate present, as the reference selects them for
// `-n a b c` (ProcessCvtPhen, src/param.cpp:2090-2160); per-phenotype missingness is not supported.  Follows multi_file_driver.cpp:
// first pass (device QC) -> kinship file (or -d / -u) -> U^T W, U^T Y -> one null model per column -> the scan.
#include <cstdlib>
#include <iostream>
#include <map>
#include <set>
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

// the rows of the analysed SNPs of a BIMBAM file over the analysed individuals, one block ahead of the device (AnalyzeBimbamMulti)
static void AnalyzeBimbamScorePanelHits(LMM &lmm, const Matrix *U, const Vector *eval, const Matrix *UtW, const Matrix *UtY, double p_max) {
  const size_t ni_total = lmm.indicator_idv.size(), n = UtY->size1;
  BimbamReader rd(lmm.file_geno, ni_total);
  if (!rd.ok()) throw std::runtime_error("error reading genotype file");
  const size_t B = bimbam_block_rows(n, LMM_BATCH_SIZE);
  const std::vector<int> keep = lmm.analysed_snps();
  BlockPrefetch pf(B * n * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= keep.size()) return 0;
    return rd.read_block(B, static_cast<double *>(slot), n, nullptr, &keep, lmm.indicator_idv.data());
  });
  LMM::RowFeeder feed = [&](const double *&X) -> size_t {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) throw std::runtime_error("Problem reading geno file (not enough genotypes in line)");
    X = static_cast<const double *>(slot);
    return l;
  };
  lmm.AnalyzeFeedScorePanelHits(U, eval, UtW, UtY, feed, B, n, p_max);
}

int main(int argc, char **argv) {
  std::string file_geno, file_pheno, file_anno, file_bfile, file_cvt, file_kin, file_kd, file_ku, file_out = "result", path_out = "./output";
  int a_mode = 0;
  double p_max = -1.0;
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
    else if (a == "-d" && has) file_kd = argv[++i];
    else if (a == "-u" && has) file_ku = argv[++i];
    else if (a == "-o" && has) file_out = argv[++i];
    else if (a == "-outdir" && has) path_out = argv[++i];
    else if (a == "-lmm" && has) a_mode = atoi(argv[++i]);
    else if (a == "-pmax" && has) p_max = atof(argv[++i]);
    else if (a == "-maf" && has) qc.maf_level = atof(argv[++i]);
    else if (a == "-miss" && has) qc.miss_level = atof(argv[++i]);
    else if (a == "-hwe" && has) qc.hwe_level = atof(argv[++i]);
    else if (a == "-r2" && has) qc.r2_level = atof(argv[++i]);
    else {
      std::cerr << "unknown or incomplete option " << a << std::endl;
      return 2;
    }
  }
  if (a_mode != 3 || !(p_max >= 0.0 && p_max <= 1.0) || (file_kin.empty() && (file_kd.empty() || file_ku.empty())) ||
      (file_bfile.empty() && (file_geno.empty() || file_pheno.empty()))) {
    std::cerr << "need -lmm 3, -pmax x in [0, 1], -k kin or -d eval -u U, and -bfile or -g/-p" << std::endl;
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
    std::vector<size_t> cols;
    const size_t n_cols = file_pheno.empty() ? 1 : count_columns(file_pheno); // without -p: the phenotype of the .fam file
    if (n_cols == 0) {
      std::cout << "error! no phenotype column in " << file_pheno << std::endl;
      return 3;
    }
    for (size_t t = 0; t < n_cols; ++t) cols.push_back(t + 1);
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
    // ---- eigen pairs: from -k (centre + decompose) or from -d / -u (gemma_file_driver.cpp) ---------------------------------------
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
    // ---- one null model per column, then the scan ----------------------------------------------------------------------------------
    LMM cLmm;
    cLmm.a_mode = 3;
    cLmm.file_bfile = file_bfile;
    cLmm.file_geno = file_geno;
    cLmm.path_out = path_out;
    cLmm.ni_total = ni_total;
    cLmm.indicator_idv = cp.indicator_idv;
    cLmm.indicator_snp = indicator_snp;
    cLmm.snpInfo = std::move(snpInfo);
    std::vector<double> col(ni_test);
    for (size_t t = 0; t < n_ph; ++t) {
      for (size_t i = 0; i < ni_test; ++i) col[i] = UtYb[i * n_ph + t];
      Vector Uty = vector_view(col.data(), ni_test);
      cLmm.l_mle_null_multi.push_back(CalcLambdaNull(&eval, &UtW, &Uty, 1e-5, 1e5, 10, trace_G).l_mle_null);
    }
    if (!file_bfile.empty()) cLmm.AnalyzePlinkScorePanelHits(&U, &eval, &UtW, &UtY, p_max);
    else AnalyzeBimbamScorePanelHits(cLmm, &U, &eval, &UtW, &UtY, p_max);
    // ---- the three files ---------------------------------------------------------------------------------------------------------------
    std::vector<size_t> rows; // snpInfo index of the s-th analysed SNP
    const std::vector<int> keep = cLmm.analysed_snps();
    for (size_t i = 0; i < cLmm.snpInfo.size(); ++i)
      if (i < keep.size() && keep[i]) rows.push_back(i);
    const std::string stem = path_out + "/" + file_out;
    std::ofstream hits_file((stem + ".hits.txt").c_str()), best_file((stem + ".best.txt").c_str()), log_file((stem + ".log.txt").c_str());
    if (!hits_file || !best_file || !log_file) {
      std::cout << "error writing file: " << stem << ".*.txt" << std::endl;
      return 6;
    }
    hits_file << "chr\trs\tps\tn_miss\tallele1\tallele0\taf\tphenotype\tbeta\tse\tp_score" << std::endl;
    write_rows(hits_file, cLmm.scoreHits.size(), [&](AssocLine &ln, size_t k) {
      const gemma_score_hit &h = cLmm.scoreHits[k];
      const SNPINFO &s = cLmm.snpInfo[rows.at(h.snp)];
      ln.str(s.chr).tab().str(s.rs_number).tab().num(s.base_position).tab().unum(s.n_miss).tab().str(s.a_minor).tab().str(s.a_major)
          .tab().fix3(s.maf).tab().unum(cols[h.pheno]).tab().sci(h.beta).tab().sci(h.se).tab().sci(h.p_score);
      ln.endl();
    });
    best_file << "phenotype\trs\tps\tbeta\tse\tp_score" << std::endl;
    write_rows(best_file, cLmm.scoreBest.size(), [&](AssocLine &ln, size_t t) {
      const gemma_score_best &b = cLmm.scoreBest[t];
      ln.unum(cols[t]).tab();
      if (b.snp >= 0) {
        const SNPINFO &s = cLmm.snpInfo[rows.at((size_t)b.snp)];
        ln.str(s.rs_number).tab().num(s.base_position);
      } else {
        ln.str("NA").tab().num(-9);
      }
      ln.tab().sci(b.beta).tab().sci(b.se).tab().sci(b.p_score);
      ln.endl();
    });
    log_file << "## score panel: -lmm 3 of " << n_ph << " phenotypes, p_max = " << p_max << "\n";
    log_file << "## number of total individuals = " << ni_total << "\n## number of analyzed individuals = " << ni_test << "\n";
    log_file << "## number of covariates = " << n_cvt << "\n## number of total SNPs = " << indicator_snp.size()
             << "\n## number of analyzed SNPs = " << ns_test << "\n";
    log_file << std::setprecision(6);
    for (size_t t = 0; t < n_ph; ++t) log_file << "## l_mle_null." << cols[t] << " = " << cLmm.l_mle_null_multi[t] << "\n";
    log_file << "## number of hits = " << cLmm.scoreHits.size() << std::endl;
    std::cout << " snps=" << rows.size() << " hits=" << cLmm.scoreHits.size() << std::endl;
    gemma_hip_shutdown();
  } catch (const std::exception &e) {
    std::cerr << "score_panel_file_driver: " << e.what() << std::endl;
    return 1;
  }
  return 0;
}

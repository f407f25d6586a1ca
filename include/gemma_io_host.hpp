// gemma_io_host.hpp -- the data formats either side of the hot path: the
// readers that decide WHICH individuals and SNPs the device sees, the genotype feeders, and the artefacts the
// reference leaves between runs.  Header-only C++11 over include/gemma_host.hpp and the C ABI.
//
//   phenotypes / covariates / annotation : ReadFile_pheno, ReadFile_fam, ReadFile_cvt, ReadFile_bim, ReadFile_anno
//                                           (src/gemma_io.cpp:280-637), ProcessCvtPhen / CheckCvt / CopyCvtPhen
//                                           (src/param.cpp:1937-2198)
//   first pass over the genotypes         : ReadFile_bed  (src/gemma_io.cpp:876-1064)  -- .bed rows go to the device
//                                           ReadFile_geno (src/gemma_io.cpp:639-873)   -- text rows are parsed by a
//                                           pool of host threads (BimbamReader), statistics and filters on the device
//                                           (gemma_hip_snp_qc)
//   feeders                               : BimbamKin / AnalyzeBimbam over BimbamReader (src/gemma_io.cpp:1418-1597,
//                                           src/lmm.cpp:1660-1706)
//   -eigen / -d -u artefacts              : WriteEigen (src/gemma.cpp:1779-1800 -> PARAM::WriteMatrix / WriteVector),
//                                           ReadFile_eigenU / ReadFile_eigenD (src/gemma_io.cpp:1323-1416)
//   MQS summary statistics (-gs, -vc 1 -beta) : ReadHeader_io, ReadFile_cat, ReadFile_snps_header, ReadFile_beta, Calcq
//                                           (src/gemma_io.cpp:2367-2718, :3363-3551, :3716-3870), ObtainWeight / UpdateSNP
//                                           (src/param.cpp:2214-2296, :2420-2453), CalcVCss (src/vc.cpp:1309-1500), CalcS
//                                           (src/param.cpp:1717-1812: the .bed rows go to gemma_hip_mqs_*), WriteMQS
//   MQS confidence intervals (-ci 1, -ci 2)   : ReadFile_wsnp (-wcat), ObtainWeight with -wcat, UpdateWeight, UpdateSNPnZ,
//                                           ReadFile_beta (signed z and allele), ReadFile_ref, ReadFile_study, CalcCIss
//                                           (src/vc.cpp:2727-2950), PlinkXwz / PlinkXtXwz, BimbamXwz / BimbamXtXwz (the rows go to
//                                           gemma_hip_ci_*), CalcVCssBeta (-vc 1 / -vc 2 with -beta), CalcVCssStudy (-study -ref)
//   windowed SNP correlation (-calccor)     : VARCOV::CalcNB, WriteCov, AnalyzePlink, AnalyzeBimbam (src/varcov.cpp; the rows go to
//                                           gemma_hip_cor_block in blocks of LMM_BATCH_SIZE outputs plus their halo)
//
// Nothing here computes on the host what the reference computes per SNP: counting, imputation and the filters run
// in gemma_hip_snp_qc; the host side only tokenises text and moves bytes.  Text -> double conversion must give the
// very double atof() gives (the reference's readers call atof on every token): parse_double() takes the exact
// fast path (<= 19 digits collected in an integer below 2^53, power of ten <= 10^22: one correctly rounded
// multiplication or division, Clinger 1990) and hands everything else to strtod.
#ifndef GEMMA_IO_HOST_HPP
#define GEMMA_IO_HOST_HPP

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <set>
#include <thread>

#include <zlib.h>

#include "gemma_host.hpp"

namespace gemma_amd {

// ---------------------------------------------------------------------------------------------------------------
// text -> double, identical to atof
// ---------------------------------------------------------------------------------------------------------------
inline double parse_double(const char *s, const char *end) {
  static const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
  const char *p = s;
  bool neg = false;
  if (p < end && (*p == '-' || *p == '+')) neg = (*p++ == '-');
  uint64_t w = 0;
  int nd = 0, frac = 0;
  bool any = false;
  while (p < end && *p >= '0' && *p <= '9') {
    if (nd < 19) { w = w * 10 + (uint64_t)(*p - '0'); if (w) ++nd; } else goto slow;
    ++p; any = true;
  }
  if (p < end && *p == '.') {
    ++p;
    while (p < end && *p >= '0' && *p <= '9') {
      if (nd < 19) { w = w * 10 + (uint64_t)(*p - '0'); if (w) ++nd; ++frac; } else goto slow;
      ++p; any = true;
    }
  }
  if (!any) goto slow;
  {
    int e10 = 0;
    if (p < end && (*p == 'e' || *p == 'E')) {
      const char *q = p + 1;
      bool eneg = false;
      if (q < end && (*q == '-' || *q == '+')) eneg = (*q++ == '-');
      if (q >= end || *q < '0' || *q > '9') goto slow;
      int ev = 0;
      while (q < end && *q >= '0' && *q <= '9') { if (ev < 10000) ev = ev * 10 + (*q - '0'); ++q; }
      e10 = eneg ? -ev : ev;
      p = q;
    }
    if (p != end) goto slow; // trailing characters: let strtod decide where the number ends
    e10 -= frac;
    if (w > (uint64_t(1) << 53) || e10 < -22 || e10 > 22) goto slow;
    double v = (double)w;
    if (e10 < 0) v /= p10[-e10]; else v *= p10[e10];
    return neg ? -v : v;
  }
slow : {
  char buf[64];
  const size_t len = (size_t)(end - s);
  if (len < sizeof(buf)) {
    memcpy(buf, s, len);
    buf[len] = 0;
    return strtod(buf, nullptr);
  }
  return strtod(std::string(s, end).c_str(), nullptr);
}
}

// ---------------------------------------------------------------------------------------------------------------
// plain or gzip-compressed text, line by line (the reference's igzstream + safeGetline, src/gemma_io.cpp:118-151:
// "\n", "\r\n" and "\r" all end a line)
// ---------------------------------------------------------------------------------------------------------------
class TextFile {
public:
  explicit TextFile(const std::string &path) : f_(gzopen(path.c_str(), "rb")), buf_(1 << 20), pos_(0), len_(0) {
    if (f_) gzbuffer(f_, 1 << 20);
  }
  ~TextFile() { if (f_) gzclose(f_); }
  TextFile(const TextFile &) = delete;
  TextFile &operator=(const TextFile &) = delete;
  bool ok() const { return f_ != nullptr; }
  // false at end of file with nothing read (safeGetline(...).eof() on an empty tail)
  bool getline(std::string &line) {
    line.clear();
    bool got = false;
    for (;;) {
      if (pos_ == len_) {
        const int r = f_ ? gzread(f_, buf_.data(), (unsigned)buf_.size()) : 0;
        if (r <= 0) return got;
        len_ = (size_t)r;
        pos_ = 0;
      }
      const char *b = buf_.data() + pos_, *e = buf_.data() + len_;
      const char *q = b;
      while (q < e && *q != '\n' && *q != '\r') ++q;
      line.append(b, q);
      got = got || q > b;
      pos_ = (size_t)(q - buf_.data());
      if (q == e) continue;
      ++pos_;
      if (*q == '\r') { // swallow the "\n" of "\r\n"
        if (pos_ == len_) {
          const int r = gzread(f_, buf_.data(), (unsigned)buf_.size());
          len_ = r > 0 ? (size_t)r : 0;
          pos_ = 0;
        }
        if (pos_ < len_ && buf_[pos_] == '\n') ++pos_;
      }
      return true;
    }
  }

private:
  gzFile f_;
  std::vector<char> buf_;
  size_t pos_, len_;
};

namespace detail {
inline bool is_delim(char c, bool comma) { return c == ' ' || c == '\t' || (comma && c == ','); }
// strtok(line, " ,\t") without touching the buffer: next token [b, e) at or after p
inline bool next_token(const char *&p, const char *end, const char *&b, const char *&e, bool comma = true) {
  while (p < end && is_delim(*p, comma)) ++p;
  if (p >= end) return false;
  b = p;
  while (p < end && !is_delim(*p, comma)) ++p;
  e = p;
  return true;
}
inline bool tok_is_na(const char *b, const char *e) { return e - b == 2 && b[0] == 'N' && b[1] == 'A'; }
} // namespace detail

// ---------------------------------------------------------------------------------------------------------------
// phenotypes, covariates, annotation
// ---------------------------------------------------------------------------------------------------------------
// ReadFile_snps, src/gemma_io.cpp:153-178 (`-snps`): one SNP id per line (first token)
inline bool ReadFile_snps(const std::string &file_snps, std::set<std::string> &setSnps) {
  setSnps.clear();
  TextFile infile(file_snps);
  if (!infile.ok()) {
    std::cout << "error! fail to open snps file: " << file_snps << std::endl;
    return false;
  }
  std::string line;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    if (!detail::next_token(p, end, b, e)) {
      std::cout << "Problem reading SNP file" << std::endl;
      return false;
    }
    setSnps.insert(std::string(b, e));
  }
  return true;
}

// ReadFile_column, src/gemma_io.cpp:344-383: one column of a text file (the -gxe / -widv inputs); "NA" -> indicator 0
inline bool ReadFile_column(const std::string &file_pheno, std::vector<int> &indicator_idv, std::vector<double> &pheno,
                            const int &p_column) {
  indicator_idv.clear();
  pheno.clear();
  TextFile infile(file_pheno);
  if (!infile.ok()) {
    std::cout << "error! fail to open phenotype file: " << file_pheno << std::endl;
    return false;
  }
  std::string line;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b = nullptr, *e = nullptr;
    bool have = false;
    for (int i = 0; i < p_column; ++i) have = detail::next_token(p, end, b, e);
    if (!have) {
      std::cout << "Problem reading PHENO column" << std::endl;
      return false;
    }
    if (detail::tok_is_na(b, e)) {
      indicator_idv.push_back(0);
      pheno.push_back(-9);
    } else {
      indicator_idv.push_back(1);
      pheno.push_back(parse_double(b, e));
    }
  }
  return true;
}

// ReadFile_pheno, src/gemma_io.cpp:386-444: BIMBAM phenotype file, p_column = 1-based columns; "NA" -> indicator 0, -9
inline bool ReadFile_pheno(const std::string &file_pheno, std::vector<std::vector<int>> &indicator_pheno,
                           std::vector<std::vector<double>> &pheno, const std::vector<size_t> &p_column) {
  indicator_pheno.clear();
  pheno.clear();
  TextFile infile(file_pheno);
  if (!infile.ok()) {
    std::cout << "error! fail to open phenotype file: " << file_pheno << std::endl;
    return false;
  }
  const size_t p_max = *std::max_element(p_column.begin(), p_column.end());
  std::map<size_t, size_t> mapP2c;
  for (size_t i = 0; i < p_column.size(); i++) mapP2c[p_column[i]] = i;
  std::vector<double> pheno_row(p_column.size(), -9);
  std::vector<int> ind_pheno_row(p_column.size(), 0);
  std::string line;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    for (size_t i = 0; i < p_max; ++i) {
      if (!detail::next_token(p, end, b, e)) {
        std::cout << "Number of phenotypes in pheno file do not match phenotypes in geno file" << std::endl;
        return false;
      }
      std::map<size_t, size_t>::const_iterator it = mapP2c.find(i + 1);
      if (it == mapP2c.end()) continue;
      if (detail::tok_is_na(b, e)) {
        ind_pheno_row[it->second] = 0;
        pheno_row[it->second] = -9;
      } else {
        ind_pheno_row[it->second] = 1;
        pheno_row[it->second] = parse_double(b, e);
      }
    }
    indicator_pheno.push_back(ind_pheno_row);
    pheno.push_back(pheno_row);
  }
  return true;
}

// ReadFile_fam, src/gemma_io.cpp:559-635: phenotype = column 6 (+ further columns); "NA" and -9 are missing
inline bool ReadFile_fam(const std::string &file_fam, std::vector<std::vector<int>> &indicator_pheno,
                         std::vector<std::vector<double>> &pheno, std::map<std::string, int> &mapID2num,
                         const std::vector<size_t> &p_column) {
  indicator_pheno.clear();
  pheno.clear();
  mapID2num.clear();
  TextFile infile(file_fam);
  if (!infile.ok()) {
    std::cout << "error opening .fam file: " << file_fam << std::endl;
    return false;
  }
  const size_t p_max = *std::max_element(p_column.begin(), p_column.end());
  std::map<size_t, size_t> mapP2c;
  for (size_t i = 0; i < p_column.size(); i++) mapP2c[p_column[i]] = i;
  std::vector<double> pheno_row(p_column.size(), -9);
  std::vector<int> ind_pheno_row(p_column.size(), 0);
  std::string line;
  int c = 0;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    std::string id;
    for (int k = 0; k < 5; ++k) { // family, individual, father, mother, sex: " \t" only
      if (!detail::next_token(p, end, b, e, false)) {
        std::cout << "Parsing input file '" << file_fam << "' failed in function ReadFile_fam" << std::endl;
        return false;
      }
      if (k == 1) id.assign(b, e);
    }
    bool have = detail::next_token(p, end, b, e, false); // first phenotype: " \t"; the following ones " ,\t"
    for (size_t i = 0; i < p_max; ++i) {
      std::map<size_t, size_t>::const_iterator it = mapP2c.find(i + 1);
      if (it != mapP2c.end()) {
        if (!have) {
          std::cout << "Problem reading FAM file (phenotypes do not match geno file)" << std::endl;
          return false;
        }
        const double v = detail::tok_is_na(b, e) ? -9.0 : parse_double(b, e);
        if (detail::tok_is_na(b, e) || v == -9) {
          ind_pheno_row[it->second] = 0;
          pheno_row[it->second] = -9;
        } else {
          ind_pheno_row[it->second] = 1;
          pheno_row[it->second] = v;
        }
      }
      have = detail::next_token(p, end, b, e, true);
    }
    indicator_pheno.push_back(ind_pheno_row);
    pheno.push_back(pheno_row);
    mapID2num[id] = c++;
  }
  return true;
}

// ReadFile_cvt, src/gemma_io.cpp:446-511: a row with any "NA" is flagged 0; all flagged-1 rows must have n_cvt columns
inline bool ReadFile_cvt(const std::string &file_cvt, std::vector<int> &indicator_cvt,
                         std::vector<std::vector<double>> &cvt, size_t &n_cvt) {
  indicator_cvt.clear();
  TextFile infile(file_cvt);
  if (!infile.ok()) {
    std::cout << "error! fail to open covariates file: " << file_cvt << std::endl;
    return false;
  }
  std::string line;
  while (infile.getline(line)) {
    std::vector<double> v_d;
    int flag_na = 0;
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    while (detail::next_token(p, end, b, e)) {
      if (detail::tok_is_na(b, e)) {
        flag_na = 1;
        v_d.push_back(-9);
      } else {
        v_d.push_back(parse_double(b, e));
      }
    }
    indicator_cvt.push_back(flag_na == 0 ? 1 : 0);
    cvt.push_back(v_d);
  }
  if (indicator_cvt.empty()) {
    n_cvt = 0;
  } else {
    int first = 0;
    for (size_t i = 0; i < indicator_cvt.size(); ++i) {
      if (indicator_cvt[i] == 0) continue;
      if (first == 0) {
        first = 1;
        n_cvt = cvt[i].size();
      }
      if (n_cvt != cvt[i].size()) {
        std::cout << "error! number of covariates in row " << i << " do not match other rows." << std::endl;
        return false;
      }
    }
  }
  return true;
}

// ReadFile_bim, src/gemma_io.cpp:514-556: chr rs cM bp minor major (" \t" separated)
inline bool ReadFile_bim(const std::string &file_bim, std::vector<SNPINFO> &snpInfo) {
  snpInfo.clear();
  TextFile infile(file_bim);
  if (!infile.ok()) {
    std::cout << "error opening .bim file: " << file_bim << std::endl;
    return false;
  }
  std::string line;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b[6], *e[6];
    for (int k = 0; k < 6; ++k)
      if (!detail::next_token(p, end, b[k], e[k], false)) {
        std::cout << "Parsing input file '" << file_bim << "' failed in function ReadFile_bim" << std::endl;
        return false;
      }
    SNPINFO s;
    s.chr.assign(b[0], e[0]);
    s.rs_number.assign(b[1], e[1]);
    s.cM = parse_double(b[2], e[2]);
    s.base_position = atol(std::string(b[3], e[3]).c_str());
    s.a_minor.assign(b[4], e[4]);
    s.a_major.assign(b[5], e[5]);
    s.n_miss = 0;
    s.missingness = -9;
    s.maf = -9;
    s.n_idv = 0;
    s.n_nb = 0;
    s.file_position = 0;
    snpInfo.push_back(s);
  }
  return true;
}

// ReadFile_anno, src/gemma_io.cpp:280-341: rs, bp, chr, cM ("NA" or absent -> -9)
inline bool ReadFile_anno(const std::string &file_anno, std::map<std::string, std::string> &mapRS2chr,
                          std::map<std::string, long int> &mapRS2bp, std::map<std::string, double> &mapRS2cM) {
  mapRS2chr.clear();
  mapRS2bp.clear();
  TextFile infile(file_anno);
  if (!infile.ok()) {
    std::cout << "error opening annotation file: " << file_anno << std::endl;
    return false;
  }
  std::string line;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    if (!detail::next_token(p, end, b, e)) {
      std::cout << line << " Bad RS format" << std::endl;
      return false;
    }
    const std::string rs(b, e);
    if (!detail::next_token(p, end, b, e)) {
      std::cout << line << " Bad format" << std::endl;
      return false;
    }
    const long b_pos = detail::tok_is_na(b, e) ? -9 : atol(std::string(b, e).c_str());
    if (b_pos == 0) {
      std::cout << line << " Bad pos format (is zero)" << std::endl;
      return false;
    }
    std::string chr = "-9";
    double cM = -9;
    if (detail::next_token(p, end, b, e)) {
      if (!detail::tok_is_na(b, e)) chr.assign(b, e);
      if (detail::next_token(p, end, b, e) && !detail::tok_is_na(b, e)) cM = parse_double(b, e);
    }
    mapRS2chr[rs] = chr;
    mapRS2bp[rs] = b_pos;
    mapRS2cM[rs] = cM;
  }
  return true;
}

// The individual-selection state of PARAM (src/param.h:225-262) and the three functions that fill it
struct CvtPhen {
  std::vector<std::vector<int>> indicator_pheno;
  std::vector<std::vector<double>> pheno;
  std::vector<int> indicator_cvt;
  std::vector<std::vector<double>> cvt;
  std::vector<int> indicator_gxe; // -gxe: environment variable per individual (src/param.cpp:228-233)
  std::vector<double> gxe;
  std::vector<int> indicator_idv;
  size_t n_cvt = 0, ni_test = 0;
  bool error = false;

  // PARAM::CheckCvt, src/param.cpp:1937-1990: constant columns count as intercepts; if every column is one the
  // covariates are dropped, if none is a column of 1s is appended
  void CheckCvt() {
    if (indicator_cvt.empty()) return;
    size_t flag_ipt = 0, n_remove = 0;
    for (size_t j = 0; j < n_cvt; ++j) {
      double v_min = std::numeric_limits<double>::infinity(), v_max = -v_min;
      for (size_t i = 0; i < indicator_idv.size(); ++i) {
        if (indicator_idv[i] == 0 || indicator_cvt[i] == 0) continue;
        v_min = std::min(v_min, cvt[i][j]);
        v_max = std::max(v_max, cvt[i][j]);
      }
      if (v_min == v_max) {
        flag_ipt = 1;
        ++n_remove;
      }
    }
    if (n_cvt == n_remove) {
      // the reference keeps the rows of cvt and later copies their FIRST column as the single covariate
      // (src/param.cpp:1974-1976, 2146-2170): a constant column other than 1 becomes the intercept as it stands
      indicator_cvt.clear();
      n_cvt = 1;
    } else if (flag_ipt == 0) {
      std::cerr << "**** INFO: no intercept term is found in the cvt file: a column of 1s is added." << std::endl;
      for (size_t i = 0; i < indicator_idv.size(); ++i) {
        if (indicator_idv[i] == 0 || indicator_cvt[i] == 0) continue;
        cvt[i].push_back(1.0);
      }
      n_cvt++;
    }
  }

  // PARAM::ProcessCvtPhen, src/param.cpp:1993-2098 (no -widv / subsampling here)
  void ProcessCvtPhen() {
    indicator_idv.clear();
    for (size_t i = 0; i < indicator_pheno.size(); i++) {
      int k = 1;
      for (size_t j = 0; j < indicator_pheno[i].size(); j++)
        if (indicator_pheno[i][j] == 0) k = 0;
      indicator_idv.push_back(k);
    }
    if (!indicator_cvt.empty())
      for (size_t i = 0; i < indicator_idv.size(); ++i) indicator_idv[i] *= indicator_cvt[i];
    if (!indicator_gxe.empty()) // individuals with a missing environment value leave the analysis (:2016-2020)
      for (size_t i = 0; i < indicator_idv.size(); ++i) indicator_idv[i] *= indicator_gxe[i];
    ni_test = 0;
    for (size_t i = 0; i < indicator_idv.size(); ++i) ni_test += indicator_idv[i] != 0;
    if (ni_test == 0) {
      error = true;
      std::cout << "error! number of analyzed individuals equals 0. " << std::endl;
    }
    if (!indicator_cvt.empty()) {
      CheckCvt();
    } else {
      cvt.assign(indicator_idv.size(), std::vector<double>(1, 1.0)); // no -c file: the intercept alone
      indicator_cvt.assign(indicator_idv.size(), 1);
      n_cvt = 1;
    }
  }

  // PARAM::CopyGxe, src/param.cpp:2116-2128
  void CopyGxe(std::vector<double> &env) const {
    env.clear();
    for (size_t i = 0; i < indicator_idv.size(); ++i)
      if (indicator_idv[i] != 0 && indicator_gxe[i] != 0) env.push_back(gxe[i]);
  }

  // PARAM::CopyCvtPhen (flag 0), src/param.cpp:2146-2198: W (ni_test x n_cvt), Y (ni_test x n_ph) of the analysed
  void CopyCvtPhen(std::vector<double> &W, std::vector<double> &Y) const {
    const size_t n_ph = pheno.empty() ? 0 : pheno[0].size();
    W.assign(ni_test * n_cvt, 0.0);
    Y.assign(ni_test * n_ph, 0.0);
    size_t ci = 0;
    for (size_t i = 0; i < indicator_idv.size(); ++i) {
      if (indicator_idv[i] == 0) continue;
      for (size_t j = 0; j < n_ph; ++j) Y[ci * n_ph + j] = pheno[i][j];
      for (size_t j = 0; j < n_cvt; ++j) W[ci * n_cvt + j] = cvt[i][j];
      ci++;
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------
// BIMBAM mean-genotype text -> fp64 SNP-major blocks on a pool of host threads
// ---------------------------------------------------------------------------------------------------------------
// One line = rs, allele, allele, then ni_total values ("NA" = missing -> NaN); separators " ,\t".  read_block() pulls
// the text of up to max_snps lines through zlib in large reads on the calling thread (decompression is sequential by
// nature), finds the line ends with memchr, and splits the lines over n_threads parsers that work in place on the
// text buffer and write their own rows of the block: every value costs one token scan and -- for the usual
// "0.123"-style dosages -- one integer accumulation and one division; no locale, no allocation, no copy of the line.
class BimbamReader {
public:
  struct Row {
    std::string rs, minor, major;
  };
  // skip_fields: leading tokens that are not values (3 for BIMBAM: rs, allele, allele; 0 for a plain matrix such as the
  // kinship file); strict_columns: a line with more than skip_fields + ni_total tokens is malformed
  BimbamReader(const std::string &path, size_t ni_total, unsigned n_threads = 0, int skip_fields = 3,
               bool strict_columns = false)
      : f_(gzopen(path.c_str(), "rb")), ni_total_(ni_total), n_threads_(n_threads ? n_threads : default_threads()),
        skip_(skip_fields), strict_(strict_columns), line_no_(0), beg_(0), end_(0), eof_(false), buf_(nullptr), cap_(0) {
    if (f_) gzbuffer(f_, 1 << 20);
  }
  ~BimbamReader() {
    if (f_) gzclose(f_);
    free(buf_);
  }
  BimbamReader(const BimbamReader &) = delete;
  BimbamReader &operator=(const BimbamReader &) = delete;
  bool ok() const { return f_ != nullptr; }
  size_t lines_read() const { return line_no_; }
  size_t text_buffer_bytes() const { return cap_; } // capacity of the text buffer (tests: stays O(chunk) over dropped lines)
  // consumes one line without counting it (the header of a gene-expression file); false at end of file
  bool skip_line() {
    if (!f_) return false;
    for (;;) {
      size_t b, e, next;
      if (next_line(beg_, b, e, next)) {
        beg_ = next;
        return true;
      }
      if (eof_) {
        const bool had = beg_ < end_;
        beg_ = end_;
        return had;
      }
      if (beg_ > 0) {
        memmove(buf_, buf_ + beg_, end_ - beg_);
        end_ -= beg_;
        beg_ = 0;
      }
      fill();
    }
  }
  static unsigned default_threads() {
    const char *env = getenv("GEMMA_HIP_IO_THREADS");
    if (env && atoi(env) > 0) return (unsigned)atoi(env);
    const unsigned hc = std::thread::hardware_concurrency();
    return hc ? std::min(hc, 32u) : 4u;
  }
  // Reads up to max_snps further lines (fewer when their text would pass TEXT_CAP bytes); lines whose `keep` entry
  // (indexed by file line) is 0 are consumed and dropped without being parsed.  X gets rows x ld doubles (ld >= number
  // of columns kept); cols (optional, ni_total ints) selects the individuals copied into a row, in order.  Returns the
  // number of rows produced, 0 at end of file, or (size_t)-1 on a malformed line (message printed, as the reference's
  // enforce would).
  size_t read_block(size_t max_snps, double *X, size_t ld, std::vector<Row> *rows = nullptr,
                    const std::vector<int> *keep = nullptr, const int *cols = nullptr) {
    if (!f_) return 0;
    // drop the text of the previous block, keep the unconsumed tail at the front
    if (beg_ > 0) {
      memmove(buf_, buf_ + beg_, end_ - beg_);
      end_ -= beg_;
      beg_ = 0;
    }
    spans_.clear();
    size_t scan = 0; // everything before `scan` has been split into lines
    while (spans_.size() < max_snps) {
      size_t b, e, next;
      if (!next_line(scan, b, e, next)) {
        if (eof_) {
          if (scan < end_) { // last line without a line end
            b = scan; e = end_; next = end_;
          } else {
            break;
          }
        } else {
          if (!spans_.empty() && end_ >= text_cap()) break;
          // nothing kept yet: the text before `scan` belongs to dropped lines only (a shard's skipped prefix, -loco /
          // -snps with the kept SNPs late in the file) -- discard it so that the buffer tracks one chunk, not the prefix
          if (spans_.empty() && scan > 0) {
            memmove(buf_, buf_ + scan, end_ - scan);
            end_ -= scan;
            scan = 0;
          }
          fill();
          continue;
        }
      }
      scan = next;
      if (e == b && eof_ && scan == end_) break; // empty tail
      const size_t t = line_no_++;
      if (keep && t < keep->size() && (*keep)[t] == 0) continue;
      spans_.push_back(std::make_pair(b, e));
    }
    beg_ = scan;
    const size_t l = spans_.size();
    if (l == 0) return 0;
    if (rows) rows->assign(l, Row());
    const unsigned nt = (unsigned)std::max<size_t>(1, std::min<size_t>(n_threads_, (l + 7) / 8));
    std::vector<int> bad(nt, 0);
    auto work = [&](unsigned w, size_t r0, size_t r1) {
      for (size_t r = r0; r < r1; ++r)
        if (!parse_line(buf_ + spans_[r].first, buf_ + spans_[r].second, X + r * ld,
                        rows ? &(*rows)[r] : nullptr, cols))
          bad[w] = 1;
    };
    if (nt == 1) {
      work(0, 0, l);
    } else {
      std::vector<std::thread> pool;
      for (unsigned w = 1; w < nt; ++w) pool.emplace_back(work, w, l * w / nt, l * (w + 1) / nt);
      work(0, 0, l / nt);
      for (std::thread &th : pool) th.join();
    }
    for (int b : bad)
      if (b) {
        if (skip_ == 3) std::cout << "Problem reading geno file (not enough genotypes in line)" << std::endl;
        return (size_t)-1;
      }
    return l;
  }

private:
  static constexpr size_t TEXT_CAP = size_t(1) << 30, CHUNK = size_t(16) << 20;
  // bytes of text one block may hold before read_block returns what it has (GEMMA_HIP_IO_TEXT_CAP: test hook)
  static size_t text_cap() {
    const char *env = getenv("GEMMA_HIP_IO_TEXT_CAP");
    return env && atol(env) > 0 ? (size_t)atol(env) : TEXT_CAP;
  }
  // appends up to CHUNK further bytes of text
  void fill() {
    const size_t chunk = std::min(CHUNK, text_cap()); // (a small test cap also makes the reads small)
    if (cap_ < end_ + chunk) { // plain realloc: no zero fill of text that is about to be overwritten
      cap_ = std::max(cap_ + cap_ / 2, end_ + chunk);
      char *nb = static_cast<char *>(realloc(buf_, cap_));
      if (!nb) throw std::bad_alloc();
      buf_ = nb;
    }
    const int r = gzread(f_, buf_ + end_, (unsigned)chunk);
    if (r <= 0) eof_ = true; else end_ += (size_t)r;
  }
  // next complete line [b, e) at or after `from`; "\n", "\r\n" and "\r" end a line (src/gemma_io.cpp:118-151)
  bool next_line(size_t from, size_t &b, size_t &e, size_t &next) const {
    if (from >= end_) return false;
    const char *base = buf_;
    const char *nl = (const char *)memchr(base + from, '\n', end_ - from);
    const size_t lim = nl ? (size_t)(nl - base) : end_;
    const char *cr = (const char *)memchr(base + from, '\r', lim - from);
    if (cr) {
      const size_t q = (size_t)(cr - base);
      if (q + 1 == end_ && !eof_) return false; // cannot tell "\r" from "\r\n" yet
      b = from; e = q;
      next = (q + 1 < end_ && base[q + 1] == '\n') ? q + 2 : q + 1;
      return true;
    }
    if (!nl) return false;
    b = from; e = lim; next = lim + 1;
    return true;
  }
  bool parse_line(const char *p, const char *end, double *x, Row *row, const int *cols) const {
    const char *b, *e;
    for (int k = 0; k < skip_; ++k) {
      if (!detail::next_token(p, end, b, e)) return false;
      if (row) (k == 0 ? row->rs : k == 1 ? row->minor : row->major).assign(b, e);
    }
    size_t o = 0;
    for (size_t i = 0; i < ni_total_; ++i) {
      if (!detail::next_token(p, end, b, e)) return false;
      if (cols && cols[i] == 0) continue;
      // only the genotype reader knows "NA"; the kinship and gene-expression readers call atof on every token
      x[o++] = (skip_ == 3 && detail::tok_is_na(b, e)) ? std::numeric_limits<double>::quiet_NaN() : parse_double(b, e);
    }
    return !(strict_ && detail::next_token(p, end, b, e));
  }
  gzFile f_;
  size_t ni_total_;
  unsigned n_threads_;
  int skip_;
  bool strict_;
  size_t line_no_, beg_, end_;
  bool eof_;
  char *buf_;
  size_t cap_;
  std::vector<std::pair<size_t, size_t>> spans_;
};

// rows per block of the text feeders: at most `cap` rows and about 256 MiB of doubles (two such slots are in flight)
inline size_t bimbam_block_rows(size_t row_len, size_t cap) {
  return io_block_rows(std::max<size_t>(64, std::min<size_t>(cap, (size_t(256) << 20) / (8 * std::max<size_t>(row_len, 1)))));
}

// ---------------------------------------------------------------------------------------------------------------
// first pass: which SNPs are analysed
// ---------------------------------------------------------------------------------------------------------------
struct QcLevels {
  double maf_level = 0.01, miss_level = 0.05, hwe_level = 0, r2_level = 0.9999; // src/param.cpp:94-107
};

// ReadFile_bed, src/gemma_io.cpp:876-1064.  W: ni_test x n_cvt covariates of the analysed individuals.
inline bool ReadFile_bed(const std::string &file_bed, const std::set<std::string> &setSnps, const Matrix *W,
                         std::vector<int> &indicator_idv, std::vector<int> &indicator_snp,
                         std::vector<SNPINFO> &snpInfo, const double &maf_level, const double &miss_level,
                         const double &hwe_level, const double &r2_level, size_t &ns_test) {
  indicator_snp.clear();
  const size_t ns_total = snpInfo.size();
  std::ifstream infile(file_bed.c_str(), std::ios::binary);
  if (!infile) {
    std::cout << "error reading bed file:" << file_bed << std::endl;
    return false;
  }
  if (W->tda != W->size2) return false;
  const size_t ni_total = indicator_idv.size(), n_bit = (ni_total + 3) / 4;
  size_t ni_test = 0;
  for (int v : indicator_idv) ni_test += v;
  ns_test = 0;
  const gemma_qc_cfg cfg = {maf_level, miss_level, hwe_level, r2_level};
  const size_t B = io_block_rows(std::min<size_t>(std::max<size_t>(ns_total, 1), K_BATCH_SIZE));
  std::vector<int> ind(B);
  std::vector<double> maf(B);
  std::vector<size_t> n_miss(B);
  const std::vector<int> all(ns_total, 1); // the first pass looks at every SNP of the file
  size_t t_next = 0;
  BlockPrefetch pf(B * n_bit, [&](void *slot, int) {
    return read_bed_rows(infile, all, t_next, n_bit, static_cast<unsigned char *>(slot), B);
  });
  for (size_t t0 = 0; t0 < ns_total;) {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == 0 || l == (size_t)-1) {
      std::cout << "error reading bed file:" << file_bed << " (truncated)" << std::endl;
      return false;
    }
    enforce_hip(gemma_hip_snp_qc(GEMMA_GENO_PLINK_2BIT, slot, l, n_bit, indicator_idv.data(), ni_total, W->data, W->size1,
                                 W->size2, &cfg, ind.data(), maf.data(), n_miss.data()),
                "ReadFile_bed");
    for (size_t i = 0; i < l; ++i) {
      SNPINFO &s = snpInfo[t0 + i];
      s.file_position = t0 + i;
      if (!setSnps.empty() && setSnps.count(s.rs_number) == 0) {
        s.n_miss = (size_t)-9;
        s.missingness = -9;
        s.maf = -9;
        indicator_snp.push_back(0);
        continue;
      }
      s.n_miss = n_miss[i];
      s.missingness = (double)n_miss[i] / (double)ni_test;
      s.maf = maf[i];
      s.n_idv = ni_test - n_miss[i];
      s.n_nb = 0;
      indicator_snp.push_back(ind[i]);
      ns_test += ind[i] != 0;
    }
    t0 += l;
  }
  return true;
}

// ReadFile_geno (first pass), src/gemma_io.cpp:639-873
inline bool ReadFile_geno(const std::string &file_geno, const std::set<std::string> &setSnps, const Matrix *W,
                          std::vector<int> &indicator_idv, std::vector<int> &indicator_snp, const double &maf_level,
                          const double &miss_level, const double &hwe_level, const double &r2_level,
                          std::map<std::string, std::string> &mapRS2chr, std::map<std::string, long int> &mapRS2bp,
                          std::map<std::string, double> &mapRS2cM, std::vector<SNPINFO> &snpInfo, size_t &ns_test) {
  indicator_snp.clear();
  snpInfo.clear();
  const size_t ni_total = indicator_idv.size();
  BimbamReader rd(file_geno, ni_total);
  if (!rd.ok()) {
    std::cout << "error reading genotype file:" << file_geno << std::endl;
    return false;
  }
  if (W->tda != W->size2) return false;
  size_t ni_test = 0;
  for (int v : indicator_idv) ni_test += v;
  ns_test = 0;
  const gemma_qc_cfg cfg = {maf_level, miss_level, hwe_level, r2_level};
  const size_t B = bimbam_block_rows(ni_total, 8192);
  std::vector<BimbamReader::Row> names[2];
  std::vector<int> ind(B);
  std::vector<double> maf(B);
  std::vector<size_t> n_miss(B);
  size_t file_pos = 0;
  // block k+1 is read and parsed while the device filters block k
  BlockPrefetch pf(B * ni_total * sizeof(double), [&](void *slot, int k) {
    return rd.read_block(B, static_cast<double *>(slot), ni_total, &names[k]);
  });
  for (;;) {
    void *slot = nullptr;
    int k = 0;
    const size_t l = pf.next(slot, &k);
    if (l == (size_t)-1) return false;
    if (l == 0) break;
    const std::vector<BimbamReader::Row> &rows = names[k];
    enforce_hip(gemma_hip_snp_qc(GEMMA_GENO_F64_SNP_MAJOR, slot, l, ni_total, indicator_idv.data(), ni_total, W->data,
                                 W->size1, W->size2, &cfg, ind.data(), maf.data(), n_miss.data()),
                "ReadFile_geno");
    for (size_t i = 0; i < l; ++i, ++file_pos) {
      const BimbamReader::Row &r = rows[i];
      SNPINFO s;
      s.rs_number = r.rs;
      s.a_minor = r.minor;
      s.a_major = r.major;
      s.n_nb = 0;
      s.file_position = file_pos;
      if (!setSnps.empty() && setSnps.count(r.rs) == 0) { // src/gemma_io.cpp:722-731
        s.chr = "-9"; s.cM = -9; s.base_position = -9; s.n_miss = 0; s.missingness = -9; s.maf = -9; s.n_idv = 0;
        snpInfo.push_back(s);
        indicator_snp.push_back(0);
        continue;
      }
      std::map<std::string, long int>::const_iterator it = mapRS2bp.find(r.rs);
      if (it == mapRS2bp.end()) {
        s.chr = "-9"; s.base_position = -9; s.cM = -9;
      } else {
        s.base_position = it->second; s.chr = mapRS2chr[r.rs]; s.cM = mapRS2cM[r.rs];
      }
      s.n_miss = n_miss[i];
      s.missingness = (double)n_miss[i] / (double)ni_test;
      s.maf = maf[i];
      s.n_idv = ni_test - n_miss[i];
      snpInfo.push_back(s);
      indicator_snp.push_back(ind[i]);
      ns_test += ind[i] != 0;
    }
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------
// feeders over the threaded reader
// ---------------------------------------------------------------------------------------------------------------
// LOCO_set_Snps, src/param.cpp:52-66: with `-loco C` the kinship uses the annotated SNPs NOT on chromosome C and the
// association tests the ones on it (SNPs without annotation are in neither set)
inline void LOCO_set_Snps(std::set<std::string> &ksnps, std::set<std::string> &gwasnps,
                          const std::map<std::string, std::string> &mapchr, const std::string &loco) {
  for (std::map<std::string, std::string>::const_iterator kv = mapchr.begin(); kv != mapchr.end(); ++kv)
    (kv->second != loco ? ksnps : gwasnps).insert(kv->first);
}

// BimbamKin, src/gemma_io.cpp:1418-1597 (kinship over ALL ni_total individuals, analysed SNPs only; with a non-empty
// ksnps only its members, :1478-1480 -- snpInfo supplies the rs of every file line from the first pass)
inline bool BimbamKinThreaded(const std::string &file_geno, const std::vector<int> &indicator_snp_in, const int k_mode,
                              Matrix *matrix_kin, const std::set<std::string> &ksnps = std::set<std::string>(),
                              const std::vector<SNPINFO> *snpInfo = nullptr, const KinKeep &kk = KinKeep()) {
  std::vector<int> indicator_snp(indicator_snp_in);
  if (!ksnps.empty() && snpInfo)
    for (size_t t = 0; t < indicator_snp.size() && t < snpInfo->size(); ++t)
      if (indicator_snp[t] && ksnps.count((*snpInfo)[t].rs_number) == 0) indicator_snp[t] = 0;
  if (kk.keep) shard_keep(indicator_snp, kk.rank, kk.world);
  const size_t ni_total = matrix_kin->size1;
  BimbamReader rd(file_geno, ni_total);
  if (!rd.ok()) {
    std::cout << "error reading genotype file:" << file_geno << std::endl;
    return false;
  }
  if (matrix_kin->tda != matrix_kin->size2) return false;
  enforce_hip(gemma_hip_kin_begin(ni_total, k_mode), "BimbamKin");
  const size_t B = bimbam_block_rows(ni_total, 8192);
  BlockPrefetch pf(B * ni_total * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= indicator_snp.size()) return 0;
    return rd.read_block(B, static_cast<double *>(slot), ni_total, nullptr, &indicator_snp);
  });
  for (;;) {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) return false;
    if (l == 0) break;
    enforce_hip(gemma_hip_kin_add(GEMMA_GENO_F64_SNP_MAJOR, slot, l, ni_total), "BimbamKin");
  }
  kin_finish(matrix_kin, kk, "BimbamKin");
  return true;
}

// LMM::AnalyzeBimbam, src/lmm.cpp:1660-1706: rows of the analysed SNPs over the analysed individuals, NaN = missing,
// in blocks of LMM_BATCH_SIZE rows at most (about 256 MiB of doubles per block), parsed one block ahead of the device
inline void AnalyzeBimbam(LMM &lmm, const Matrix *U, const Vector *eval, const Matrix *UtW, const Vector *Uty) {
  const size_t ni_total = lmm.indicator_idv.size(), n = U->size1;
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
  lmm.AnalyzeFeed(U, eval, UtW, Uty, feed, B, n);
}

// the same for T phenotypes over one pass of the file (LMM::AnalyzeFeedMulti)
inline void AnalyzeBimbamMulti(LMM &lmm, const Matrix *U, const Vector *eval, const Matrix *UtW, const Matrix *UtY) {
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
  lmm.AnalyzeFeedMulti(U, eval, UtW, UtY, feed, B, n);
}

// MVLMM::AnalyzeBimbam, src/mvlmm.cpp:2972-3416, over the same threaded reader (mv.file_geno, mv.indicator_idv / _snp)
inline void AnalyzeBimbam(MVLMM &mv, const Matrix *U, const Vector *eval, const Matrix *UtW, const Matrix *UtY) {
  const size_t ni_total = mv.indicator_idv.size(), n = U->size1;
  BimbamReader rd(mv.file_geno, ni_total);
  if (!rd.ok()) throw std::runtime_error("error reading genotype file");
  const size_t B = bimbam_block_rows(n, LMM_BATCH_SIZE);
  const std::vector<int> keep = mv.analysed_snps();
  BlockPrefetch pf(B * n * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= keep.size()) return 0;
    return rd.read_block(B, static_cast<double *>(slot), n, nullptr, &keep, mv.indicator_idv.data());
  });
  LMM::RowFeeder feed = [&](const double *&X) -> size_t {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) throw std::runtime_error("Problem reading geno file (not enough genotypes in line)");
    X = static_cast<const double *>(slot);
    return l;
  };
  mv.AnalyzeFeed(U, eval, UtW, UtY, feed, B, n);
}

// ReadFile_gene, src/gemma_io.cpp:2307-2364 (`-gene`): a header line, then one row per gene: id and ni_total expression
// values.  Only the ids (into snpInfo.rs_number) and the row count matter to the LMM path.
inline bool ReadFile_gene(const std::string &file_gene, std::vector<SNPINFO> &snpInfo, size_t &ng_total) {
  ng_total = 0;
  TextFile infile(file_gene);
  if (!infile.ok()) {
    std::cout << "error! fail to open gene expression file: " << file_gene << std::endl;
    return false;
  }
  std::string line;
  infile.getline(line); // header
  size_t n_idv = 0;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    if (!detail::next_token(p, end, b, e)) {
      std::cout << "Parsing input file '" << file_gene << "' failed in function ReadFile_gene" << std::endl;
      return false;
    }
    SNPINFO s;
    s.chr = "-9"; s.rs_number.assign(b, e); s.cM = -9; s.base_position = -9; s.a_minor = "-9"; s.a_major = "-9";
    s.n_miss = 0; s.missingness = -9; s.maf = -9; s.n_idv = 0; s.n_nb = 0; s.file_position = 0;
    size_t t = 0;
    while (detail::next_token(p, end, b, e)) ++t;
    if (ng_total == 0) n_idv = t;
    if (t != n_idv) {
      std::cout << "error! number of columns doesn't match in row: " << ng_total << std::endl;
      return false;
    }
    snpInfo.push_back(s);
    ng_total++;
  }
  return true;
}

// LMM::AnalyzeGene, src/lmm.cpp:1365-1471, from the file: rows = genes over the analysed individuals (atof on every
// token), the tested variable is the -p phenotype whose rotation arrives in Utx; ng_total rows after the header
inline void AnalyzeGene(LMM &lmm, const Matrix *U, const Vector *eval, const Matrix *UtW, const Vector *Utx, size_t ng_total) {
  const size_t ni_total = lmm.indicator_idv.size(), n = U->size1;
  BimbamReader rd(lmm.file_gene, ni_total, 0, 1);
  if (!rd.ok() || !rd.skip_line()) throw std::runtime_error("error reading gene expression file");
  const size_t B = bimbam_block_rows(n, LMM_BATCH_SIZE);
  BlockPrefetch pf(B * n * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= ng_total) return 0;
    return rd.read_block(std::min(B, ng_total - rd.lines_read()), static_cast<double *>(slot), n, nullptr, nullptr,
                         lmm.indicator_idv.data());
  });
  LMM::RowFeeder feed = [&](const double *&Y) -> size_t {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) throw std::runtime_error("Parsing the gene expression file failed (not enough columns)");
    Y = static_cast<const double *>(slot);
    return l;
  };
  lmm.AnalyzeGeneFeed(U, eval, UtW, Utx, feed, B, n);
}

// LM::AnalyzeBimbam, src/lm.cpp:382-503, over the same threaded reader (lm.file_geno, lm.indicator_idv / _snp)
inline void AnalyzeBimbam(LM &lm, const Matrix *W, const Vector *y) {
  const size_t ni_total = lm.indicator_idv.size(), n = W->size1;
  BimbamReader rd(lm.file_geno, ni_total);
  if (!rd.ok()) throw std::runtime_error("error reading genotype file");
  const size_t B = bimbam_block_rows(n, LMM_BATCH_SIZE);
  const std::vector<int> keep = lm.analysed_snps();
  BlockPrefetch pf(B * n * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= keep.size()) return 0;
    return rd.read_block(B, static_cast<double *>(slot), n, nullptr, &keep, lm.indicator_idv.data());
  });
  LMM::RowFeeder feed = [&](const double *&X) -> size_t {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) throw std::runtime_error("Problem reading geno file (not enough genotypes in line)");
    X = static_cast<const double *>(slot);
    return l;
  };
  lm.AnalyzeFeed(W, y, feed, B, n);
}

// ReadFile_kin (k_mode == 1), src/gemma_io.cpp:1186-1243, on the thread pool: the same dense ni_total x ni_total text,
// rows and columns of non-analysed individuals dropped while parsing, straight into G (the serial twin is
// gemma_host.hpp's ReadFile_kin; at n = 20 000 the file holds 4e8 numbers)
inline void ReadFile_kin_threaded(const std::string &file_kin, std::vector<int> &indicator_idv, bool &error, Matrix *G) {
  const size_t ni_total = indicator_idv.size();
  BimbamReader rd(file_kin, ni_total, 0, 0, true);
  if (!rd.ok()) {
    std::cout << "error! fail to open kinship file: " << file_kin << std::endl;
    error = true;
    return;
  }
  size_t i_test = 0;
  while (i_test < G->size1) {
    const size_t l = rd.read_block(G->size1 - i_test, G->data + i_test * G->tda, G->tda, nullptr, &indicator_idv,
                                   indicator_idv.data());
    if (l == (size_t)-1) {
      std::cout << "number of columns in the kinship file does not match the number of individuals" << std::endl;
      error = true;
      return;
    }
    if (l == 0) break;
    i_test += l;
  }
  // whatever is left must be rows of non-analysed individuals, and the file must end with row ni_total
  std::vector<double> rest(G->size2 ? G->size2 : 1);
  while (rd.lines_read() < ni_total) {
    const size_t before = rd.lines_read();
    const size_t l = rd.read_block(1, rest.data(), rest.size(), nullptr, &indicator_idv, indicator_idv.data());
    if (l == (size_t)-1 || (l == 0 && rd.lines_read() == before)) break;
  }
  std::vector<double> extra(ni_total ? ni_total : 1);
  if (i_test != G->size1 || rd.lines_read() != ni_total || rd.read_block(1, extra.data(), extra.size()) != 0) {
    std::cout << "number of rows in the kinship file does not match the number of individuals." << std::endl;
    error = true;
  }
}

// ReadFile_kin with k_mode == 2 (`-km 2`), src/gemma_io.cpp:1244-1288: "id1 id2 value" triples over the .fam ids
// (mapID2num from ReadFile_fam); pairs with an unknown or non-analysed id are skipped, the matrix is filled symmetrically,
// a pair given twice with different values is an error
inline void ReadFile_kin_km2(const std::string &file_kin, const std::vector<int> &indicator_idv,
                             const std::map<std::string, int> &mapID2num, bool &error, Matrix *G) {
  TextFile infile(file_kin);
  if (!infile.ok()) {
    std::cout << "error! fail to open kinship file: " << file_kin << std::endl;
    error = true;
    return;
  }
  for (size_t i = 0; i < G->size1; ++i)
    for (size_t j = 0; j < G->size2; ++j) G->data[i * G->tda + j] = 0.0;
  std::vector<long> id2id(indicator_idv.size(), -1);
  long c = 0;
  for (size_t i = 0; i < indicator_idv.size(); ++i)
    if (indicator_idv[i] == 1) id2id[i] = c++;
  std::string line;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b[3], *e[3];
    for (int k = 0; k < 3; ++k)
      if (!detail::next_token(p, end, b[k], e[k])) {
        std::cout << "Parsing input file '" << file_kin << "' failed in function ReadFile_kin" << std::endl;
        error = true;
        return;
      }
    const std::map<std::string, int>::const_iterator i1 = mapID2num.find(std::string(b[0], e[0])),
                                                     i2 = mapID2num.find(std::string(b[1], e[1]));
    if (i1 == mapID2num.end() || i2 == mapID2num.end()) continue;
    const long r = id2id[(size_t)i1->second], q = id2id[(size_t)i2->second];
    if (r < 0 || q < 0) continue;
    const double d = parse_double(b[2], e[2]);
    const double have = G->data[(size_t)r * G->tda + (size_t)q];
    if (have != 0 && have != d) {
      std::cout << "error! redundant and unequal terms in the kinship file, for id1 = " << std::string(b[0], e[0])
                << " and id2 = " << std::string(b[1], e[1]) << std::endl;
      error = true;
      return;
    }
    G->data[(size_t)r * G->tda + (size_t)q] = d;
    G->data[(size_t)q * G->tda + (size_t)r] = d;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// -eigen artefacts and their readers
// ---------------------------------------------------------------------------------------------------------------
// `gemma -k K -eigen` (src/gemma.cpp:1779-1800): <out>.eigenU.txt and <out>.eigenD.txt through PARAM::WriteMatrix /
// WriteVector (src/param.cpp:1886-1935: precision(10), tab separated)
inline bool WriteEigen(const Matrix *U, const Vector *eval, const std::string &path_out, const std::string &file_out) {
  return WriteMatrix(U, path_out + "/" + file_out + ".eigenU.txt") &&
         WriteVector(eval, path_out + "/" + file_out + ".eigenD.txt");
}

// ReadFile_eigenU, src/gemma_io.cpp:1323-1369: n_row lines of n_col numbers; U must be n_row x n_col
inline void ReadFile_eigenU(const std::string &file_ku, bool &error, Matrix *U) {
  TextFile infile(file_ku);
  if (!infile.ok()) {
    std::cout << "error! fail to open the U file: " << file_ku << std::endl;
    error = true;
    return;
  }
  const size_t n_row = U->size1, n_col = U->size2;
  for (size_t i = 0; i < n_row; ++i)
    for (size_t j = 0; j < n_col; ++j) U->data[i * U->tda + j] = 0.0;
  std::string line;
  size_t i_row = 0;
  while (infile.getline(line)) {
    if (i_row == n_row) {
      std::cout << "error! number of rows in the U file is larger than expected." << std::endl;
      error = true;
      return;
    }
    size_t i_col = 0;
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    while (detail::next_token(p, end, b, e)) {
      if (i_col == n_col) {
        std::cout << "error! number of columns in the U file is larger than expected, for row = " << i_row << std::endl;
        error = true;
        return;
      }
      U->data[i_row * U->tda + i_col++] = parse_double(b, e);
    }
    i_row++;
  }
}

// ReadFile_eigenU on the thread pool (at n = 20 000 the file holds 4e8 numbers): the same doubles for a well-formed
// file; stricter on a malformed one -- the reference zero-fills rows / columns a short file lacks and only rejects a surplus
// (src/gemma_io.cpp:1338-1362), here both are errors
inline void ReadFile_eigenU_threaded(const std::string &file_ku, bool &error, Matrix *U) {
  BimbamReader rd(file_ku, U->size2, 0, 0, true);
  if (!rd.ok()) {
    std::cout << "error! fail to open the U file: " << file_ku << std::endl;
    error = true;
    return;
  }
  size_t i_row = 0;
  while (i_row < U->size1) {
    const size_t l = rd.read_block(U->size1 - i_row, U->data + i_row * U->tda, U->tda);
    if (l == (size_t)-1) {
      std::cout << "error! number of columns in the U file does not match, near row = " << i_row << std::endl;
      error = true;
      return;
    }
    if (l == 0) break;
    i_row += l;
  }
  std::vector<double> extra(U->size2 ? U->size2 : 1);
  if (i_row != U->size1 || rd.read_block(1, extra.data(), extra.size()) != 0) {
    std::cout << "error! number of rows in the U file does not match." << std::endl;
    error = true;
  }
}

// ReadFile_eigenD, src/gemma_io.cpp:1372-1416: one number per line
inline void ReadFile_eigenD(const std::string &file_kd, bool &error, Vector *eval) {
  TextFile infile(file_kd);
  if (!infile.ok()) {
    std::cout << "error! fail to open the D file: " << file_kd << std::endl;
    error = true;
    return;
  }
  const size_t n_row = eval->size;
  for (size_t i = 0; i < n_row; ++i) eval->data[i * eval->stride] = 0.0;
  std::string line;
  size_t i_row = 0;
  while (infile.getline(line)) {
    if (i_row == n_row) {
      std::cout << "error! number of rows in the D file is larger than expected." << std::endl;
      error = true;
      return;
    }
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    if (!detail::next_token(p, end, b, e)) {
      std::cout << "Parsing input file '" << file_kd << "' failed in function ReadFile_eigenD" << std::endl;
      error = true;
      return;
    }
    eval->data[i_row * eval->stride] = parse_double(b, e);
    if (detail::next_token(p, end, b, e)) {
      std::cout << "error! number of columns in the D file is larger than expected, for row = " << i_row << std::endl;
      error = true;
      return;
    }
    i_row++;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// <o>.log.txt -- the lines of GEMMA::WriteLog (src/gemma.cpp:3159-3590) that belong to this path, in its format
// ("## key = value", ostream default precision): the summary counts, the null-model estimates of the univariate LMM and
// the five timers (minutes), plus one line naming the device.  The null model's beta / se(beta) lines are not written by this
// log: gemma_hip_lmm_null returns the variance components only.  The covariate effects come from gemma_hip_lmm_null_panel
// (CalcLambdaNullPanel of gemma_host.hpp, T >= 1); tests/cpp/null_panel_file_driver.cpp prints them per phenotype.
// ---------------------------------------------------------------------------------------------------------------
struct RunLog {
  std::string command_line;
  int a_mode = 0; // 1-4, 9: -lmm; 21 / 22: -gk; 51-54: -lm (src/gemma.h:39-43)
  size_t ni_total = 0, ni_test = 0, n_cvt = 1, n_ph = 1, ns_total = 0, ns_test = 0;
  bool have_null = false;
  NullModel null;
  double time_total = 0, time_G = 0, time_eigen = 0, time_UtX = 0, time_opt = 0; // minutes

  bool Write(const std::string &path_out, const std::string &file_out) const {
    const std::string file_str = path_out + "/" + file_out + ".log.txt";
    std::ofstream outfile(file_str.c_str(), std::ofstream::out);
    if (!outfile) {
      std::cout << "error writing log file: " << file_str << std::endl;
      return false;
    }
    char name[256] = "no device";
    int n_cu = 0;
    size_t hbm = 0;
    gemma_hip_device_info(name, sizeof name, &n_cu, &hbm);
    outfile << "##" << std::endl;
    outfile << "## GEMMA path on HIP, C ABI version = " << gemma_hip_abi_version() << std::endl;
    outfile << "## device = " << name << ", " << n_cu << " CUs, " << (double)hbm / 1e9 << " GB" << std::endl;
    outfile << "##" << std::endl;
    outfile << "## Command Line Input = " << command_line << std::endl;
    outfile << "##" << std::endl;
    outfile << "## Summary Statistics:" << std::endl;
    outfile << "## number of total individuals = " << ni_total << std::endl;
    outfile << "## number of analyzed individuals = " << ni_test << std::endl;
    outfile << "## number of covariates = " << n_cvt << std::endl;
    outfile << "## number of phenotypes = " << n_ph << std::endl;
    outfile << "## number of total SNPs/var = " << ns_total << std::endl;
    outfile << "## number of analyzed SNPs/var = " << ns_test << std::endl;
    if (have_null) {
      outfile << "## REMLE log-likelihood in the null model = " << null.logl_remle_H0 << std::endl;
      outfile << "## MLE log-likelihood in the null model = " << null.logl_mle_H0 << std::endl;
      if (n_ph == 1) {
        outfile << "## pve estimate in the null model = " << null.pve_null << std::endl;
        outfile << "## se(pve) in the null model = " << null.pve_se_null << std::endl;
        outfile << "## vg estimate in the null model = " << null.vg_remle_null << std::endl;
        outfile << "## ve estimate in the null model = " << null.ve_remle_null << std::endl;
      }
    }
    outfile << "##" << std::endl;
    outfile << "## Computation Time:" << std::endl;
    outfile << "## total computation time = " << time_total << " min " << std::endl;
    outfile << "## computation time break down: " << std::endl;
    if (a_mode == 21 || a_mode == 22)
      outfile << "##      time on calculating relatedness matrix = " << time_G << " min " << std::endl;
    if ((a_mode >= 1 && a_mode <= 4) || a_mode == 9) {
      outfile << "##      time on eigen-decomposition = " << time_eigen << " min " << std::endl;
      outfile << "##      time on calculating UtX = " << time_UtX << " min " << std::endl;
    }
    if ((a_mode >= 1 && a_mode <= 4) || a_mode == 9 || (a_mode >= 51 && a_mode <= 54))
      outfile << "##      time on optimization = " << time_opt << " min " << std::endl;
    outfile << "##" << std::endl;
    return true;
  }
};

// ---------------------------------------------------------------------------------------------------------------
// MQS summary statistics: -gs (a_mode 25) and -vc 1 -beta (a_mode 61), src/gemma.cpp:1948-1999, :2102-2230
// ---------------------------------------------------------------------------------------------------------------
// class HEADER, src/gemma_io.h: 1-based column numbers, 0 = absent
struct HEADER {
  size_t rs_col, chr_col, pos_col, cm_col, a1_col, a0_col, z_col, beta_col, sebeta_col, chisq_col, p_col, n_col, nmis_col, nobs_col,
      ncase_col, ncontrol_col, af_col, var_col, ws_col, cor_col, coln;
  std::set<size_t> catc_col, catd_col;
};

// ReadHeader_io, src/gemma_io.cpp:2367-2629: every spelling of every column name; any other name is a category column
// (continuous when it ends in _c / _C).  The a1 / a0 sets are built one name short there (INC_ALLELE / DEC_ALLELE never match).
inline bool ReadHeader_io(const std::string &line, HEADER &header) {
  struct Names {
    size_t HEADER::*col;
    const char *what;
    std::vector<std::string> names;
  };
  static const std::vector<Names> table = {
      {&HEADER::rs_col, "rs", {"rs", "RS", "snp", "SNP", "snps", "SNPS", "snpid", "SNPID", "rsid", "RSID", "MarkerName"}},
      {&HEADER::chr_col, "chr", {"chr", "CHR"}},
      {&HEADER::pos_col, "pos", {"ps", "PS", "pos", "POS", "base_position", "BASE_POSITION", "bp", "BP"}},
      {&HEADER::cm_col, "cm", {"cm", "CM"}},
      {&HEADER::a1_col, "allele1", {"a1", "A1", "allele1", "ALLELE1", "Allele1"}},
      {&HEADER::a0_col, "allele0", {"a0", "A0", "allele0", "ALLELE0", "Allele0", "a2", "A2", "allele2", "ALLELE2", "Allele2"}},
      {&HEADER::z_col, "z", {"z", "Z", "z_score", "Z_SCORE", "zscore", "ZSCORE"}},
      {&HEADER::beta_col, "beta", {"beta", "BETA", "b", "B"}},
      {&HEADER::sebeta_col, "se_beta", {"se_beta", "SE_BETA", "se", "SE"}},
      {&HEADER::chisq_col, "z", {"chisq", "CHISQ", "chisquare", "CHISQUARE"}},
      {&HEADER::p_col, "p", {"p", "P", "pvalue", "PVALUE", "p-value", "P-VALUE"}},
      {&HEADER::n_col, "n_total", {"n", "N", "ntotal", "NTOTAL", "n_total", "N_TOTAL"}},
      {&HEADER::nmis_col, "n_mis", {"nmis", "NMIS", "n_mis", "N_MIS", "n_miss", "N_MISS"}},
      {&HEADER::nobs_col, "n_obs", {"nobs", "NOBS", "n_obs", "N_OBS"}},
      {&HEADER::ncase_col, "n_case", {"ncase", "NCASE", "n_case", "N_CASE"}},
      {&HEADER::ncontrol_col, "n_control", {"ncontrol", "NCONTROL", "n_control", "N_CONTROL"}},
      {&HEADER::ws_col, "window_size", {"window_size", "WINDOW_SIZE", "ws", "WS"}},
      {&HEADER::af_col, "af", {"af", "AF", "maf", "MAF", "f", "F", "allele_freq", "ALLELE_FREQ", "allele_frequency", "ALLELE_FREQUENCY",
                               "Freq.Allele1.HapMapCEU", "FreqAllele1HapMapCEU", "Freq1.Hapmap"}},
      {&HEADER::cor_col, "cor", {"cor", "COR", "r", "R"}}};
  header = HEADER();
  size_t n_error = 0;
  const char *p = line.data(), *end = p + line.size(), *b, *e;
  while (detail::next_token(p, end, b, e)) {
    const std::string type(b, e);
    bool named = false;
    for (size_t k = 0; k < table.size() && !named; ++k)
      if (std::find(table[k].names.begin(), table[k].names.end(), type) != table[k].names.end()) {
        named = true;
        if (header.*(table[k].col) == 0) header.*(table[k].col) = header.coln + 1;
        else {
          std::cout << "error! more than two " << table[k].what << " columns in the file." << std::endl;
          n_error++;
        }
      }
    if (!named) {
      const std::string cat = type.size() >= 2 ? type.substr(type.size() - 2, 2) : std::string();
      if (cat == "_c" || cat == "_C") header.catc_col.insert(header.coln + 1);
      else header.catd_col.insert(header.coln + 1);
    }
    header.coln++;
  }
  if (header.cor_col != 0 && header.cor_col != header.coln) {
    std::cout << "error! the cor column should be the last column." << std::endl;
    n_error++;
  }
  if (header.rs_col == 0) {
    if (header.chr_col != 0 && header.pos_col != 0) std::cout << "missing an rs column. rs id will be replaced by chr:pos" << std::endl;
    else {
      std::cout << "error! missing an rs column." << std::endl;
      n_error++;
    }
  }
  return n_error == 0;
}

// ReadFile_cat, src/gemma_io.cpp:2634-2718 (`-cat`): the first category column that holds 1 names the SNP's category; a SNP with
// 0 everywhere is in no category and leaves the analysis
inline bool ReadFile_cat(const std::string &file_cat, std::map<std::string, size_t> &mapRS2cat, size_t &n_vc) {
  mapRS2cat.clear();
  TextFile infile(file_cat);
  if (!infile.ok()) {
    std::cout << "error! fail to open category file: " << file_cat << std::endl;
    return false;
  }
  std::string line, rs, chr, pos;
  HEADER header;
  infile.getline(line);
  ReadHeader_io(line, header);
  n_vc = header.coln;
  const size_t named[6] = {header.rs_col, header.chr_col, header.pos_col, header.cm_col, header.a1_col, header.a0_col};
  for (size_t k = 0; k < 6; ++k)
    if (named[k] != 0) n_vc--;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    size_t i_cat = 0;
    for (size_t i = 0; i < header.coln; i++) {
      if (!detail::next_token(p, end, b, e)) throw std::runtime_error("Parsing input file '" + file_cat + "' failed");
      const std::string tok(b, e);
      if (header.rs_col == i + 1) rs = tok;
      else if (header.chr_col == i + 1) chr = tok;
      else if (header.pos_col == i + 1) pos = tok;
      else if (header.cm_col == i + 1 || header.a1_col == i + 1 || header.a0_col == i + 1) {
      } else if (atoi(tok.c_str()) == 1 || atoi(tok.c_str()) == 0) {
        if (i_cat == 0 && header.rs_col == 0) rs = chr + ":" + pos;
        if (atoi(tok.c_str()) == 1 && mapRS2cat.count(rs) == 0) mapRS2cat[rs] = i_cat;
        i_cat++;
      }
    }
  }
  return true;
}

// ReadFile_snps_header, src/gemma_io.cpp:181-250: the SNP ids of a file with a header line (rs column, else chr:pos)
inline bool ReadFile_snps_header(const std::string &file_snps, std::set<std::string> &setSnps) {
  setSnps.clear();
  TextFile infile(file_snps);
  if (!infile.ok()) {
    std::cout << "error! fail to open snps file: " << file_snps << std::endl;
    return false;
  }
  std::string line, rs, chr, pos;
  HEADER header;
  infile.getline(line);
  ReadHeader_io(line, header);
  if (header.rs_col == 0 && (header.chr_col == 0 || header.pos_col == 0)) std::cout << "missing rs id in the hearder" << std::endl;
  while (infile.getline(line)) {
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    bool any = false;
    for (size_t i = 0; i < header.coln && detail::next_token(p, end, b, e); i++) {
      any = true;
      if (header.rs_col == i + 1) rs.assign(b, e);
      if (header.chr_col == i + 1) chr.assign(b, e);
      if (header.pos_col == i + 1) pos.assign(b, e);
    }
    if (!any) continue;
    if (header.rs_col == 0) rs = chr + ":" + pos;
    setSnps.insert(rs);
  }
  return true;
}

// gsl_cdf_chisq_Qinv(p, 1) = (Phi^-1(p / 2))^2: Acklam's rational approximation of Phi^-1 and one Halley step on erfc
inline double chisq1_Qinv(double pvalue) {
  const double p = pvalue / 2;
  if (p <= 0.0) return std::numeric_limits<double>::infinity();
  if (p >= 1.0) return std::numeric_limits<double>::infinity();
  static const double a[6] = {-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02,
                              -3.066479806614716e+01, 2.506628277459239e+00};
  static const double b[5] = {-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01,
                              -1.328068155288572e+01};
  static const double c[6] = {-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00,
                              4.374664141464968e+00, 2.938163982698783e+00};
  static const double d[4] = {7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00};
  double x;
  if (p < 0.02425) {
    const double q = std::sqrt(-2 * std::log(p));
    x = (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
  } else if (p > 1 - 0.02425) {
    const double q = std::sqrt(-2 * std::log(1 - p));
    x = -(((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1);
  } else {
    const double q = p - 0.5, r = q * q;
    x = (((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
        (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1);
  }
  const double er = 0.5 * std::erfc(-x / std::sqrt(2.0)) - p;
  const double u = er * std::sqrt(2 * 3.14159265358979323846) * std::exp(x * x / 2);
  x = x - u / (1 + x * u / 2);
  return x * x;
}

// ReadFile_beta, the z-score overload, src/gemma_io.cpp:3363-3551: z^2 from z, else beta / se, else chisq, else the p-value
inline void ReadFile_beta(const std::string &file_beta, const std::map<std::string, size_t> &mapRS2cat,
                          const std::map<std::string, double> &mapRS2wA, std::vector<size_t> &vec_cat, std::vector<size_t> &vec_ni,
                          std::vector<double> &vec_weight, std::vector<double> &vec_z2, size_t &ni_total, size_t &ns_total,
                          size_t &ns_test) {
  vec_cat.clear();
  vec_ni.clear();
  vec_weight.clear();
  vec_z2.clear();
  ni_total = ns_total = ns_test = 0;
  TextFile infile(file_beta);
  if (!infile.ok()) {
    std::cout << "error! fail to open beta file: " << file_beta << std::endl;
    return;
  }
  std::string line, rs, chr, pos;
  HEADER header;
  infile.getline(line);
  ReadHeader_io(line, header);
  if (header.n_col == 0) {
    if ((header.nobs_col == 0 && header.nmis_col == 0) && (header.ncase_col == 0 && header.ncontrol_col == 0))
      std::cout << "error! missing sample size in the beta file." << std::endl;
    else std::cout << "total sample size will be replaced by obs/mis sample size." << std::endl;
  }
  if (header.z_col == 0 && (header.beta_col == 0 || header.sebeta_col == 0) && header.chisq_col == 0 && header.p_col == 0)
    std::cout << "error! missing z scores in the beta file." << std::endl;
  while (infile.getline(line)) {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    double z = 0, beta = 0, se_beta = 0, chisq = 0, pvalue = 0, zsquare = 0;
    size_t n_total = 0, n_mis = 0, n_obs = 0, n_case = 0, n_control = 0;
    for (size_t i = 0; i < header.coln; i++) {
      if (!detail::next_token(p, end, b, e)) throw std::runtime_error("Parsing input file '" + file_beta + "' failed");
      const std::string tok(b, e);
      if (header.rs_col == i + 1) rs = tok;
      if (header.chr_col == i + 1) chr = tok;
      if (header.pos_col == i + 1) pos = tok;
      if (header.z_col == i + 1) z = atof(tok.c_str());
      if (header.beta_col == i + 1) beta = atof(tok.c_str());
      if (header.sebeta_col == i + 1) se_beta = atof(tok.c_str());
      if (header.chisq_col == i + 1) chisq = atof(tok.c_str());
      if (header.p_col == i + 1) pvalue = atof(tok.c_str());
      if (header.n_col == i + 1) n_total = (size_t)atoi(tok.c_str());
      if (header.nmis_col == i + 1) n_mis = (size_t)atoi(tok.c_str());
      if (header.nobs_col == i + 1) n_obs = (size_t)atoi(tok.c_str());
      if (header.ncase_col == i + 1) n_case = (size_t)atoi(tok.c_str());
      if (header.ncontrol_col == i + 1) n_control = (size_t)atoi(tok.c_str());
    }
    if (header.rs_col == 0) rs = chr + ":" + pos;
    if (header.n_col == 0) n_total = (header.nmis_col != 0 && header.nobs_col != 0) ? n_mis + n_obs : n_case + n_control;
    if (header.z_col != 0) zsquare = z * z;
    else if (header.beta_col != 0 && header.sebeta_col != 0) {
      z = beta / se_beta;
      zsquare = z * z;
    } else if (header.chisq_col != 0) zsquare = chisq;
    else if (header.p_col != 0) zsquare = chisq1_Qinv(pvalue);
    else zsquare = 0;
    if ((mapRS2wA.size() == 0 || mapRS2wA.count(rs) != 0) && (mapRS2cat.size() == 0 || mapRS2cat.count(rs) != 0) && zsquare != 0) {
      vec_cat.push_back(mapRS2cat.size() != 0 ? mapRS2cat.at(rs) : 0);
      vec_ni.push_back(n_total);
      vec_weight.push_back(mapRS2wA.size() == 0 ? 1 : mapRS2wA.at(rs));
      vec_z2.push_back(zsquare);
      ni_total = std::max(ni_total, n_total);
      ns_test++;
    }
    ns_total++;
  }
}

// PARAM::ObtainWeight without -wsnp / -wcat, src/param.cpp:2214-2296: weight 1 for every analysed SNP that the beta file (when one
// is given) and the category file (when one is given) both know
inline void ObtainWeight(const std::vector<SNPINFO> &snpInfo, const std::vector<int> &indicator_snp,
                         const std::set<std::string> &setSnps_beta, const std::map<std::string, size_t> &mapRS2cat,
                         std::map<std::string, double> &mapRS2wK) {
  mapRS2wK.clear();
  for (size_t i = 0; i < snpInfo.size(); i++) {
    if (indicator_snp[i] == 0) continue;
    const std::string &rs = snpInfo[i].rs_number;
    if ((setSnps_beta.size() == 0 || setSnps_beta.count(rs) != 0) && (mapRS2cat.size() == 0 || mapRS2cat.count(rs) != 0)) mapRS2wK[rs] = 1;
  }
}

// PARAM::UpdateSNP, src/param.cpp:2420-2453
inline void UpdateSNP(const std::vector<SNPINFO> &snpInfo, std::vector<int> &indicator_snp, const std::map<std::string, double> &mapRS2wA) {
  for (size_t i = 0; i < snpInfo.size(); i++)
    if (indicator_snp[i] != 0 && mapRS2wA.count(snpInfo[i].rs_number) == 0) indicator_snp[i] = 0;
}

// Calcq, src/gemma_io.cpp:3716-3870: q per category and the block jackknife of its variance over n_block blocks of SNPs, with
// the reference's branch structure (the `!= 0` tests that stand for "this block holds SNPs of the category", the halving of the
// off-diagonal elements that were added twice)
inline void Calcq(const size_t n_block, const std::vector<size_t> &vec_cat, const std::vector<size_t> &vec_ni,
                  const std::vector<double> &vec_weight, const std::vector<double> &vec_z2, Matrix *Vq, Vector *q, Vector *s) {
  const size_t nq = q->size;
  for (size_t i = 0; i < Vq->size1; i++)
    for (size_t j = 0; j < Vq->size2; j++) Vq->data[i * Vq->tda + j] = 0;
  for (size_t i = 0; i < nq; i++) q->data[i * q->stride] = 0;
  for (size_t i = 0; i < s->size; i++) s->data[i * s->stride] = 0;
  std::vector<double> vec_q(nq, 0.0), vec_s(nq, 0.0), n_snps(nq, 0.0);
  std::vector<std::vector<double>> mat_q(n_block, vec_q), mat_s(n_block, vec_s);
  for (size_t i = 0; i < vec_cat.size(); i++) {
    const size_t cat = vec_cat[i];
    vec_q[cat] += (vec_z2[i] - 1.0) * vec_weight[i] / (double)vec_ni[i];
    vec_s[cat] += vec_weight[i];
    n_snps[cat]++;
  }
  for (size_t i = 0; i < nq; i++) {
    if (vec_s[i] != 0) q->data[i * q->stride] = vec_q[i] / vec_s[i];
    s->data[i * s->stride] = vec_s[i];
  }
  size_t t = 0, b = 0, n_snp = 0;
  double d, m, n;
  for (size_t l = 0; l < nq; l++) {
    n_snp = (size_t)std::floor(n_snps[l] / n_block);
    t = 0;
    b = 0;
    if (n_snp == 0) continue;
    for (size_t i = 0; i < n_block; i++)
      for (size_t j = 0; j < nq; j++) {
        mat_q[i][j] = 0;
        mat_s[i][j] = 0;
      }
    for (size_t i = 0; i < vec_cat.size(); i++) {
      const size_t cat = vec_cat[i];
      mat_q[b][cat] += (vec_z2[i] - 1.0) * vec_weight[i];
      mat_s[b][cat] += vec_weight[i];
      if (cat == l) {
        if (b < n_block - 1) {
          if (t < n_snp - 1) t++;
          else {
            b++;
            t = 0;
          }
        } else t++;
      }
    }
    for (size_t i = 0; i < nq; i++) {
      m = 0;
      n = 0;
      for (size_t k = 0; k < n_block; k++)
        if (mat_s[k][i] != 0 && vec_s[i] != mat_s[k][i]) {
          d = (vec_q[i] - mat_q[k][i]) / (vec_s[i] - mat_s[k][i]);
          mat_q[k][i] = d;
          m += d;
          n++;
        }
      if (n != 0) m /= n;
      for (size_t k = 0; k < n_block; k++)
        if (mat_q[k][i] != 0) mat_q[k][i] -= m;
    }
    for (size_t i = 0; i < nq; i++) {
      d = 0;
      n = 0;
      for (size_t k = 0; k < n_block; k++)
        if (mat_q[k][l] != 0 && mat_q[k][i] != 0) {
          d += mat_q[k][l] * mat_q[k][i];
          n++;
        }
      if (n != 0) {
        d /= n;
        d *= n - 1;
      }
      d += Vq->data[i * Vq->tda + l];
      Vq->data[i * Vq->tda + l] = d;
      if (i != l) Vq->data[l * Vq->tda + i] = d;
    }
  }
  for (size_t i = 0; i < nq; i++)
    for (size_t j = i + 1; j < nq; j++) {
      d = Vq->data[i * Vq->tda + j];
      Vq->data[i * Vq->tda + j] = d / 2;
      Vq->data[j * Vq->tda + i] = d / 2;
    }
}

namespace detail {
// inverse of an m x m matrix by elimination with partial pivoting (LUDecomp + LUInvert on n_vc <= 8); false if singular
inline bool small_inverse(std::vector<double> &A, size_t m) {
  std::vector<double> I(m * m, 0.0);
  for (size_t i = 0; i < m; ++i) I[i * m + i] = 1.0;
  for (size_t k = 0; k < m; ++k) {
    size_t p = k;
    for (size_t i = k + 1; i < m; ++i)
      if (std::fabs(A[i * m + k]) > std::fabs(A[p * m + k])) p = i;
    if (A[p * m + k] == 0.0) return false;
    for (size_t j = 0; j < m && p != k; ++j) {
      std::swap(A[k * m + j], A[p * m + j]);
      std::swap(I[k * m + j], I[p * m + j]);
    }
    const double d = 1.0 / A[k * m + k];
    for (size_t j = 0; j < m; ++j) {
      A[k * m + j] *= d;
      I[k * m + j] *= d;
    }
    for (size_t i = 0; i < m; ++i) {
      const double f = A[i * m + k];
      if (i == k || f == 0.0) continue;
      for (size_t j = 0; j < m; ++j) {
        A[i * m + j] -= f * A[k * m + j];
        I[i * m + j] -= f * I[k * m + j];
      }
    }
  }
  A = I;
  return true;
}
inline std::vector<double> matmul(const std::vector<double> &A, const std::vector<double> &B, size_t m, bool transB = false) {
  std::vector<double> Cm(m * m, 0.0);
  for (size_t i = 0; i < m; ++i)
    for (size_t j = 0; j < m; ++j)
      for (size_t k = 0; k < m; ++k) Cm[i * m + j] += A[i * m + k] * (transB ? B[j * m + k] : B[k * m + j]);
  return Cm;
}
} // namespace detail

// CalcVCss, src/vc.cpp:1309-1500: pve = S^-1 q, its variance from Svar and Vq / df^2, the per-SNP sigma2 and the enrichment
inline void CalcVCss(const Matrix *Vq, const Matrix *S_mat, const Matrix *Svar_mat, const Vector *q_vec, const Vector *s_vec,
                     const double df, std::vector<double> &v_pve, std::vector<double> &v_se_pve, double &pve_total,
                     double &se_pve_total, std::vector<double> &v_sigma2, std::vector<double> &v_se_sigma2,
                     std::vector<double> &v_enrich, std::vector<double> &v_se_enrich) {
  const size_t n_vc = S_mat->size1;
  std::vector<double> Si(n_vc * n_vc), Var(n_vc * n_vc, 0.0), pve(n_vc, 0.0), sigma2persnp(n_vc), se_pve(n_vc), se_sigma2persnp(n_vc);
  for (size_t i = 0; i < n_vc; i++)
    for (size_t j = 0; j < n_vc; j++) Si[i * n_vc + j] = S_mat->data[i * S_mat->tda + j];
  if (!detail::small_inverse(Si, n_vc)) throw std::runtime_error("CalcVCss: S is singular");
  auto qv = [&](size_t i) { return q_vec->data[i * q_vec->stride]; };
  auto sv = [&](size_t i) { return s_vec->data[i * s_vec->stride]; };
  for (size_t i = 0; i < n_vc; i++) {
    for (size_t j = 0; j < n_vc; j++) pve[i] += Si[i * n_vc + j] * qv(j);
    sigma2persnp[i] = pve[i] / sv(i);
  }
  for (size_t i = 0; i < n_vc; i++)
    for (size_t j = i; j < n_vc; j++) {
      double d = Svar_mat->data[i * Svar_mat->tda + j];
      d *= pve[i] * pve[j];
      d += Vq->data[i * Vq->tda + j] * (1.0 / (df * df));
      Var[i * n_vc + j] = Var[j * n_vc + i] = d;
    }
  Var = detail::matmul(detail::matmul(Si, Var, n_vc), Si, n_vc);
  for (size_t i = 0; i < n_vc; i++) {
    const double d = std::sqrt(Var[i * n_vc + i]);
    se_pve[i] = d;
    se_sigma2persnp[i] = d / sv(i);
  }
  pve_total = 0;
  se_pve_total = 0;
  for (size_t i = 0; i < n_vc; i++) {
    pve_total += pve[i];
    for (size_t j = 0; j < n_vc; j++) se_pve_total += Var[i * n_vc + j];
  }
  se_pve_total = std::sqrt(se_pve_total);
  double s_pve = 0, s_snp = 0;
  for (size_t i = 0; i < n_vc; i++) {
    s_pve += pve[i];
    s_snp += sv(i);
  }
  std::vector<double> T(n_vc * n_vc);
  for (size_t i = 0; i < n_vc; i++) {
    const double d = pve[i] / s_pve, d1 = sv(i);
    for (size_t j = 0; j < n_vc; j++) T[i * n_vc + j] = (i == j ? (1 - d) : -1 * d) / d1 * s_snp / s_pve;
  }
  const std::vector<double> VarEnrich = detail::matmul(detail::matmul(T, Var, n_vc), T, n_vc, true);
  v_pve.clear();
  v_se_pve.clear();
  v_sigma2.clear();
  v_se_sigma2.clear();
  v_enrich.clear();
  v_se_enrich.clear();
  for (size_t i = 0; i < n_vc; i++) {
    v_pve.push_back(pve[i]);
    v_se_pve.push_back(se_pve[i]);
    v_sigma2.push_back(sigma2persnp[i]);
    v_se_sigma2.push_back(se_sigma2persnp[i]);
    v_enrich.push_back(sigma2persnp[i] * (s_snp / s_pve));
    v_se_enrich.push_back(std::sqrt(VarEnrich[i * n_vc + i]));
  }
}

// PARAM::CalcS on a PLINK set, src/param.cpp:1717-1812 with PlinkKin(..., mapRS2weight, mapRS2cat, ...), src/gemma_io.cpp:2947-3170:
// the .bed rows of the SNPs with indicator_snp != 0 go to the device in blocks with their category (-1: no category or no
// weight) and weight; S (2 n_vc x n_vc: S on top of Svar) and ns (n_vc) come back.  slot 0: K, and A = K (empty mapRS2wA);
// slot 1: A beside the K of the previous call, from 0; slot 2: the same with A starting from that K, centred and scaled, which
// is what the reference's second call computes (src/gemma.cpp:2198: PlinkKin adds to the A the first call left).
inline bool CalcS(const std::string &file_bed, const std::vector<int> &indicator_idv, const std::vector<int> &indicator_snp,
                  const std::map<std::string, double> &mapRS2weight, const std::map<std::string, size_t> &mapRS2cat,
                  const std::vector<SNPINFO> &snpInfo, const Matrix *W, const size_t n_vc, Matrix *S, Vector *ns, const int slot = 0) {
  std::ifstream infile(file_bed.c_str(), std::ios::binary);
  if (!infile) {
    std::cout << "error reading bed file:" << file_bed << std::endl;
    return false;
  }
  if (W->tda != W->size2 || S->tda != S->size2 || S->size1 != 2 * n_vc || S->size2 != n_vc || ns->size < n_vc || ns->stride != 1)
    throw HipError(GEMMA_HIP_EINVAL, "CalcS: contiguous W, S (2 n_vc x n_vc) and ns (n_vc)");
  const size_t ni_total = indicator_idv.size(), n_bit = (ni_total + 3) / 4;
  std::vector<int> cat;
  std::vector<double> weight;
  for (size_t t = 0; t < indicator_snp.size(); ++t) {
    if (indicator_snp[t] == 0) continue;
    const std::string &rs = snpInfo[t].rs_number;
    int c = 0;
    double w = 1.0;
    if (mapRS2weight.size() != 0) {
      if (mapRS2weight.count(rs) == 0) c = -1;
      else w = mapRS2weight.at(rs);
    }
    if (c == 0 && !(n_vc == 1 || mapRS2cat.size() == 0)) c = mapRS2cat.count(rs) != 0 ? (int)mapRS2cat.at(rs) : -1;
    cat.push_back(c);
    weight.push_back(w);
  }
  enforce_hip(gemma_hip_mqs_begin(ni_total, indicator_idv.data(), n_vc, W->data, W->size2, slot), "CalcS");
  const size_t B = io_block_rows(K_BATCH_SIZE);
  std::vector<unsigned char> block(B * n_bit);
  size_t t_next = 0, done = 0;
  for (;;) {
    const size_t l = read_bed_rows(infile, indicator_snp, t_next, n_bit, block.data(), B);
    if (l == (size_t)-1) {
      std::cout << "error reading bed file:" << file_bed << " (truncated)" << std::endl;
      return false;
    }
    if (l == 0) break;
    enforce_hip(gemma_hip_mqs_add(GEMMA_GENO_PLINK_2BIT, block.data(), l, n_bit, cat.data() + done, weight.data() + done), "CalcS");
    done += l;
  }
  enforce_hip(gemma_hip_mqs_end(S->data, ns->data), "CalcS");
  return true;
}

// The four files of src/gemma.cpp:2217-2220 (-gs: S and size only), precision(10): prefix.S.txt, .Vq.txt, .q.txt, .size.txt;
// size = ns per category followed by ni_test.  Vq / q may be NULL.
inline bool WriteMQS(const std::string &prefix, const Matrix *S, const Matrix *Vq, const Vector *q, const Vector *size) {
  bool ok = WriteMatrix(S, prefix + ".S.txt") && WriteVector(size, prefix + ".size.txt");
  if (Vq) ok = ok && WriteMatrix(Vq, prefix + ".Vq.txt");
  if (q) ok = ok && WriteVector(q, prefix + ".q.txt");
  return ok;
}

// ---------------------------------------------------------------------------------------------------------------
// MQS confidence intervals (-ci 1 / -ci 2, a_mode 66 / 67, src/gemma.cpp:2400-2554) and the LDSC-weighted second round of
// -vc 2 -beta (a_mode 62, src/gemma.cpp:2182-2212)
// ---------------------------------------------------------------------------------------------------------------
// ReadFile_wsnp, the -wcat overload, src/gemma_io.cpp:3281-3353: per SNP its n_vc weights, one per column that names nothing else
inline bool ReadFile_wsnp(const std::string &file_wcat, const size_t n_vc, std::map<std::string, std::vector<double>> &mapRS2wvector) {
  mapRS2wvector.clear();
  TextFile infile(file_wcat);
  if (!infile.ok()) {
    std::cout << "error! fail to open snp weight file: " << file_wcat << std::endl;
    return false;
  }
  std::vector<double> weight(n_vc, 0.0);
  std::string line, rs, chr, pos;
  HEADER header;
  infile.getline(line);
  ReadHeader_io(line, header);
  while (infile.getline(line)) {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    size_t t = 0;
    for (size_t i = 0; i < header.coln; i++) {
      if (!detail::next_token(p, end, b, e)) throw std::runtime_error("Parsing input file '" + file_wcat + "' failed");
      const std::string tok(b, e);
      if (header.rs_col == i + 1) rs = tok;
      else if (header.chr_col == i + 1) chr = tok;
      else if (header.pos_col == i + 1) pos = tok;
      else if (header.cm_col == i + 1 || header.a1_col == i + 1 || header.a0_col == i + 1) continue;
      else {
        if (t < n_vc) weight[t] = atof(tok.c_str());
        t++;
      }
    }
    if (t != n_vc) {
      std::cout << "error! Number of columns in the wcat file does not match that of cat file.";
      return false;
    }
    if (header.rs_col == 0) rs = chr + ":" + pos;
    mapRS2wvector[rs] = weight;
  }
  return true;
}

// PARAM::ObtainWeight with the mapRS2wcat membership test of src/param.cpp:2233-2236 (still without -wsnp)
inline void ObtainWeight(const std::vector<SNPINFO> &snpInfo, const std::vector<int> &indicator_snp,
                         const std::set<std::string> &setSnps_beta, const std::map<std::string, std::vector<double>> &mapRS2wcat,
                         const std::map<std::string, size_t> &mapRS2cat, std::map<std::string, double> &mapRS2wK) {
  mapRS2wK.clear();
  for (size_t i = 0; i < snpInfo.size(); i++) {
    if (indicator_snp[i] == 0) continue;
    const std::string &rs = snpInfo[i].rs_number;
    if ((setSnps_beta.size() == 0 || setSnps_beta.count(rs) != 0) && (mapRS2wcat.size() == 0 || mapRS2wcat.count(rs) != 0) &&
        (mapRS2cat.size() == 0 || mapRS2cat.count(rs) != 0))
      mapRS2wK[rs] = 1;
  }
}

// PARAM::UpdateWeight, src/param.cpp:2300-2349: pve_flag 0 leaves pve as it is (-ci 2), 1 clamps it to [0, 1] (-vc 2)
inline void UpdateWeight(const size_t pve_flag, const std::map<std::string, double> &mapRS2wK, const size_t ni_test, const Vector *ns,
                         const std::vector<double> &v_pve, const std::map<std::string, std::vector<double>> &mapRS2wcat,
                         const std::map<std::string, size_t> &mapRS2cat, std::map<std::string, double> &mapRS2wA) {
  const size_t n_vc = v_pve.size();
  double d;
  std::vector<double> wsum(n_vc, 0.0), wcount(n_vc, 0.0);
  const std::vector<double> none(n_vc, 0.0);
  for (std::map<std::string, double>::const_iterator it = mapRS2wK.begin(); it != mapRS2wK.end(); ++it) {
    const std::vector<double> &wc = mapRS2wcat.count(it->first) != 0 ? mapRS2wcat.at(it->first) : none;
    d = 1;
    for (size_t i = 0; i < n_vc; i++) {
      if (v_pve[i] >= 1 && pve_flag == 1) {
        d += (double)ni_test / ns->data[i * ns->stride] * wc[i];
      } else if (v_pve[i] <= 0 && pve_flag == 1) {
        d += 0;
      } else {
        d += (double)ni_test / ns->data[i * ns->stride] * wc[i] * v_pve[i];
      }
    }
    mapRS2wA[it->first] = 1 / (d * d);
    const size_t k = mapRS2cat.size() == 0 ? 0 : mapRS2cat.at(it->first);
    wsum[k] += mapRS2wA[it->first];
    wcount[k]++;
  }
  for (size_t i = 0; i < n_vc; i++) wsum[i] /= wcount[i];
  for (std::map<std::string, double>::iterator it = mapRS2wA.begin(); it != mapRS2wA.end(); ++it)
    it->second /= wsum[mapRS2cat.size() == 0 ? 0 : mapRS2cat.at(it->first)];
}

// ReadFile_beta, the (mapRS2wA, mapRS2A1, mapRS2z) overload, src/gemma_io.cpp:3553-3714: the signed z (from z, else beta / se, else
// 0) and the allele it refers to; without an allele column a1 stays empty
inline void ReadFile_beta(const std::string &file_beta, const std::map<std::string, double> &mapRS2wA,
                          std::map<std::string, std::string> &mapRS2A1, std::map<std::string, double> &mapRS2z) {
  mapRS2A1.clear();
  mapRS2z.clear();
  TextFile infile(file_beta);
  if (!infile.ok()) {
    std::cout << "error! fail to open beta file: " << file_beta << std::endl;
    return;
  }
  std::string line, rs, chr, pos, a1;
  HEADER header;
  infile.getline(line);
  ReadHeader_io(line, header);
  if (header.z_col == 0 && (header.beta_col == 0 || header.sebeta_col == 0)) std::cout << "error! missing z scores in the beta file." << std::endl;
  while (infile.getline(line)) {
    if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
    const char *p = line.data(), *end = p + line.size(), *b, *e;
    double z = 0, beta = 0, se_beta = 0;
    for (size_t i = 0; i < header.coln; i++) {
      if (!detail::next_token(p, end, b, e)) throw std::runtime_error("Parsing input file '" + file_beta + "' failed");
      const std::string tok(b, e);
      if (header.rs_col == i + 1) rs = tok;
      if (header.chr_col == i + 1) chr = tok;
      if (header.pos_col == i + 1) pos = tok;
      if (header.a1_col == i + 1) a1 = tok;
      if (header.z_col == i + 1) z = atof(tok.c_str());
      if (header.beta_col == i + 1) beta = atof(tok.c_str());
      if (header.sebeta_col == i + 1) se_beta = atof(tok.c_str());
    }
    if (header.rs_col == 0) rs = chr + ":" + pos;
    if (header.z_col != 0) {
    } else if (header.beta_col != 0 && header.sebeta_col != 0) {
      z = beta / se_beta;
    } else {
      z = 0;
    }
    if (mapRS2wA.size() == 0 || mapRS2wA.count(rs) != 0) {
      mapRS2z[rs] = z;
      mapRS2A1[rs] = a1;
    }
  }
}

// PARAM::UpdateSNPnZ, src/param.cpp:2353-2416, single-file branch: w, z (negated when the beta file's allele is not the minor
// allele of the genotype file) and vec_cat of the SNPs that have a weight, in file order; the others leave indicator_snp
inline void UpdateSNPnZ(const std::vector<SNPINFO> &snpInfo, std::vector<int> &indicator_snp, const std::map<std::string, double> &mapRS2wA,
                        const std::map<std::string, std::string> &mapRS2A1, const std::map<std::string, double> &mapRS2z,
                        const std::map<std::string, size_t> &mapRS2cat, std::vector<double> &w, std::vector<double> &z,
                        std::vector<size_t> &vec_cat) {
  w.clear();
  z.clear();
  vec_cat.clear();
  for (size_t i = 0; i < snpInfo.size(); i++) {
    if (indicator_snp[i] == 0) continue;
    const std::string &rs = snpInfo[i].rs_number, &a1 = snpInfo[i].a_minor;
    if (mapRS2wA.count(rs) != 0) {
      if (a1 == mapRS2A1.at(rs)) z.push_back(mapRS2z.at(rs));
      else z.push_back(-1 * mapRS2z.at(rs));
      vec_cat.push_back(mapRS2cat.size() == 0 ? 0 : mapRS2cat.at(rs));
      w.push_back(mapRS2wA.at(rs));
    } else {
      indicator_snp[i] = 0;
    }
  }
}

namespace detail {
inline bool read_numbers(const std::string &file, std::vector<double> &v) {
  std::ifstream f(file.c_str());
  if (!f) {
    std::cout << "error! fail to open file: " << file << std::endl;
    return false;
  }
  v.clear();
  double d;
  while (f >> d) v.push_back(d);
  return true;
}
} // namespace detail

// ReadFile_ref, src/gemma_io.cpp:3987-4009: prefix.S.txt (S on top of Svar) and prefix.size.txt (ns per category, then ni)
inline bool ReadFile_ref(const std::string &file_ref, std::vector<double> &S_mat, std::vector<double> &Svar_mat, std::vector<double> &s_vec,
                         size_t &ni) {
  std::vector<double> s, S;
  if (!detail::read_numbers(file_ref + ".size.txt", s) || !detail::read_numbers(file_ref + ".S.txt", S) || s.size() < 2) return false;
  const size_t n_vc = s.size() - 1;
  if (S.size() != 2 * n_vc * n_vc) return false;
  S_mat.assign(S.begin(), S.begin() + n_vc * n_vc);
  Svar_mat.assign(S.begin() + n_vc * n_vc, S.end());
  s_vec.assign(s.begin(), s.begin() + n_vc);
  ni = (size_t)s[n_vc];
  return true;
}

// ReadFile_study, src/gemma_io.cpp:3961-3985: prefix.Vq.txt, prefix.q.txt and prefix.size.txt
inline bool ReadFile_study(const std::string &file_study, std::vector<double> &Vq_mat, std::vector<double> &q_vec, std::vector<double> &s_vec,
                           size_t &ni) {
  std::vector<double> s;
  if (!detail::read_numbers(file_study + ".size.txt", s) || s.size() < 2) return false;
  const size_t n_vc = s.size() - 1;
  if (!detail::read_numbers(file_study + ".Vq.txt", Vq_mat) || !detail::read_numbers(file_study + ".q.txt", q_vec) ||
      Vq_mat.size() != n_vc * n_vc || q_vec.size() != n_vc)
    return false;
  s_vec.assign(s.begin(), s.begin() + n_vc);
  ni = (size_t)s[n_vc];
  return true;
}

// PlinkXwz, src/vc.cpp:2314-2437, for Xz (w = 1) and XWz in ONE pass over the file: the .bed rows of the SNPs with
// indicator_snp != 0 go to gemma_hip_ci_xwz in blocks.  w == NULL: -ci 1 (XWz = Xz).  Starts the session; Xz, XWz: ni_test x n_vc.
inline bool PlinkXwz(const std::string &file_bed, const std::vector<int> &indicator_idv, const std::vector<int> &indicator_snp,
                     const std::vector<size_t> &vec_cat, const std::vector<double> *w, const std::vector<double> &z, const size_t n_vc,
                     Matrix *Xz, Matrix *XWz, size_t *n_skipped = nullptr) {
  std::ifstream infile(file_bed.c_str(), std::ios::binary);
  if (!infile) {
    std::cout << "error reading bed file:" << file_bed << std::endl;
    return false;
  }
  if (Xz->tda != Xz->size2 || XWz->tda != XWz->size2 || Xz->size2 != n_vc || XWz->size2 != n_vc)
    throw HipError(GEMMA_HIP_EINVAL, "PlinkXwz: contiguous Xz and XWz (ni_test x n_vc)");
  const size_t ni_total = indicator_idv.size(), n_bit = (ni_total + 3) / 4;
  const std::vector<int> cat(vec_cat.begin(), vec_cat.end());
  enforce_hip(gemma_hip_ci_begin(ni_total, indicator_idv.data(), n_vc), "PlinkXwz");
  const size_t B = io_block_rows(LMM_BATCH_SIZE);
  std::vector<unsigned char> block(B * n_bit);
  size_t t_next = 0, done = 0, skipped = 0;
  if (n_skipped) *n_skipped = 0;
  for (;;) {
    const size_t l = read_bed_rows(infile, indicator_snp, t_next, n_bit, block.data(), B);
    if (l == (size_t)-1) {
      std::cout << "error reading bed file:" << file_bed << " (truncated)" << std::endl;
      return false;
    }
    if (l == 0) break;
    if (done + l > cat.size() || done + l > z.size()) throw HipError(GEMMA_HIP_EINVAL, "PlinkXwz: fewer z-scores than analysed SNPs");
    enforce_hip(gemma_hip_ci_xwz(GEMMA_GENO_PLINK_2BIT, block.data(), l, n_bit, cat.data() + done, z.data() + done,
                                 w ? w->data() + done : nullptr, &skipped), "PlinkXwz");
    if (n_skipped) *n_skipped += skipped;
    done += l;
  }
  enforce_hip(gemma_hip_ci_xwz_end(Xz->data, XWz->data), "PlinkXwz");
  return true;
}

// PlinkXtXwz, src/vc.cpp:2568-2688, after PlinkXwz (the finished XWz is on the device): XtXWz is ns_test x n_vc
inline bool PlinkXtXwz(const std::string &file_bed, const std::vector<int> &indicator_idv, const std::vector<int> &indicator_snp,
                       const size_t n_vc, Matrix *XtXWz) {
  std::ifstream infile(file_bed.c_str(), std::ios::binary);
  if (!infile) {
    std::cout << "error reading bed file:" << file_bed << std::endl;
    return false;
  }
  if (XtXWz->tda != n_vc || XtXWz->size2 != n_vc) throw HipError(GEMMA_HIP_EINVAL, "PlinkXtXwz: contiguous XtXWz (ns_test x n_vc)");
  const size_t n_bit = (indicator_idv.size() + 3) / 4, B = io_block_rows(LMM_BATCH_SIZE);
  std::vector<unsigned char> block(B * n_bit);
  size_t t_next = 0, done = 0;
  for (;;) {
    const size_t l = read_bed_rows(infile, indicator_snp, t_next, n_bit, block.data(), B);
    if (l == (size_t)-1) {
      std::cout << "error reading bed file:" << file_bed << " (truncated)" << std::endl;
      return false;
    }
    if (l == 0) break;
    if (done + l > XtXWz->size1) throw HipError(GEMMA_HIP_EINVAL, "PlinkXtXwz: fewer rows of XtXWz than analysed SNPs");
    enforce_hip(gemma_hip_ci_xtxwz(GEMMA_GENO_PLINK_2BIT, block.data(), l, n_bit, XtXWz->data + done * n_vc), "PlinkXtXwz");
    done += l;
  }
  return true;
}

// BimbamXwz, src/vc.cpp:2225-2312, for Xz and XWz in ONE pass over the text file: the rows of the SNPs with indicator_snp != 0 over
// all ni_total individuals (NaN = NA) go to gemma_hip_ci_xwz in blocks.  The individuals are the ones indicator_idv selects; the
// reference takes the first ni_test tokens of a line (:2263-2279).
inline bool BimbamXwz(const std::string &file_geno, const std::vector<int> &indicator_idv, const std::vector<int> &indicator_snp,
                      const std::vector<size_t> &vec_cat, const std::vector<double> *w, const std::vector<double> &z, const size_t n_vc,
                      Matrix *Xz, Matrix *XWz, size_t *n_skipped = nullptr) {
  const size_t ni_total = indicator_idv.size();
  BimbamReader rd(file_geno, ni_total);
  if (!rd.ok()) {
    std::cout << "error reading genotype file:" << file_geno << std::endl;
    return false;
  }
  if (Xz->tda != Xz->size2 || XWz->tda != XWz->size2 || Xz->size2 != n_vc || XWz->size2 != n_vc)
    throw HipError(GEMMA_HIP_EINVAL, "BimbamXwz: contiguous Xz and XWz (ni_test x n_vc)");
  const std::vector<int> cat(vec_cat.begin(), vec_cat.end());
  enforce_hip(gemma_hip_ci_begin(ni_total, indicator_idv.data(), n_vc), "BimbamXwz");
  const size_t B = bimbam_block_rows(ni_total, LMM_BATCH_SIZE);
  BlockPrefetch pf(B * ni_total * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= indicator_snp.size()) return 0;
    return rd.read_block(B, static_cast<double *>(slot), ni_total, nullptr, &indicator_snp);
  });
  size_t done = 0, skipped = 0;
  if (n_skipped) *n_skipped = 0;
  for (;;) {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) return false;
    if (l == 0) break;
    if (done + l > cat.size() || done + l > z.size()) throw HipError(GEMMA_HIP_EINVAL, "BimbamXwz: fewer z-scores than analysed SNPs");
    enforce_hip(gemma_hip_ci_xwz(GEMMA_GENO_F64_SNP_MAJOR, slot, l, ni_total, cat.data() + done, z.data() + done,
                                 w ? w->data() + done : nullptr, &skipped), "BimbamXwz");
    if (n_skipped) *n_skipped += skipped;
    done += l;
  }
  enforce_hip(gemma_hip_ci_xwz_end(Xz->data, XWz->data), "BimbamXwz");
  return true;
}

// BimbamXtXwz, src/vc.cpp:2480-2566, after BimbamXwz: XtXWz is ns_test x n_vc
inline bool BimbamXtXwz(const std::string &file_geno, const std::vector<int> &indicator_idv, const std::vector<int> &indicator_snp,
                        const size_t n_vc, Matrix *XtXWz) {
  const size_t ni_total = indicator_idv.size();
  BimbamReader rd(file_geno, ni_total);
  if (!rd.ok()) {
    std::cout << "error reading genotype file:" << file_geno << std::endl;
    return false;
  }
  if (XtXWz->tda != n_vc || XtXWz->size2 != n_vc) throw HipError(GEMMA_HIP_EINVAL, "BimbamXtXwz: contiguous XtXWz (ns_test x n_vc)");
  const size_t B = bimbam_block_rows(ni_total, LMM_BATCH_SIZE);
  BlockPrefetch pf(B * ni_total * sizeof(double), [&](void *slot, int) -> size_t {
    if (rd.lines_read() >= indicator_snp.size()) return 0;
    return rd.read_block(B, static_cast<double *>(slot), ni_total, nullptr, &indicator_snp);
  });
  size_t done = 0;
  for (;;) {
    void *slot = nullptr;
    const size_t l = pf.next(slot);
    if (l == (size_t)-1) return false;
    if (l == 0) break;
    if (done + l > XtXWz->size1) throw HipError(GEMMA_HIP_EINVAL, "BimbamXtXwz: fewer rows of XtXWz than analysed SNPs");
    enforce_hip(gemma_hip_ci_xtxwz(GEMMA_GENO_F64_SNP_MAJOR, slot, l, ni_total, XtXWz->data + done * n_vc), "BimbamXtXwz");
    done += l;
  }
  return true;
}

// CalcCIss, src/vc.cpp:2727-2950, with detail::small_inverse in place of the LU calls
inline void CalcCIss(const Matrix *Xz, const Matrix *XWz, const Matrix *XtXWz, const Matrix *S_mat, const Matrix *Svar_mat,
                     const std::vector<double> &w, const std::vector<double> &z, const Vector *s_vec, const std::vector<size_t> &vec_cat,
                     const std::vector<double> &v_pve, std::vector<double> &v_se_pve, double &pve_total, double &se_pve_total,
                     std::vector<double> &v_sigma2, std::vector<double> &v_se_sigma2, std::vector<double> &v_enrich,
                     std::vector<double> &v_se_enrich) {
  const size_t n_vc = XWz->size2, ns_test = w.size(), ni_test = XWz->size1;
  auto sv = [&](size_t i) { return s_vec->data[i * s_vec->stride]; };
  auto at = [](const Matrix *M, size_t i, size_t j) { return M->data[i * M->tda + j]; };
  std::vector<double> w_pve(ns_test), zwz(n_vc, 0.0), zz(n_vc, 0.0), Xz_pve(ni_test, 0.0), WXtXWz(ns_test);
  std::vector<double> Si(n_vc * n_vc), Var(n_vc * n_vc, 0.0), qvar(n_vc * n_vc, 0.0);
  double d, s0, s1, s, s_pve = 0, s_snp = 0;
  for (size_t i = 0; i < ns_test; i++) {
    zwz[vec_cat[i]] += z[i] * w[i] * z[i];
    zz[vec_cat[i]] += z[i] * z[i];
  }
  for (size_t i = 0; i < n_vc; i++) {
    s_pve += v_pve[i];
    s_snp += sv(i);
    const double a = v_pve[i] / sv(i);
    for (size_t k = 0; k < ni_test; k++) Xz_pve[k] += a * at(Xz, k, i);
  }
  for (size_t i = 0; i < ns_test; i++) w_pve[i] = v_pve[vec_cat[i]] / sv(vec_cat[i]);
  s0 = 1 - s_pve;
  for (size_t i = 0; i < n_vc; i++) s0 += zz[i] * v_pve[i] / sv(i);
  auto dot_cols = [&](const Matrix *A, size_t i, const Matrix *Bm, size_t j, size_t rows) {
    double r = 0;
    for (size_t k = 0; k < rows; k++) r += at(A, k, i) * at(Bm, k, j);
    return r;
  };
  for (size_t i = 0; i < n_vc; i++) {
    s1 = s0;
    s1 -= zwz[i] * (1 - s_pve) / sv(i);
    for (size_t k = 0; k < ns_test; k++) WXtXWz[k] = at(XtXWz, k, i) * w_pve[k];
    d = 0;
    for (size_t k = 0; k < ni_test; k++) d += Xz_pve[k] * at(XWz, k, i);
    s1 -= d / sv(i);
    for (size_t j = 0; j < n_vc; j++) {
      s = s1;
      s -= zwz[j] * (1 - s_pve) / sv(j);
      d = 0;
      for (size_t k = 0; k < ns_test; k++) d += WXtXWz[k] * at(XtXWz, k, j);
      s += d / (sv(i) * sv(j));
      d = dot_cols(XWz, i, XWz, j, ni_test);
      s += d / (sv(i) * sv(j)) * (1 - s_pve);
      d = 0;
      for (size_t k = 0; k < ni_test; k++) d += Xz_pve[k] * at(XWz, k, j);
      s -= d / sv(j);
      qvar[i * n_vc + j] = s;
    }
  }
  d = (double)(ni_test - 1);
  for (double &v : qvar) v *= 2.0 / (d * d * d);
  for (size_t i = 0; i < n_vc; i++)
    for (size_t j = 0; j < n_vc; j++) Si[i * n_vc + j] = at(S_mat, i, j);
  if (!detail::small_inverse(Si, n_vc)) throw std::runtime_error("CalcCIss: S is singular");
  for (size_t i = 0; i < n_vc; i++)
    for (size_t j = i; j < n_vc; j++) {
      d = at(Svar_mat, i, j);
      d *= v_pve[i] * v_pve[j];
      d += qvar[i * n_vc + j];
      Var[i * n_vc + j] = Var[j * n_vc + i] = d;
    }
  Var = detail::matmul(detail::matmul(Si, Var, n_vc), Si, n_vc);
  v_sigma2.clear();
  v_enrich.clear();
  v_se_pve.clear();
  v_se_sigma2.clear();
  v_se_enrich.clear();
  for (size_t i = 0; i < n_vc; i++) {
    v_sigma2.push_back(v_pve[i] / sv(i));
    v_enrich.push_back(v_pve[i] / sv(i) * s_snp / s_pve);
  }
  for (size_t i = 0; i < n_vc; i++) {
    d = std::sqrt(Var[i * n_vc + i]);
    v_se_pve.push_back(d);
    v_se_sigma2.push_back(d / sv(i));
  }
  pve_total = 0;
  se_pve_total = 0;
  for (size_t i = 0; i < n_vc; i++) {
    pve_total += v_pve[i];
    for (size_t j = 0; j < n_vc; j++) se_pve_total += Var[i * n_vc + j];
  }
  se_pve_total = std::sqrt(se_pve_total);
  std::vector<double> T(n_vc * n_vc);
  for (size_t i = 0; i < n_vc; i++) {
    d = v_pve[i] / s_pve;
    const double d1 = sv(i);
    for (size_t j = 0; j < n_vc; j++) T[i * n_vc + j] = (i == j ? (1 - d) : -1 * d) / d1 * s_snp / s_pve;
  }
  const std::vector<double> VarEnrich = detail::matmul(detail::matmul(T, Var, n_vc), T, n_vc, true);
  for (size_t i = 0; i < n_vc; i++) v_se_enrich.push_back(std::sqrt(VarEnrich[i * n_vc + i]));
}

// The estimates of CalcVCss / CalcCIss, as PARAM keeps them
struct VCEST {
  std::vector<double> v_pve, v_se_pve, v_sigma2, v_se_sigma2, v_enrich, v_se_enrich;
  double pve_total = 0, se_pve_total = 0;
};

// The -beta branch of a_mode 61 / 62 on a PLINK set, src/gemma.cpp:2102-2220: ObtainWeight, UpdateSNP, ReadFile_beta, Calcq, CalcS,
// CalcVCss -- and for a_mode 62 (ldsc) the second round of :2182-2212: UpdateWeight from the first round's pve, ReadFile_beta and
// Calcq with those weights, CalcS for A beside the kept K, CalcVCss.  The second CalcS uses slot 2: the reference's PlinkKin adds
// to the A the first round left.  S: 2 n_vc x n_vc, s: n_vc + 1 (ns per category, then ni_test).
inline bool CalcVCssBeta(const std::string &file_bed, const std::string &file_beta, const std::vector<int> &indicator_idv,
                         std::vector<int> &indicator_snp, const std::vector<SNPINFO> &snpInfo, const std::map<std::string, size_t> &mapRS2cat,
                         const std::map<std::string, std::vector<double>> &mapRS2wcat, const Matrix *W, const size_t n_vc,
                         const size_t n_block, const bool ldsc, Matrix *S, Matrix *Vq, Vector *q, Vector *s, size_t &ni_study,
                         size_t &ns_study, size_t &ns_test, VCEST &est) {
  std::set<std::string> setSnps_beta;
  if (!ReadFile_snps_header(file_beta, setSnps_beta)) return false;
  std::map<std::string, double> mapRS2wA, mapRS2wK;
  ObtainWeight(snpInfo, indicator_snp, setSnps_beta, mapRS2wcat, mapRS2cat, mapRS2wK);
  UpdateSNP(snpInfo, indicator_snp, mapRS2wK);
  Matrix S_mat = matrix_view(S->data, n_vc, n_vc), Svar_mat = matrix_view(S->data + n_vc * n_vc, n_vc, n_vc);
  Vector s_vec = vector_view(s->data, n_vc);
  std::vector<size_t> vec_cat, vec_ni;
  std::vector<double> vec_weight, vec_z2;
  size_t ni_test = 0;
  for (int v : indicator_idv) ni_test += v != 0;
  ReadFile_beta(file_beta, mapRS2cat, mapRS2wK, vec_cat, vec_ni, vec_weight, vec_z2, ni_study, ns_study, ns_test);
  Calcq(n_block, vec_cat, vec_ni, vec_weight, vec_z2, Vq, q, &s_vec);
  if (!CalcS(file_bed, indicator_idv, indicator_snp, mapRS2wK, mapRS2cat, snpInfo, W, n_vc, S, &s_vec, 0)) return false;
  CalcVCss(Vq, &S_mat, &Svar_mat, q, &s_vec, (double)ni_study, est.v_pve, est.v_se_pve, est.pve_total, est.se_pve_total, est.v_sigma2,
           est.v_se_sigma2, est.v_enrich, est.v_se_enrich);
  if (ldsc) {
    size_t ns_total = 0;
    UpdateWeight(1, mapRS2wK, ni_study, &s_vec, est.v_pve, mapRS2wcat, mapRS2cat, mapRS2wA);
    ReadFile_beta(file_beta, mapRS2cat, mapRS2wA, vec_cat, vec_ni, vec_weight, vec_z2, ni_study, ns_total, ns_test);
    Calcq(n_block, vec_cat, vec_ni, vec_weight, vec_z2, Vq, q, &s_vec);
    if (!CalcS(file_bed, indicator_idv, indicator_snp, mapRS2wA, mapRS2cat, snpInfo, W, n_vc, S, &s_vec, 2)) return false;
    CalcVCss(Vq, &S_mat, &Svar_mat, q, &s_vec, (double)ni_study, est.v_pve, est.v_se_pve, est.pve_total, est.se_pve_total, est.v_sigma2,
             est.v_se_sigma2, est.v_enrich, est.v_se_enrich);
  }
  s->data[n_vc * s->stride] = (double)ni_test;
  return true;
}

// -study PREFIX -ref PREFIX without genotypes, src/gemma.cpp:2231-2330: ReadFile_study + ReadFile_ref + CalcVCss with the study's
// SNP counts and sample size (:2299); the reference panel's counts and ni_ref only go into the size vector it writes (:2305-2307),
// returned in size_out (n_vc + 1) when given
inline bool CalcVCssStudy(const std::string &file_study, const std::string &file_ref, VCEST &est, std::vector<double> *size_out = nullptr) {
  std::vector<double> Vq, q, s_study, S, Svar, s_ref;
  size_t ni_study = 0, ni_ref = 0;
  if (!ReadFile_study(file_study, Vq, q, s_study, ni_study) || !ReadFile_ref(file_ref, S, Svar, s_ref, ni_ref) || q.size() != s_ref.size())
    return false;
  const size_t n_vc = q.size();
  Matrix Vm = matrix_view(Vq.data(), n_vc, n_vc), Sm = matrix_view(S.data(), n_vc, n_vc), Sv = matrix_view(Svar.data(), n_vc, n_vc);
  Vector qv = vector_view(q.data(), n_vc), sv = vector_view(s_study.data(), n_vc);
  CalcVCss(&Vm, &Sm, &Sv, &qv, &sv, (double)ni_study, est.v_pve, est.v_se_pve, est.pve_total, est.se_pve_total, est.v_sigma2,
           est.v_se_sigma2, est.v_enrich, est.v_se_enrich);
  if (size_out) {
    *size_out = s_ref;
    size_out->push_back((double)ni_ref);
  }
  return true;
}

// ---------------------------------------------------------------------------------------------------------------
// windowed SNP correlation: -calccor (a_mode 71), src/gemma.cpp:2046-2059
// ---------------------------------------------------------------------------------------------------------------
// VARCOV::CalcNB, src/varcov.cpp:168-217, branch for branch: the number of right-hand neighbours of every analysed SNP
inline void VARCOV::CalcNB(std::vector<SNPINFO> &snpInfo_sort) {
  size_t t2 = 0, n_nb = 0;
  for (size_t t = 0; t < indicator_snp.size(); ++t) {
    if (indicator_snp[t] == 0) {
      continue;
    }

    if (snpInfo_sort[t].chr == "-9" || (snpInfo_sort[t].cM == -9 && window_cm != 0) ||
        (snpInfo_sort[t].base_position == -9 && window_bp != 0)) {
      snpInfo_sort[t].n_nb = 0;
      continue;
    }

    if (t == indicator_snp.size() - 1) {
      snpInfo_sort[t].n_nb = 0;
      continue;
    }

    t2 = t + 1;
    n_nb = 0;

    while (t2 < indicator_snp.size() && snpInfo_sort[t2].chr == snpInfo_sort[t].chr && indicator_snp[t2] == 0) {
      t2++;
    }

    while (t2 < indicator_snp.size() && snpInfo_sort[t2].chr == snpInfo_sort[t].chr &&
           (snpInfo_sort[t2].cM - snpInfo_sort[t].cM < window_cm || window_cm == 0) &&
           (snpInfo_sort[t2].base_position - snpInfo_sort[t].base_position < (long int)window_bp || window_bp == 0) &&
           (n_nb < window_ns || window_ns == 0)) {
      t2++;
      n_nb++;
      while (t2 < indicator_snp.size() && snpInfo_sort[t2].chr == snpInfo_sort[t].chr && indicator_snp[t2] == 0) {
        t2++;
      }
    }

    snpInfo_sort[t].n_nb = n_nb;
  }
}

// VARCOV::WriteCov, src/varcov.cpp:74-145: flag 0 writes the header, any other flag appends one line per row of Cov_mat
// (row = var followed by the correlations of the window)
inline void VARCOV::WriteCov(const int flag, const std::vector<SNPINFO> &snpInfo_sub, const std::vector<std::vector<double>> &Cov_mat) {
  const std::string file_cov = path_out + "/" + file_out + ".cor.txt";
  std::ofstream outfile;
  if (flag == 0) {
    outfile.open(file_cov.c_str(), std::ofstream::out);
    if (!outfile) {
      std::cout << "error writing file: " << file_cov << std::endl;
      return;
    }
    outfile << "chr\trs\tps\tn_mis\tn_obs\tallele1\tallele0\taf\twindow_size\tvar\tcor" << std::endl;
  } else {
    outfile.open(file_cov.c_str(), std::ofstream::app);
    if (!outfile) {
      std::cout << "error writing file: " << file_cov << std::endl;
      return;
    }
    for (size_t i = 0; i < Cov_mat.size(); i++) {
      outfile << snpInfo_sub[i].chr << "\t" << snpInfo_sub[i].rs_number << "\t" << snpInfo_sub[i].base_position << "\t"
              << snpInfo_sub[i].n_miss << "\t" << snpInfo_sub[i].n_idv << "\t" << snpInfo_sub[i].a_minor << "\t"
              << snpInfo_sub[i].a_major << "\t" << std::fixed << std::setprecision(3) << snpInfo_sub[i].maf << "\t"
              << Cov_mat[i].size() - 1 << "\t";
      outfile << std::scientific << std::setprecision(6) << Cov_mat[i][0] << "\t";
      if (Cov_mat[i].size() == 1) {
        outfile << "NA";
      } else {
        for (size_t j = 1; j < Cov_mat[i].size(); j++) {
          if (j == (Cov_mat[i].size() - 1)) outfile << Cov_mat[i][j];
          else outfile << Cov_mat[i][j] << ",";
        }
      }
      outfile << "\n";
    }
  }
  outfile.close();
  outfile.clear();
}

// The loop over t of src/varcov.cpp:281-338 / :381-438 in blocks: LMM_BATCH_SIZE output SNPs and the halo their windows reach
// into go to gemma_hip_cor_block together; the halo rows are read again with the next block, nothing is kept across calls.
// read_rows(first, count, dst) fetches the rows of analysed SNPs first .. first + count - 1 (false: read error).
template <class ReadRows> inline void VARCOV::Analyze(int geno_kind, size_t row_len, ReadRows read_rows) {
  CalcNB(snpInfo);
  std::vector<size_t> keep;
  std::vector<int> nb;
  for (size_t t = 0; t < indicator_snp.size(); ++t)
    if (indicator_snp[t] != 0) {
      keep.push_back(t);
      nb.push_back((int)snpInfo[t].n_nb);
    }
  std::vector<SNPINFO> snpInfo_sub;
  std::vector<std::vector<double>> Cov_mat;
  WriteCov(0, snpInfo_sub, Cov_mat);
  enforce_hip(gemma_hip_cor_begin(indicator_idv.size(), indicator_idv.data()), "VARCOV");
  const size_t l = keep.size(), B = io_block_rows(LMM_BATCH_SIZE);
  const size_t elem = geno_kind == GEMMA_GENO_PLINK_2BIT ? 1 : sizeof(double);
  std::vector<unsigned char> block;
  std::vector<double> var, cor;
  for (size_t s0 = 0; s0 < l; s0 += B) {
    const size_t s1 = std::min(l, s0 + B);
    size_t last = s1 - 1, total = 0;
    for (size_t j = s0; j < s1; ++j) {
      last = std::max(last, j + (size_t)nb[j]);
      total += (size_t)nb[j];
    }
    const size_t l_in = last + 1 - s0, l_out = s1 - s0;
    block.resize(l_in * row_len * elem);
    if (!read_rows(s0, l_in, block.data())) { // the records of the earlier blocks are in the file; the state is given back
      error = true;
      enforce_hip(gemma_hip_cor_release(), "VARCOV");
      return;
    }
    var.resize(l_out);
    cor.resize(std::max<size_t>(total, 1));
    enforce_hip(gemma_hip_cor_block(geno_kind, block.data(), l_in, row_len, l_out, nb.data() + s0, var.data(), cor.data()), "VARCOV");
    snpInfo_sub.clear();
    Cov_mat.assign(l_out, std::vector<double>());
    size_t o = 0;
    for (size_t j = s0; j < s1; ++j) {
      std::vector<double> &row = Cov_mat[j - s0];
      row.push_back(var[j - s0]);
      row.insert(row.end(), cor.begin() + (long)o, cor.begin() + (long)(o + (size_t)nb[j]));
      o += (size_t)nb[j];
      snpInfo_sub.push_back(snpInfo[keep[j]]);
    }
    WriteCov(1, snpInfo_sub, Cov_mat);
  }
  enforce_hip(gemma_hip_cor_release(), "VARCOV");
}

// VARCOV::AnalyzePlink, src/varcov.cpp:348-446
inline void VARCOV::AnalyzePlink() {
  const std::string file_bed = file_bfile + ".bed";
  std::ifstream infile(file_bed.c_str(), std::ios::binary);
  if (!infile) {
    std::cout << "error reading bed file:" << file_bed << std::endl;
    error = true;
    return;
  }
  const size_t n_bit = (indicator_idv.size() + 3) / 4;
  std::vector<size_t> pos; // file index of the j-th analysed SNP
  for (size_t t = 0; t < indicator_snp.size(); ++t)
    if (indicator_snp[t] != 0) pos.push_back(t);
  Analyze(GEMMA_GENO_PLINK_2BIT, n_bit, [&](size_t first, size_t count, unsigned char *dst) {
    size_t t_next = pos[first];
    if (read_bed_rows(infile, indicator_snp, t_next, n_bit, dst, count) != count) {
      std::cout << "error reading bed file:" << file_bed << " (truncated)" << std::endl;
      return false;
    }
    return true;
  });
}

// VARCOV::AnalyzeBimbam, src/varcov.cpp:249-346.  The text cannot be repositioned: every block opens the file again and lets the
// reader drop the lines before its first row unparsed.
inline void VARCOV::AnalyzeBimbam() {
  const size_t ni_total = indicator_idv.size();
  std::vector<size_t> pos;
  for (size_t t = 0; t < indicator_snp.size(); ++t)
    if (indicator_snp[t] != 0) pos.push_back(t);
  Analyze(GEMMA_GENO_F64_SNP_MAJOR, ni_total, [&](size_t first, size_t count, unsigned char *dst) {
    BimbamReader rd(file_geno, ni_total);
    if (!rd.ok()) {
      std::cout << "error reading genotype file:" << file_geno << std::endl;
      return false;
    }
    std::vector<int> sel(indicator_snp.size(), 0);
    for (size_t j = first; j < first + count; ++j) sel[pos[j]] = 1;
    double *X = reinterpret_cast<double *>(dst);
    for (size_t got = 0; got < count;) {
      const size_t r = rd.read_block(count - got, X + got * ni_total, ni_total, nullptr, &sel);
      if (r == 0 || r == (size_t)-1) {
        std::cout << "error reading genotype file:" << file_geno << " (truncated)" << std::endl;
        return false;
      }
      got += r;
    }
    return true;
  });
}

} // namespace gemma_amd
#endif

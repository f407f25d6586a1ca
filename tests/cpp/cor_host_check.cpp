// Host side of -calccor without a device (tests/test_cor_host.py, also built with -fsanitize=address,undefined):
// VARCOV::CalcNB and VARCOV::WriteCov of include/gemma_io_host.hpp.
//
//   cor_host_check nb    snps.txt window_cm window_bp window_ns           -> one n_nb per line of snps.txt on stdout
//   cor_host_check write snps.txt rows.txt outdir name                    -> outdir/name.cor.txt
//
// snps.txt: one SNP per line, `indicator chr rs cM bp a_minor a_major n_miss n_idv maf` (maf as a hexadecimal float);
// rows.txt: one line per analysed SNP, `var cor_1 ... cor_w` as hexadecimal floats.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gemma_io_host.hpp"

using namespace gemma_amd;

static bool read_snps(const char *path, VARCOV &v) {
  std::ifstream in(path);
  if (!in) return false;
  std::string line;
  while (std::getline(in, line)) {
    if (line.empty()) continue;
    std::istringstream ss(line);
    SNPINFO s;
    int ind;
    std::string maf;
    long bp;
    if (!(ss >> ind >> s.chr >> s.rs_number >> s.cM >> bp >> s.a_minor >> s.a_major >> s.n_miss >> s.n_idv >> maf)) return false;
    s.base_position = bp;
    s.maf = strtod(maf.c_str(), nullptr);
    s.missingness = 0;
    s.n_nb = 0;
    s.file_position = v.snpInfo.size();
    v.snpInfo.push_back(s);
    v.indicator_snp.push_back(ind);
  }
  return true;
}

int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const std::string mode = argv[1];
  VARCOV v;
  if (!read_snps(argv[2], v)) return 3;
  if (mode == "nb" && argc == 6) {
    v.window_cm = atof(argv[3]);
    v.window_bp = strtoul(argv[4], nullptr, 10);
    v.window_ns = strtoul(argv[5], nullptr, 10);
    v.CalcNB(v.snpInfo);
    for (const SNPINFO &s : v.snpInfo) printf("%zu\n", s.n_nb);
    return 0;
  }
  if (mode == "write" && argc == 6) {
    v.path_out = argv[4];
    v.file_out = argv[5];
    std::ifstream in(argv[3]);
    if (!in) return 3;
    std::vector<SNPINFO> sub;
    std::vector<std::vector<double>> Cov_mat;
    v.WriteCov(0, sub, Cov_mat);
    std::string line;
    size_t t = 0;
    while (std::getline(in, line)) {
      while (t < v.indicator_snp.size() && v.indicator_snp[t] == 0) ++t;
      if (t >= v.indicator_snp.size()) return 4;
      std::istringstream ss(line);
      std::vector<double> row;
      std::string tok;
      while (ss >> tok) row.push_back(strtod(tok.c_str(), nullptr));
      if (row.empty()) return 4;
      Cov_mat.push_back(row);
      sub.push_back(v.snpInfo[t++]);
      if (Cov_mat.size() == 1000) { // appended in pieces, as the reference appends every 10 000 SNPs
        v.WriteCov(1, sub, Cov_mat);
        sub.clear();
        Cov_mat.clear();
      }
    }
    if (!Cov_mat.empty()) v.WriteCov(1, sub, Cov_mat);
    return 0;
  }
  return 2;
}

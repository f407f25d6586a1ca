// Driver over the prediction part of include/gemma_host.hpp (class BSLMM, class PRDT) for tests/test_prdt_cpu.py and
// tests/test_gpu_prdt.py.
//   prdt_mirror_driver writers DIR   no GPU: DIR/snps.txt ("chr rs ps n_miss alpha" per analysed SNP), DIR/bv.txt ("1 value" per
//                                    analysed individual, "0" otherwise), DIR/prdt.txt ("0 value" per predicted individual, "1"
//                                    otherwise) -> DIR/out.param.txt, out.bv.txt, out.prdt.txt through WriteParam / WriteBV / WriteFiles
//   prdt_mirror_driver chain DIR     GPU: DIR/meta.txt "n ni_total l ld ns_test lambda pheno_mean a_mode", U.bin, eval.bin, Uty.bin,
//                                    ind.bin (int32), rows.bin (l x ld bytes of .bed rows), eff.bin (l doubles) -> RidgeR over the rows
//                                    (alpha.bin, bv.bin), then PRDT::Analyze of the same rows with eff and Finish (y.bin); prints
//                                    "ns_test K" and "ignored i" lines
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "gemma_host.hpp"

using namespace gemma_amd;

template <class T> static std::vector<T> slurp(const std::string &path, size_t count) {
  std::vector<T> v(count);
  std::ifstream f(path.c_str(), std::ios::binary);
  if (!f.read(reinterpret_cast<char *>(v.data()), (std::streamsize)(count * sizeof(T)))) throw std::runtime_error("short read: " + path);
  return v;
}
static void dump(const std::string &path, const std::vector<double> &v) {
  std::ofstream f(path.c_str(), std::ios::binary);
  f.write(reinterpret_cast<const char *>(v.data()), (std::streamsize)(v.size() * sizeof(double)));
}

static int writers(const std::string &dir) {
  BSLMM b;
  std::ifstream f((dir + "/snps.txt").c_str());
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    SNPINFO si = SNPINFO();
    double a;
    if (!(ss >> si.chr >> si.rs_number >> si.base_position >> si.n_miss >> a)) continue;
    b.snpInfo.push_back(si);
    b.alpha.push_back(a);
  }
  std::ifstream g((dir + "/bv.txt").c_str());
  int k;
  while (g >> k) {
    b.indicator_idv.push_back(k);
    if (k) { double v; g >> v; b.bv.push_back(v); }
  }
  b.WriteParam(dir + "/out.param.txt");
  b.WriteBV(dir + "/out.bv.txt");
  std::ifstream h((dir + "/prdt.txt").c_str());
  std::vector<int> ind;
  std::vector<double> y;
  while (h >> k) {
    ind.push_back(k);
    if (!k) { double v; h >> v; y.push_back(v); }
  }
  PRDT::WriteFiles(dir + "/out.prdt.txt", ind, y);
  return 0;
}

static int chain(const std::string &dir) {
  size_t n, ni, l, ld, ns_test;
  double lambda, mean;
  int a_mode;
  std::ifstream m((dir + "/meta.txt").c_str());
  if (!(m >> n >> ni >> l >> ld >> ns_test >> lambda >> mean >> a_mode)) throw std::runtime_error("meta.txt");
  std::vector<double> U = slurp<double>(dir + "/U.bin", n * n), ev = slurp<double>(dir + "/eval.bin", n), uty = slurp<double>(dir + "/Uty.bin", n);
  std::vector<double> eff = slurp<double>(dir + "/eff.bin", l);
  std::vector<int> ind = slurp<int>(dir + "/ind.bin", ni);
  std::vector<unsigned char> rows = slurp<unsigned char>(dir + "/rows.bin", l * ld);
  enforce_hip(gemma_hip_init(0, 0), "init");
  BSLMM b;
  b.indicator_idv = ind;
  Matrix Um = matrix_view(U.data(), n, n);
  Vector e = vector_view(ev.data(), n), u = vector_view(uty.data(), n);
  b.RidgeR(&Um, &u, &e, lambda, GEMMA_GENO_PLINK_2BIT, rows.data(), l, ld, ns_test);
  dump(dir + "/alpha.bin", b.alpha);
  dump(dir + "/bv.bin", b.bv);
  PRDT p(ind);
  const size_t half = l / 2; // two calls: the bookkeeping of `ignored` counts rows over all of them
  p.Analyze(GEMMA_GENO_PLINK_2BIT, rows.data(), half, ld, eff.data());
  p.Analyze(GEMMA_GENO_PLINK_2BIT, rows.data() + half * ld, l - half, ld, eff.data() + half);
  dump(dir + "/y.bin", p.Finish(mean, a_mode));
  std::cout << "ns_test " << p.ns_test << std::endl;
  for (size_t i : p.ignored) std::cout << "ignored " << i << std::endl;
  gemma_hip_shutdown();
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: prdt_mirror_driver writers|chain DIR\n");
    return 2;
  }
  try {
    const std::string mode = argv[1];
    if (mode == "writers") return writers(argv[2]);
    if (mode == "chain") return chain(argv[2]);
    return 2;
  } catch (const std::exception &ex) {
    std::fprintf(stderr, "%s\n", ex.what());
    return 1;
  }
}

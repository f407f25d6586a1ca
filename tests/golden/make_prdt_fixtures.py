"""Printed outputs of the reference binary's ridge / BLUP fit (-bslmm 2, BSLMM::RidgeR) and of -predict 1 / 2 (class PRDT) for
tests/test_prdt_cpu.py and tests/test_gpu_prdt.py -- run in the build container only (oracle/_ref/gemma, see oracle/Makefile):

    python tests/golden/make_prdt_fixtures.py

Sets:
* P   the committed PLINK set, phenotype = P.fam's column 6 (-9 = missing; 154 of 240 analysed);
* B   BXD, the reference's BIMBAM example (bxd_*.gz), trait column 1;
* S   a synthetic PLINK set written by this script from a fixed numpy seed (S.bed / S.bim / S.fam): 300 individuals of which 100
      have no phenotype, 600 SNPs, 1 % missing calls, a trait with heritability about 0.6; SNPs 7 and 311 are missing in every
      unphenotyped individual (-predict skips them), SNP 40 has a single missing training call;
* Sb  the BIMBAM twin of S (Sb.geno.txt.gz, Sb.pheno.txt, Sb.anno.txt) with a covariate file Sb.cvt.txt (an intercept and one
      covariate correlated with the trait).  The reference refuses -c together with -bslmm (src/param.cpp:964-969), so the ridge
      runs have the intercept only; the covariates enter where the reference takes them, in the kinship-only prediction.
Runs, each recorded as the files the reference wrote (text, gzip'd) and <tag>.log.json (what it printed):
* <set>_R    -bslmm 2                          -> .param.txt, .bv.txt; log: pve, se(pve), estimated mean, counts  
* <set>_p1   -epm R.param -emu R.log -predict 1  -> .prdt.txt; log: the SNPs "ignored" (missing in every test individual)
* <set>_p1k  the same with -ebv R.bv -k K (K = the reference's own -gk 1 of the set)
* <set>_p2, <set>_p2k   the two with -predict 2
* B_m43, Sb_m43          -predict 1 with -k K and no -epm (a_mode 43, PRDT::MvnormPrdt; BIMBAM input only: with -bfile and -p
                         the reference's own CheckData refuses the run) -> .prdt.txt; log: the printed vg, ve
* Sb_m43c                the same with -c Sb.cvt.txt (two covariates: W_full beta and the c x c solve for beta take part)
The reference raises SIGINT on a failed enforce: every run is a child process whose exit status is read."""
import gzip
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GEMMA = os.path.join(ROOT, "oracle", "_ref", "gemma")
TXT = os.path.join(ROOT, "tests", "golden", "text")
OUT = os.path.join(ROOT, "tests", "golden", "prdt")


def run(tmp, *args):
    r = subprocess.run([GEMMA] + [str(a) for a in args], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("exit status %d\n%s" % (r.returncode, r.stdout[-2000:]))
    return r.stdout


def keep(tmp, tag, ext):
    with open(os.path.join(tmp, "output", tag + ext), "rb") as f, gzip.GzipFile(os.path.join(OUT, tag + ext + ".gz"), "wb", mtime=0) as g:
        g.write(f.read())


def log_meta(tmp, tag, out):
    meta = {"ignored": [l.split()[1] for l in out.splitlines() if l.startswith("snp ") and "will be ignored" in l]}
    for line in open(os.path.join(tmp, "output", tag + ".log.txt")):
        for key in ("number of total individuals", "number of analyzed individuals", "number of covariates", "number of total SNPs/var",
                    "number of analyzed SNPs/var", "pve estimate in the null model", "se(pve) in the null model", "estimated mean"):
            if line.startswith("## " + key + " ="):
                meta[key] = line.split("=", 1)[1].strip()
    json.dump(meta, open(os.path.join(OUT, tag + ".log.json"), "w"), indent=1, sort_keys=True)


def all_runs(tmp, name, geno, extra_fit):
    """geno: the arguments that name genotypes and phenotypes; extra_fit: added to the -bslmm 2 run only (-a, -c)"""
    R = name + "_R"
    out = run(tmp, *geno, *extra_fit, "-bslmm", 2, "-o", R)
    log_meta(tmp, R, out)
    keep(tmp, R, ".param.txt")
    keep(tmp, R, ".bv.txt")
    run(tmp, *geno, "-gk", 1, "-o", name + "_K")
    epm = ["-epm", os.path.join("output", R + ".param.txt"), "-emu", os.path.join("output", R + ".log.txt")]
    ebv = ["-ebv", os.path.join("output", R + ".bv.txt"), "-k", os.path.join("output", name + "_K.cXX.txt")]
    for mode in (1, 2):
        for suffix, more in (("", []), ("k", ebv)):
            tag = "%s_p%d%s" % (name, mode, suffix)
            out = run(tmp, *geno, *epm, *more, "-predict", mode, "-o", tag)
            log_meta(tmp, tag, out)
            keep(tmp, tag, ".prdt.txt")
    if "-g" in geno:
        for tag, more in ((name + "_m43", []), (name + "_m43c", ["-c", name + ".cvt.txt"])):
            if more and not os.path.exists(os.path.join(tmp, more[1])):
                continue
            out = run(tmp, *geno, *more, "-k", os.path.join("output", name + "_K.cXX.txt"), "-predict", 1, "-o", tag)
            meta = {}
            for line in out.splitlines():
                for key in ("vg", "ve"):
                    if line.startswith("REMLE estimate for %s in the null model = " % key):
                        meta[key] = line.split("=", 1)[1].strip()
            for line in open(os.path.join(tmp, "output", tag + ".log.txt")):
                if line.startswith("## number of covariates ="):
                    meta["number of covariates"] = line.split("=", 1)[1].strip()
            json.dump(meta, open(os.path.join(OUT, tag + ".log.json"), "w"), indent=1, sort_keys=True)
            keep(tmp, tag, ".prdt.txt")


def synthetic(tmp):
    """S (PLINK) and Sb (BIMBAM) from one draw; the committed copies go to tests/golden/prdt/"""
    rng = np.random.default_rng(20240611)
    n, p, n_test = 300, 600, 100
    maf = rng.uniform(0.1, 0.5, p)
    G = rng.binomial(2, maf[:, None], size=(p, n)).astype(np.float64)  # SNP-major
    test = np.zeros(n, dtype=bool)
    test[rng.choice(n, n_test, replace=False)] = True
    beta = np.zeros(p)
    causal = rng.choice(p, 60, replace=False)
    beta[causal] = rng.standard_normal(60)
    g = (G - G.mean(1, keepdims=True)).T @ beta
    y = 3.0 + g + rng.standard_normal(n) * np.sqrt(np.var(g) * 0.4 / 0.6)
    # the covariate file (an intercept and one covariate that carries part of the trait), from a generator of its own so that the
    # draws above and below stay what they were
    cov = 0.6 * (y - y.mean()) / y.std() + np.random.default_rng(20240612).standard_normal(n)
    miss = rng.random((p, n)) < 0.01
    miss[7] = test
    miss[311] = test
    miss[40] = False
    miss[40, np.flatnonzero(~test)[3]] = True
    G[miss] = np.nan
    # PLINK: code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing (src/gemma_io.cpp:2026-2041), individual i in bits 2 (i % 4) of byte i / 4
    code = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    pad = np.zeros((p, (-n) % 4), dtype=np.uint8)
    c4 = np.hstack([code, pad]).reshape(p, -1, 4)
    rows = (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)
    for d in (tmp, OUT):
        with open(os.path.join(d, "S.bed"), "wb") as f:
            f.write(bytes([0x6C, 0x1B, 0x01]) + rows.tobytes())
        with open(os.path.join(d, "S.bim"), "w") as f:
            for s in range(p):
                f.write("%d\tsnp%d\t0\t%d\tA\tG\n" % (1 + s // 200, s, 1000 + 10 * s))
        with open(os.path.join(d, "S.fam"), "w") as f:
            for i in range(n):
                f.write("F%d I%d 0 0 1 %s\n" % (i, i, "-9" if test[i] else "%.6f" % y[i]))
        with open(os.path.join(d, "Sb.pheno.txt"), "w") as f:
            for i in range(n):
                f.write(("NA" if test[i] else "%.6f" % y[i]) + "\n")
        with open(os.path.join(d, "Sb.cvt.txt"), "w") as f:
            for i in range(n):
                f.write("1 %.6f\n" % cov[i])
        with open(os.path.join(d, "Sb.anno.txt"), "w") as f:
            for s in range(p):
                f.write("snp%d, %d, %d\n" % (s, 1000 + 10 * s, 1 + s // 200))
    lines = []
    for s in range(p):
        lines.append(", ".join(["snp%d" % s, "A", "G"] + ["NA" if np.isnan(v) else "%d" % v for v in G[s]]) + "\n")
    open(os.path.join(tmp, "Sb.geno.txt"), "w").write("".join(lines))
    with gzip.GzipFile(os.path.join(OUT, "Sb.geno.txt.gz"), "wb", mtime=0) as f:
        f.write("".join(lines).encode())


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp()
    try:
        for ext in (".bed", ".bim", ".fam"):
            shutil.copy(os.path.join(TXT, "P" + ext), tmp)
        all_runs(tmp, "P", ["-bfile", "P"], [])
        for src, dst in (("bxd_mean_genotypes.txt.gz", "bxd_geno.txt"), ("bxd_trait.txt.gz", "bxd_pheno.txt"),
                         ("bxd_anno.txt.gz", "bxd_anno.txt")):
            with gzip.open(os.path.join(TXT, src), "rt") as f, open(os.path.join(tmp, dst), "w") as g:
                g.write(f.read())
        all_runs(tmp, "B", ["-g", "bxd_geno.txt", "-p", "bxd_pheno.txt"], ["-a", "bxd_anno.txt"])
        synthetic(tmp)
        all_runs(tmp, "S", ["-bfile", "S"], [])
        all_runs(tmp, "Sb", ["-g", "Sb.geno.txt", "-p", "Sb.pheno.txt"], ["-a", "Sb.anno.txt"])
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

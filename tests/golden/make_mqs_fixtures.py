"""Files of the reference binary's MQS runs -- `-gs` (a_mode 25: S, its jackknife variance, the SNP counts) and `-vc 1 -beta`
(a_mode 61 with z-scores: q, Vq, S and the estimates) -- on the committed PLINK set P and on BXD, for tests/test_mqs_cpu.py and
tests/test_gpu_mqs.py.  Run in the build container only (oracle/_ref/gemma, see oracle/Makefile):

    python tests/golden/make_mqs_fixtures.py

Inputs, written here and committed (tests/golden/text/):
* mqs_cat2.txt   `rs catA catB`: SNP t of P.bim is in catA when t % 3 != 0, else in catB;
* mqs_cat3.txt   three categories by t % 5 in {0, 1}, {2}, {3}; t % 5 == 4 is in none (all zeros: the SNP leaves the analysis);
* mqs_beta.txt   `rs z n_total`: seeded z-scores for 19 of every 20 SNPs of P (SNPs without a row leave the -vc 1 runs);
* mqs_bcat2.txt  BXD: first half of the SNPs / second half.
P: the phenotype is P.fam's column 6 with -9 written as NA (154 of 240 analysed; 153 with -c P.cov.txt).
Outputs, one set per run <tag>: <tag>.S.txt (2 n_vc rows: S, then Svar), <tag>.size.txt (ns per category, then ni_test), for the
-vc 1 runs <tag>.q.txt / <tag>.Vq.txt and <tag>.log.json (the estimate lines of the log as printed, six digits), for the -gs runs
<tag>.snps.txt.gz (the analysed SNPs).  A -gs run of the reference ends with a segmentation fault after it wrote its files (a
double free at src/gemma.cpp:1995 / :1998; glibc may catch it first and abort): exit status -11 / 139, or -6 / 134 with glibc's
"double free" message, is accepted when all three files exist, and only then.
* G1 (-gs, no -cat), G2 / G2c (-cat mqs_cat2.txt, without / with -c P.cov.txt), G3 / G3c (mqs_cat3.txt), GB2 (BXD, mqs_bcat2.txt);
* Q2 / Q2c / Q3 / Q3c: the same four P runs as `-beta mqs_beta.txt -vc 1`."""
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
LOG_KEYS = ("pve estimates", "se(pve)", "total pve", "se(total pve)", "sigma2 estimates", "se(sigma2)", "enrichment", "se(enrichment)")


def run(tmp, *args):
    r = subprocess.run([GEMMA] + [str(a) for a in args], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def keep(tmp, tag, suffixes):
    for suf in suffixes:
        shutil.copy(os.path.join(tmp, "output", tag + suf), os.path.join(TXT, tag + suf))


def gs(tmp, tag, extra):
    rc, out = run(tmp, *extra, "-gs", "-o", tag)
    files = [os.path.join(tmp, "output", tag + s) for s in (".S.txt", ".size.txt", ".snps.txt.gz")]
    died_at_the_double_free = rc in (-11, 139) or (rc in (-6, 134) and "double free" in out)
    if not (rc == 0 or died_at_the_double_free) or not all(os.path.exists(f) and os.path.getsize(f) > 0 for f in files):
        raise RuntimeError("%s: exit %d\n%s" % (tag, rc, out[-2000:]))
    keep(tmp, tag, (".S.txt", ".size.txt", ".snps.txt.gz"))


def vc1(tmp, tag, extra):
    rc, out = run(tmp, *extra, "-beta", "mqs_beta.txt", "-vc", 1, "-o", tag)
    if rc != 0:
        raise RuntimeError("%s: exit %d\n%s" % (tag, rc, out[-2000:]))
    keep(tmp, tag, (".S.txt", ".size.txt", ".q.txt", ".Vq.txt"))
    meta = {}
    for line in open(os.path.join(tmp, "output", tag + ".log.txt")):
        for key in LOG_KEYS:
            if line.startswith("## " + key + " ="):
                meta[key] = line.split("=", 1)[1].split()
        if line.startswith("## number of") and ("individuals" in line or "components" in line):
            k, v = line[2:].split("=", 1)
            meta[k.strip()] = v.strip()
    json.dump(meta, open(os.path.join(TXT, tag + ".log.json"), "w"), indent=1, sort_keys=True)


def main():
    tmp = tempfile.mkdtemp()
    try:
        for ext in (".bed", ".bim", ".fam", ".cov.txt"):
            shutil.copy(os.path.join(TXT, "P" + ext), tmp)
        with open(os.path.join(tmp, "P.fam")) as f, open(os.path.join(tmp, "pheno.txt"), "w") as g:
            for line in f:
                v = line.split()[5]
                g.write(("NA" if v == "-9" else v) + "\n")
        snps = [l.split()[1] for l in open(os.path.join(tmp, "P.bim")) if l.strip()]
        with open(os.path.join(TXT, "mqs_cat2.txt"), "w") as f:
            f.write("rs catA catB\n")
            for t, rs in enumerate(snps):
                f.write("%s %d %d\n" % (rs, t % 3 != 0, t % 3 == 0))
        with open(os.path.join(TXT, "mqs_cat3.txt"), "w") as f:
            f.write("rs catA catB catC\n")
            for t, rs in enumerate(snps):
                f.write("%s %d %d %d\n" % (rs, t % 5 in (0, 1), t % 5 == 2, t % 5 == 3))
        rng = np.random.default_rng(20170601)
        z = rng.standard_normal(len(snps)) * 1.4
        with open(os.path.join(TXT, "mqs_beta.txt"), "w") as f:
            f.write("rs z n_total\n")
            for t, rs in enumerate(snps):
                if t % 20 != 7:
                    f.write("%s %.6f %d\n" % (rs, z[t], 154 - (t % 4)))
        for name in ("mqs_cat2.txt", "mqs_cat3.txt", "mqs_beta.txt"):
            shutil.copy(os.path.join(TXT, name), tmp)
        base = ["-bfile", "P", "-p", "pheno.txt"]
        gs(tmp, "G1", base)
        for tag, cat in (("2", "mqs_cat2.txt"), ("3", "mqs_cat3.txt")):
            for suf, cov in (("", []), ("c", ["-c", "P.cov.txt"])):
                gs(tmp, "G" + tag + suf, base + ["-cat", cat] + cov)
                vc1(tmp, "Q" + tag + suf, base + ["-cat", cat] + cov)
        # BXD
        for src, dst in (("bxd_mean_genotypes.txt.gz", "bxd_geno.txt"), ("bxd_trait.txt.gz", "bxd_pheno.txt"),
                         ("bxd_anno.txt.gz", "bxd_anno.txt")):
            with gzip.open(os.path.join(TXT, src), "rt") as f, open(os.path.join(tmp, dst), "w") as g:
                g.write(f.read())
        bsnps = [l.split(",")[0].strip() for l in open(os.path.join(tmp, "bxd_geno.txt")) if l.strip()]
        with open(os.path.join(TXT, "mqs_bcat2.txt"), "w") as f:
            f.write("rs catA catB\n")
            for t, rs in enumerate(bsnps):
                f.write("%s %d %d\n" % (rs, t < len(bsnps) // 2, t >= len(bsnps) // 2))
        shutil.copy(os.path.join(TXT, "mqs_bcat2.txt"), tmp)
        gs(tmp, "GB2", ["-g", "bxd_geno.txt", "-p", "bxd_pheno.txt", "-a", "bxd_anno.txt", "-cat", "mqs_bcat2.txt"])
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

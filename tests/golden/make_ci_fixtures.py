"""Files of the reference binary's runs of the MQS confidence intervals (`-ci 1`, `-ci 2`; a_mode 66 / 67) and of the LDSC-weighted
second round of `-vc 2 -beta` (a_mode 62) on the committed PLINK set P, for tests/test_ci_cpu.py and tests/test_gpu_ci.py.  Run
where oracle/_ref/gemma exists (see oracle/Makefile), after tests/golden/make_mqs_fixtures.py:

    python tests/golden/make_ci_fixtures.py

Inputs, written here and committed (tests/golden/text/):
* ci_wcat2.txt     `rs wA wB`: per SNP of P.bim, in order, rng.uniform(1, 30) then rng.uniform(0.5, 10) of default_rng(5);
* ci_wcat3.txt     `rs wA wB wC`: rng.uniform(0.5, 20, size=3) of default_rng(6);
* ci_beta_a1.txt   `rs a1 z n_total`: the rows and z of mqs_beta.txt with an allele column -- .bim column 5 (the minor allele)
                   when t % 3 != 0, column 6 otherwise, so that a third of the z change sign against C1_2.
The phenotype is P.fam's column 6 with -9 written as NA; the -ref prefixes are the committed G2 / G3 / G3c files.
Outputs per run <tag>: <tag>.log.json (the estimate lines and the `## number of ...` lines of the log as printed); for the -vc 2 runs
also <tag>.S.txt / .Vq.txt / .q.txt / .size.txt.  Every run has to end with exit status 0."""
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GEMMA = os.path.join(ROOT, "oracle", "_ref", "gemma")
TXT = os.path.join(ROOT, "tests", "golden", "text")
LOG_KEYS = ("pve estimates", "se(pve)", "total pve", "se(total pve)", "sigma2 estimates", "se(sigma2)", "sigma2 per snp",
            "se(sigma2 per snp)", "enrichment", "se(enrichment)")

CAT2, CAT3 = ["-cat", "mqs_cat2.txt"], ["-cat", "mqs_cat3.txt"]
COV = ["-c", "P.cov.txt"]
BETA, BETA_A1 = ["-beta", "mqs_beta.txt"], ["-beta", "ci_beta_a1.txt"]
PVE2, PVE3 = ["-pve", 0.3, 0.2], ["-pve", 0.25, 0.15, 0.1]
RUNS = [
    ("C1_2", CAT2 + BETA + ["-ref", "G2"] + PVE2 + ["-ci", 1]),
    ("C1_2c", COV + CAT2 + BETA + ["-ref", "G2"] + PVE2 + ["-ci", 1]),
    ("C1_2a", CAT2 + BETA_A1 + ["-ref", "G2"] + PVE2 + ["-ci", 1]),
    ("C2_2", CAT2 + ["-wcat", "ci_wcat2.txt"] + BETA + ["-ref", "G2"] + PVE2 + ["-ci", 2]),
    ("C1_3", CAT3 + BETA + ["-ref", "G3"] + PVE3 + ["-ci", 1]),
    ("C2_3c", COV + CAT3 + ["-wcat", "ci_wcat3.txt"] + BETA + ["-ref", "G3c"] + PVE3 + ["-ci", 2]),
    ("V2_2", CAT2 + ["-wcat", "ci_wcat2.txt"] + BETA + ["-vc", 2]),
    ("V2_3c", COV + CAT3 + ["-wcat", "ci_wcat3.txt"] + BETA + ["-vc", 2]),
]


def run(tmp, tag, args):
    cmd = [GEMMA, "-bfile", "P", "-p", "pheno.txt"] + [str(a) for a in args] + ["-o", tag]
    r = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("%s: exit %d\n%s" % (tag, r.returncode, r.stdout[-2000:]))
    meta = {}
    for line in open(os.path.join(tmp, "output", tag + ".log.txt")):
        for key in LOG_KEYS:
            if line.startswith("## " + key + " ="):
                meta[key] = line.split("=", 1)[1].split()
        if line.startswith("## number of"):
            k, v = line[2:].split("=", 1)
            meta[k.strip()] = v.strip()
    if "se(pve)" not in meta or any(v.lower().strip("-") == "nan" for v in meta["se(pve)"]):
        raise RuntimeError("%s: no finite se(pve) in the log" % tag)
    json.dump(meta, open(os.path.join(TXT, tag + ".log.json"), "w"), indent=1, sort_keys=True)
    if tag.startswith("V"):
        for suf in (".S.txt", ".Vq.txt", ".q.txt", ".size.txt"):
            shutil.copy(os.path.join(tmp, "output", tag + suf), os.path.join(TXT, tag + suf))


def main():
    tmp = tempfile.mkdtemp()
    try:
        for name in ("P.bed", "P.bim", "P.fam", "P.cov.txt", "mqs_cat2.txt", "mqs_cat3.txt", "mqs_beta.txt"):
            shutil.copy(os.path.join(TXT, name), tmp)
        for ref in ("G2", "G3", "G3c"):
            for suf in (".S.txt", ".size.txt"):
                shutil.copy(os.path.join(TXT, ref + suf), tmp)
        with open(os.path.join(tmp, "P.fam")) as f, open(os.path.join(tmp, "pheno.txt"), "w") as g:
            for line in f:
                v = line.split()[5]
                g.write(("NA" if v == "-9" else v) + "\n")
        bim = [l.split() for l in open(os.path.join(tmp, "P.bim")) if l.strip()]
        snps = [b[1] for b in bim]
        rng = np.random.default_rng(5)
        with open(os.path.join(TXT, "ci_wcat2.txt"), "w") as f:
            f.write("rs wA wB\n")
            for rs in snps:
                a = rng.uniform(1, 30)
                b = rng.uniform(0.5, 10)
                f.write("%s %.4f %.4f\n" % (rs, a, b))
        rng = np.random.default_rng(6)
        with open(os.path.join(TXT, "ci_wcat3.txt"), "w") as f:
            f.write("rs wA wB wC\n")
            for rs in snps:
                f.write("%s %.4f %.4f %.4f\n" % ((rs,) + tuple(rng.uniform(0.5, 20, size=3))))
        z = np.random.default_rng(20170601).standard_normal(len(snps)) * 1.4  # as make_mqs_fixtures.py
        with open(os.path.join(TXT, "ci_beta_a1.txt"), "w") as f:
            f.write("rs a1 z n_total\n")
            for t, b in enumerate(bim):
                if t % 20 != 7:
                    f.write("%s %s %.6f %d\n" % (b[1], b[4] if t % 3 != 0 else b[5], z[t], 154 - (t % 4)))
        for name in ("ci_wcat2.txt", "ci_wcat3.txt", "ci_beta_a1.txt"):
            shutil.copy(os.path.join(TXT, name), tmp)
        for tag, args in RUNS:
            run(tmp, tag, args)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

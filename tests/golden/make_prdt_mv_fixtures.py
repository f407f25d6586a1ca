"""Printed outputs of the reference binary's kinship-only prediction for SEVERAL phenotypes (-predict 1 with -k and -n a b c and
neither -epm nor -ebv: a_mode 43, the else branch of src/gemma.cpp:1821-1871 with PRDT::MvnormPrdt) for tests/test_prdt_mv_cpu.py
and tests/test_gpu_prdt_mv.py -- run in the build container only (oracle/_ref/gemma, see oracle/Makefile):

    python tests/golden/make_prdt_mv_fixtures.py

Inputs: tests/golden/prdt/Sb.geno.txt.gz, Sb.pheno.txt and Sb.cvt.txt (read, not changed) and Sb.pheno3.txt, written here into
tests/golden/prdt_mv/ from a fixed numpy seed: 300 x 3; column 1 is the Sb trait where it is observed and a draw of the same mean
and spread elsewhere; columns 2 and 3 are correlated with column 1; about 12 % of the entries are NA, scattered; individual 17 has
all three NA; individual 23 has exactly one trait (the second) observed.
The kinship is the reference's own -gk 1 of Sb (with Sb.pheno.txt, as tests/golden/make_prdt_fixtures.py runs it: the matrix
tests/prdtcases.py:kinship_all restates).  BIMBAM input only: with -bfile the reference's own CheckData refuses the run.
Runs, each recorded as <tag>.prdt.txt.gz and <tag>.log.json (the printed lower triangles of Vg and Ve, and the counts):
* Sb_mv2   -n 1 2
* Sb_mv3   -n 1 2 3
* Sb_mv2c  -n 1 2 -c Sb.cvt.txt
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
SRC = os.path.join(ROOT, "tests", "golden", "prdt")
OUT = os.path.join(ROOT, "tests", "golden", "prdt_mv")
RUNS = (("Sb_mv2", ["-n", 1, 2]), ("Sb_mv3", ["-n", 1, 2, 3]), ("Sb_mv2c", ["-n", 1, 2, "-c", "Sb.cvt.txt"]))


def run(tmp, *args):
    r = subprocess.run([GEMMA] + [str(a) for a in args], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("exit status %d\n%s" % (r.returncode, r.stdout[-2000:]))
    return r.stdout


def pheno3(path):
    tok = [l.split()[0] for l in open(os.path.join(SRC, "Sb.pheno.txt")) if l.strip()]
    obs = np.array([t != "NA" for t in tok])
    y1 = np.array([float(t) if t != "NA" else 0.0 for t in tok])
    rng = np.random.default_rng(20240915)
    n = len(tok)
    mu, sd = y1[obs].mean(), y1[obs].std()
    y1 = np.where(obs, y1, mu + sd * rng.standard_normal(n))
    z = (y1 - mu) / sd
    # a polygenic part of their own for traits 2 and 3 (60 SNPs each), so that every trait has a genetic variance to estimate
    with gzip.open(os.path.join(SRC, "Sb.geno.txt.gz"), "rt") as f:
        X = np.array([[np.nan if t == "NA" else float(t) for t in l.replace(",", " ").split()[3:]] for l in f if l.strip()])
    X = np.where(np.isnan(X), np.nanmean(X, axis=1, keepdims=True), X)
    X = X - X.mean(1, keepdims=True)
    g = []
    for _ in range(2):
        beta = np.zeros(X.shape[0])
        beta[rng.choice(X.shape[0], 60, replace=False)] = rng.standard_normal(60)
        v = X.T @ beta
        g.append(v / v.std())
    y2 = 1.0 + 0.5 * z + 0.7 * g[0] + 0.6 * rng.standard_normal(n)
    y3 = -2.0 - 0.4 * z + 0.3 * g[0] + 0.8 * g[1] + 0.7 * rng.standard_normal(n)
    Y = np.column_stack([y1, y2, y3])
    miss = rng.random((n, 3)) < 0.115
    miss[17] = True
    miss[23] = [True, False, True]
    with open(path, "w") as f:
        for i in range(n):
            f.write("\t".join("NA" if miss[i, a] else "%.6f" % Y[i, a] for a in range(3)) + "\n")


def lower_triangle(lines, k, d):
    return [[float(v) for v in lines[k + 1 + i].split()] for i in range(d)]


def main():
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp()
    try:
        with gzip.open(os.path.join(SRC, "Sb.geno.txt.gz"), "rt") as f, open(os.path.join(tmp, "Sb.geno.txt"), "w") as g:
            g.write(f.read())
        for name in ("Sb.pheno.txt", "Sb.cvt.txt"):
            shutil.copy(os.path.join(SRC, name), tmp)
        pheno3(os.path.join(OUT, "Sb.pheno3.txt"))
        shutil.copy(os.path.join(OUT, "Sb.pheno3.txt"), tmp)
        run(tmp, "-g", "Sb.geno.txt", "-p", "Sb.pheno.txt", "-gk", 1, "-o", "Sb_K")
        for tag, more in RUNS:
            out = run(tmp, "-g", "Sb.geno.txt", "-p", "Sb.pheno3.txt", *more, "-k", os.path.join("output", "Sb_K.cXX.txt"), "-predict", 1,
                      "-o", tag)
            lines = out.splitlines()
            d = sum(1 for a in more[1:] if isinstance(a, int))
            meta = {}
            for k, line in enumerate(lines):
                for key in ("Vg", "Ve"):
                    if line.startswith("REMLE estimate for %s in the null model:" % key):
                        meta[key] = lower_triangle(lines, k, d)
            for line in open(os.path.join(tmp, "output", tag + ".log.txt")):
                for key in ("number of individuals with full phenotypes", "number of observed data", "number of missing data",
                            "number of analyzed individuals", "number of covariates", "number of phenotypes"):
                    if line.startswith("## " + key + " ="):
                        meta[key] = line.split("=", 1)[1].strip()
            json.dump(meta, open(os.path.join(OUT, tag + ".log.json"), "w"), indent=1, sort_keys=True)
            with open(os.path.join(tmp, "output", tag + ".prdt.txt"), "rb") as f, \
                    gzip.GzipFile(os.path.join(OUT, tag + ".prdt.txt.gz"), "wb", mtime=0) as g:
                g.write(f.read())
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

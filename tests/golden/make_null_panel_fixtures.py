"""The null-model lines of the reference binary's log for three phenotype columns on one set of individuals, for
tests/test_null_panel_cpu.py and tests/test_gpu_null_panel.py -- run in the build container only (oracle/_ref/gemma, see
oracle/Makefile):

    python tests/golden/make_null_panel_fixtures.py

The set is Sb of tests/golden/prdt (BIMBAM genotypes of 300 individuals, 600 SNPs, 1 % missing calls) with its covariate file
Sb.cvt.txt (an intercept and one covariate).  This script writes a COMPLETE phenotype file of three columns from a fixed numpy seed
-- polygenic traits of heritability 0.3 / 0.5 / 0.7 on the set's own genotypes, each with an effect of the covariate -- to
tests/golden/null_panel/Sb3.pheno.txt, runs the reference's `-gk 1` and then `-lmm 4 -n t -c Sb.cvt.txt` for t = 1, 2, 3, and keeps of
each run the eight null-model values of its log (src/gemma.cpp:3402-3427) as tests/golden/null_panel/Sb_n<t>.log.json: REMLE and MLE
log-likelihood, pve, se(pve), vg, ve, beta and se(beta) -- strings as printed, beta and se(beta) as lists.  Every run must have
1e-2 < vg / ve < 1e2: the REML lambda lies inside the search interval and se(pve) is the curvature at a maximum."""
import gzip
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GEMMA = os.path.join(ROOT, "oracle", "_ref", "gemma")
FX = os.path.join(ROOT, "tests", "golden", "prdt")
OUT = os.path.join(ROOT, "tests", "golden", "null_panel")
H2S = (0.3, 0.5, 0.7)
KEYS = {"REMLE log-likelihood in the null model": "logl_remle_H0", "MLE log-likelihood in the null model": "logl_mle_H0",
        "pve estimate in the null model": "pve", "se(pve) in the null model": "pve_se", "vg estimate in the null model": "vg",
        "ve estimate in the null model": "ve", "beta estimate in the null model": "beta", "se(beta)": "se_beta"}


def run(tmp, *args):
    r = subprocess.run([GEMMA] + [str(a) for a in args], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError("exit status %d\n%s" % (r.returncode, r.stdout[-2000:]))
    return r.stdout


def phenotypes():
    rows = []
    with gzip.open(os.path.join(FX, "Sb.geno.txt.gz"), "rt") as f:
        for line in f:
            t = line.replace(",", " ").split()
            if t:
                rows.append([np.nan if x == "NA" else float(x) for x in t[3:]])
    G = np.array(rows)
    cov = np.array([[float(v) for v in l.split()] for l in open(os.path.join(FX, "Sb.cvt.txt")) if l.strip()])[:, 1]
    p, n = G.shape
    Gi = np.where(np.isnan(G), np.nanmean(G, axis=1, keepdims=True), G)
    Z = (Gi - Gi.mean(1, keepdims=True)) / np.maximum(Gi.std(1, keepdims=True), 1e-9)
    rng = np.random.default_rng(20261020)
    Y = np.empty((n, len(H2S)))
    for t, h2 in enumerate(H2S):
        gen = Z.T @ rng.standard_normal(p) / np.sqrt(p)
        Y[:, t] = 2.0 + t + np.sqrt(h2) * gen / gen.std() + np.sqrt(1.0 - h2) * rng.standard_normal(n) + (0.5 - 0.4 * t) * cov
    return np.round(Y, 6)


def main():
    os.makedirs(OUT, exist_ok=True)
    Y = phenotypes()
    pheno = os.path.join(OUT, "Sb3.pheno.txt")
    with open(pheno, "w") as f:
        for row in Y:
            f.write("\t".join("%.6f" % v for v in row) + "\n")
    tmp = tempfile.mkdtemp()
    try:
        with gzip.open(os.path.join(FX, "Sb.geno.txt.gz"), "rt") as f, open(os.path.join(tmp, "Sb.geno.txt"), "w") as g:
            g.write(f.read())
        for name in ("Sb.cvt.txt", "Sb.anno.txt"):
            shutil.copy(os.path.join(FX, name), tmp)
        shutil.copy(pheno, tmp)
        geno = ["-g", "Sb.geno.txt", "-p", "Sb3.pheno.txt"]
        run(tmp, *geno, "-gk", 1, "-o", "K")
        for t in (1, 2, 3):
            tag = "Sb_n%d" % t
            run(tmp, *geno, "-a", "Sb.anno.txt", "-c", "Sb.cvt.txt", "-k", os.path.join("output", "K.cXX.txt"), "-lmm", 4, "-n", t, "-o", tag)
            meta = {}
            for line in open(os.path.join(tmp, "output", tag + ".log.txt")):
                for key, name in KEYS.items():
                    if line.startswith("## " + key + " ="):
                        v = line.split("=", 1)[1].split()
                        meta[name] = v if name in ("beta", "se_beta") else v[0]
            assert sorted(meta) == sorted(KEYS.values()), meta
            ratio = float(meta["vg"]) / float(meta["ve"])
            assert 1e-2 < ratio < 1e2, (tag, ratio)
            json.dump(meta, open(os.path.join(OUT, tag + ".log.json"), "w"), indent=1, sort_keys=True)
            print(tag, meta)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

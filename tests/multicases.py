"""Data of the multi-phenotype LMM tests (tests/test_gpu_lmm_multi.py) and of tests/golden/make_multi_fixtures.py: a small PLINK
set with three complete phenotype columns, and trait panels on synthetic genotypes with a different heritability per trait."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_NPZ = os.path.join(ROOT, "tests", "golden", "ref_multi.npz")


def pack_bed(codes):
    """(p, ni) PLINK 2-bit codes (0 hom A1, 1 missing, 2 het, 3 hom A2) -> (p, ceil(ni / 4)) .bed payload rows"""
    p, ni = codes.shape
    pad = np.zeros((p, (ni + 3) // 4 * 4), dtype=np.uint8)
    pad[:, :ni] = codes
    return (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)


def plink_set(ni=150, ns=300, seed=20):
    """codes (ns, ni), phenotypes (ni, 3): polygenic traits of different heritability; every column complete."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.1, 0.5, size=ns)
    g = rng.binomial(2, maf[:, None], size=(ns, ni))
    codes = np.array([3, 2, 0], dtype=np.uint8)[g]  # the count of A1: 0 -> hom A2 (3), 1 -> het (2), 2 -> hom A1 (0)
    codes[rng.random(codes.shape) < 0.02] = 1
    z = (g - g.mean(axis=1, keepdims=True)) / np.maximum(g.std(axis=1, keepdims=True), 1e-9)
    pheno = np.empty((ni, 3))
    for t, h2 in enumerate((0.1, 0.5, 0.9)):
        gen = z.T @ rng.standard_normal(ns) / np.sqrt(ns)
        pheno[:, t] = np.sqrt(h2) * gen / gen.std() + np.sqrt(1 - h2) * rng.standard_normal(ni)
    return codes, np.round(pheno, 6)


def write_plink(prefix, codes, pheno):
    ns, ni = codes.shape
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(pack_bed(codes).tobytes())
    with open(prefix + ".bim", "w") as f:
        for s in range(ns):
            f.write("%d\trs%d\t0\t%d\tA\tG\n" % (1 + s * 4 // ns, s + 1, 1000 * (s + 1)))
    with open(prefix + ".fam", "w") as f:
        for i in range(ni):
            f.write("f%d i%d 0 0 1 %s\n" % (i + 1, i + 1, " ".join("%.6f" % v for v in pheno[i])))


def panel(oracle, n, p, c, h2s, seed, miss=0.01, dosage=False):
    """X (p, n) SNP-major with NaN, U, eval, UtW (n, c), UtY (n, T): trait t has heritability h2s[t] on the kinship of 600 further
    SNPs (h2 = 0: noise alone, lambda-hat at l_min for most SNPs; h2 near 1: lambda-hat large) -- the brackets of the traits differ."""
    rng = np.random.default_rng(seed)
    maf = rng.uniform(0.05, 0.5, size=p + 600)
    G = rng.binomial(2, maf[:, None], size=(p + 600, n)).astype(np.float64)
    if dosage:
        G[:p] = np.clip(G[:p] + rng.normal(0.0, 0.15, size=(p, n)), 0.0, 2.0)
    G[rng.random(G.shape) < miss] = np.nan
    K = oracle.calc_kin(G[p:], 1)
    U, ev, _ = oracle.eigen_decomp_zeroed(oracle.center_matrix(K))
    W = np.ones((n, 1)) if c == 1 else np.hstack([rng.standard_normal((n, c - 1)), np.ones((n, 1))])
    Gk = np.where(np.isnan(G[p:]), 0.0, G[p:])
    Z = (Gk - Gk.mean(axis=1, keepdims=True)) / np.maximum(Gk.std(axis=1, keepdims=True), 1e-9)
    Gi = np.where(np.isnan(G[:3]), 0.0, G[:3])
    Y = np.empty((n, len(h2s)))
    for t, h2 in enumerate(h2s):
        gen = Z.T @ rng.standard_normal(600) / np.sqrt(600.0)
        Y[:, t] = np.sqrt(h2) * gen / gen.std() + np.sqrt(1.0 - h2) * rng.standard_normal(n) + 0.2 * Gi.T @ rng.standard_normal(3)
    return np.ascontiguousarray(G[:p]), U, ev, U.T @ W, np.ascontiguousarray(U.T @ Y)

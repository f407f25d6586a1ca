"""Numpy restatements of GEMMA's variance-component fit (src/vc.cpp) and the inputs of the -vc fixtures
(tests/golden/text/V*.log.json, tests/golden/make_vc_fixtures.py), shared by tests/test_vc_cpu.py and tests/test_gpu_vc.py."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXT = os.path.join(ROOT, "tests", "golden", "text")


def center_matrix(G):
    """CenterMatrix(G), src/mathfunc.cpp:147-177: (I - 11^T/n) G (I - 11^T/n)."""
    n = G.shape[0]
    w = np.ones(n)
    Gw = G @ w
    G = G - np.outer(Gw, w) / n - np.outer(w, Gw) / n
    return G + (w @ Gw) / n ** 2 * np.outer(w, w)


def center_matrix_w(G, W):
    """CenterMatrix(G, W), src/mathfunc.cpp:205-247."""
    Q = W @ np.linalg.inv(W.T @ W)
    return G - (G @ W) @ Q.T - Q @ (W.T @ G) + Q @ (W.T @ G @ W) @ Q.T


def p_inputs(cov=False, snps=None):
    """The -vc fixtures' inputs on P: the .fam phenotype (-9 = NA); the reference's -gk 1 kinship of the SNPs in `snps` (a
    range; None = all): SNP filters on the 154 phenotyped individuals, kinship over all 240, written with 10 significant
    digits; centred by CenterMatrix(G) over the analysed individuals; W = intercept (+ P.cov.txt's two columns)."""
    from oracle import oracle as O
    raw, ni, ph, ind = O.read_bed(os.path.join(TXT, "P"))
    if snps is not None:
        raw = raw[snps[0]:snps[1]]
    G_test = O.bed_decode(raw, ni, ind)
    snp = O.qc_snps_bed(G_test, np.ones((int(ind.sum()), 1)))
    K = O.round10(O.calc_kin(O.bed_decode(raw[snp == 1], ni), 1))
    if cov:
        cvt, ind_c = O.read_cvt(os.path.join(TXT, "P.cov.txt"))
        sel, W = O.process_cvt_phen(ind, cvt, ind_c)
    else:
        sel, W = O.process_cvt_phen(ind)
    ix = np.flatnonzero(sel == 1)
    return center_matrix(K[np.ix_(ix, ix)]), W, ph[ix], K, ph, ind


def p_mk(cuts, cov=False):
    """-mk of P's kinships from the SNP ranges `cuts` (as tests/golden/make_vc_fixtures.py): (Ks, W, y)"""
    Ks = []
    for c in cuts:
        K, W, y, *_ = p_inputs(cov, c)
        Ks.append(K)
    return Ks, W, y


def bxd_mk(parts):
    """BXD (trait column 1, no covariates): the -gk 1 kinship of all SNPs (parts = 1) or of the two halves of the genotype
    file (parts = 2), SNP filters on the analysed individuals, centred by CenterMatrix(G): (Ks, W, y)"""
    import gzip
    from oracle import oracle as O
    _, G = O.read_bimbam_geno(os.path.join(TXT, "bxd_mean_genotypes.txt.gz"))
    with gzip.open(os.path.join(TXT, "bxd_trait.txt.gz"), "rt") as f:
        tok = [l.split()[0] for l in f if l.strip()]
    ind = np.array([0 if t == "NA" else 1 for t in tok], dtype=np.int32)
    y_all = np.array([np.nan if t == "NA" else float(t) for t in tok])
    sel, W = O.process_cvt_phen(ind)
    ix = np.flatnonzero(sel == 1)
    half = G.shape[0] // 2
    ranges = [(0, G.shape[0])] if parts == 1 else [(0, half), (half, G.shape[0])]
    Ks = []
    for lo, hi in ranges:
        snp = O.qc_snps(G[lo:hi], ind, W)[0]
        K = O.round10(O.calc_kin(G[lo:hi][snp == 1], 1))
        Ks.append(center_matrix(K[np.ix_(ix, ix)]))
    return Ks, W, y_all[ix]


HE_CASES = [("V1", lambda: p_mk([None])), ("V1c", lambda: p_mk([None], True)),
            ("V2c", lambda: p_mk([(0, 400), (400, 800)], True)), ("V3", lambda: p_mk([(0, 250), (250, 500), (500, 800)])),
            ("VB1", lambda: bxd_mk(1)), ("VB2", lambda: bxd_mk(2))]
HE_KEYS = (("sigma2", "sigma2"), ("se_sigma2", "se(sigma2)"), ("pve", "pve"), ("se_pve", "se(pve)"),
           ("pve_total", "total pve"), ("se_pve_total", "se(total pve)"))


def fixture(tag):
    return json.load(open(os.path.join(TXT, tag + ".log.json")))


def he(Ks, W, y):
    """VC::CalcVChe, src/vc.cpp:1503-1724."""
    n, nvc = len(y), len(Ks)
    r = n / (n - W.shape[1])
    traceG = [np.trace(K) / n for K in Ks]
    Kt, tnew = [], []
    for K in Ks:
        T = center_matrix_w(K, W)
        d = np.trace(T) / n
        tnew.append(d)
        Kt.append(T / d if d != 0 else T)
    ys = y - W @ np.linalg.solve(W.T @ W, W.T @ y)
    var_y, var_y_new = np.var(y), np.var(ys)
    ys = (ys - ys.mean()) / np.sqrt(np.var(ys))
    Kry = np.column_stack([K @ ys - r * ys for K in Kt])
    q = Kry.T @ ys
    S = np.array([[np.sum(Kt[i] * Kt[j]) - r * n for j in range(nvc)] for i in range(nvc)])
    Si = np.linalg.inv(S)
    pve = Si @ q
    qvar = sum(pve[l] * (Kry.T @ Kt[l] @ Kry) for l in range(nvc)) + (1 - pve.sum()) * (Kry.T @ Kry)
    Var = Si @ (2.0 * qvar) @ Si
    f = np.array([(var_y_new / tnew[i]) * (traceG[i] / var_y) for i in range(nvc)])
    sigma2 = np.append(pve * var_y_new / np.array(tnew), (1 - pve.sum()) * r * var_y_new)
    se_sigma2 = np.append(np.sqrt(np.diag(Var)) * var_y_new / np.array(tnew), np.sqrt(Var.sum()) * r * var_y_new)
    return dict(sigma2=sigma2, se_sigma2=se_sigma2, pve=pve * f, se_pve=np.sqrt(np.diag(Var)) * f, pve_total=(pve * f).sum(),
                se_pve_total=np.sqrt(f @ Var @ f))


def reml_dev(s2, Ks, W, y):
    """UpdateParam + LogRL_dev1 / LogRL_dev2 (src/vc.cpp:168-300) in sigma2 itself: dev1 = d logRL / d sigma2_i,
    AI = -0.5 y'P K_i P K_j P y (the reference's dev2 with noconstrain)."""
    n = len(y)
    Kall = list(Ks) + [np.eye(n)]
    H = sum(s * K for s, K in zip(s2, Kall))
    Hi = np.linalg.inv(H)
    HiW = Hi @ W
    P = Hi - HiW @ np.linalg.solve(W.T @ HiW, HiW.T)
    Py = P @ y
    KPy = np.column_stack([K @ Py for K in Kall])
    PKPy = P @ KPy
    dev1 = np.array([-0.5 * np.sum(P * K) + 0.5 * Py @ KPy[:, i] for i, K in enumerate(Kall)])
    dev2 = -0.5 * KPy.T @ PKPy
    return dev1, dev2


def reml_log_dev(x, Ks, W, y):
    """the reference's dev1 / dev2 on log sigma2 (the default, constrained form)"""
    s2 = np.exp(x)
    d1, d2 = reml_dev(s2, Ks, W, y)
    return d1 * s2, d2 * np.outer(s2, s2)


def reml_summary(s2, Ks, W, y, noconstrain=False):
    """se(sigma2), pve, se(pve), total (src/vc.cpp:1820-1918) at sigma2"""
    n, nvc = len(y), len(Ks)
    tg = np.array([np.trace(K) / n for K in Ks])
    if noconstrain:
        _, d2 = reml_dev(s2, Ks, W, y)
        Hi = np.linalg.inv(d2)
        se = np.sqrt(-np.diag(Hi))
        jac = np.ones(nvc + 1)
    else:
        _, d2 = reml_log_dev(np.log(s2), Ks, W, y)
        Hi = np.linalg.inv(d2)
        se = np.sqrt(-s2 * s2 * np.diag(Hi))
        jac = s2
    s = tg @ s2[:nvc] + s2[nvc]
    pve = tg * s2[:nvc] / s
    G = np.zeros((nvc + 1, nvc + 1))
    for k in range(nvc + 1):
        for i in range(nvc + 1):
            if k < nvc:
                g = tg[k] * (s - s2[k] * tg[k]) / s ** 2 if i == k else (
                    -tg[k] * s2[k] / s ** 2 if i == nvc else -tg[i] * tg[k] * s2[k] / s ** 2)
            else:
                g = -(s - s2[nvc]) / s ** 2 if i == k else tg[i] * s2[nvc] / s ** 2
            G[k, i] = g * jac[i]
    var = np.array([-(G[k] @ Hi @ G[k]) for k in range(nvc + 1)])
    return dict(se_sigma2=se, pve=pve, se_pve=np.sqrt(var[:nvc]), pve_total=pve.sum(), se_pve_total=np.sqrt(var[nvc]))

"""Numpy restatements of GEMMA's MQS path (PARAM::CalcS, src/param.cpp:1717-1812) and the inputs of the MQS fixtures
(tests/golden/text/G*.S.txt, Q*.S.txt, ...; tests/golden/make_mqs_fixtures.py), shared by tests/test_mqs_cpu.py and
tests/test_gpu_mqs.py:

* kin_ref       the weighted, covariate-residualised, category-partitioned kinship (PlinkKin, src/gemma_io.cpp:2947-3170);
* closed_form   compAKtoS + JackknifeAKtoS in their exact O(n^2) form, in any floating-point type;
* brute_force   the reference's own loops (src/param.cpp:1325-1378, :1596-1713) in np.longdouble: the loop over l as written, the
                updates of the n leave-one-out accumulators as vectors over t, the sums over k by numpy in long double.  n <= 200.
"""
import functools
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXT = os.path.join(ROOT, "tests", "golden", "text")
EPS = np.finfo(np.float64).eps


def decode_bed(raw, ni_total):
    """.bed rows -> doubles, NaN = missing (code b0 + 2 b1: 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing)"""
    raw = np.asarray(raw, dtype=np.uint8)
    codes = np.stack([(raw >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(raw.shape[0], -1)[:, :ni_total]
    return np.array([2.0, np.nan, 1.0, 0.0])[codes]


def encode_bed(G):
    """doubles in {0, 1, 2, NaN} -> .bed rows"""
    code = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    p, n = code.shape
    pad = np.full((p, (-n) % 4), 3, dtype=np.uint8)
    c4 = np.hstack([code, pad]).reshape(p, -1, 4)
    return (c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)


def kin_ref(G_test, W, cat, weight, n_vc):
    """G_test: p x ni_test with NaN.  -> (K (n_vc, n, n), not centred, divided by ns_c; ns).  A category without SNPs is zero.
    A SNP without any called genotype is dropped (the reference would fill its matrix with NaN)."""
    p, n = G_test.shape
    cat = np.asarray(cat)
    WtWi = np.linalg.inv(W.T @ W)
    miss = np.isnan(G_test)
    cnt = n - miss.sum(axis=1)
    live = (cat >= 0) & (cnt > 0)
    mean = np.where(miss, 0.0, G_test).sum(axis=1) / np.maximum(cnt, 1)
    X = np.where(miss, mean[:, None], G_test) - mean[:, None]
    X = X - ((X @ W) @ WtWi) @ W.T
    var = (X * X).sum(axis=1) / n
    live &= var != 0
    w = np.ones(p) if weight is None else np.asarray(weight, dtype=np.float64)
    X = X * np.sqrt(w / np.where(var != 0, var, 1.0))[:, None]
    K = np.zeros((n_vc, n, n))
    ns = np.zeros(n_vc)
    for c in range(n_vc):
        Xc = X[live & (cat == c)]
        ns[c] = Xc.shape[0]
        if Xc.shape[0]:
            K[c] = Xc.T @ Xc / ns[c]
    return K, ns


def center_scale(K):
    """CenterMatrix + ScaleMatrix (src/mathfunc.cpp:147-177, :271-286) of every matrix of K (n_vc, n, n)"""
    out = np.empty_like(K)
    for c in range(K.shape[0]):
        G = K[c]
        n = G.shape[0]
        Gw = G.sum(axis=1)
        G = G - Gw[:, None] / n - Gw[None, :] / n + Gw.sum() / n ** 2
        d = np.trace(G) / n
        out[c] = G * (1.0 / d) if d != 0 else G
    return out


def closed_form(A, K, c, dtype=np.float64):
    """(S, Svar) from the centred + scaled A, K (n_vc, n, n) by the O(n^2) form; every operation in `dtype`.  `A is K`: the pair
    (j, i) is the transpose of (i, j) and is copied from it."""
    same = A is K
    A = A.astype(dtype)
    K = A if same else K.astype(dtype)
    n_vc, n = A.shape[0], A.shape[1]
    nn = dtype(n)
    S, Svar = np.zeros((n_vc, n_vc), dtype=dtype), np.zeros((n_vc, n_vc), dtype=dtype)
    for i in range(n_vc):
        for j in range(n_vc):
            if same and j < i:
                S[i, j], Svar[i, j] = S[j, i], Svar[j, i]
                continue
            Ai, Kj = A[i], K[j]
            sA, sK, dA, dK = Ai.sum(axis=1), Kj.sum(axis=1), np.diag(Ai).copy(), np.diag(Kj).copy()
            SA, SK, trA, trK = sA.sum(), sK.sum(), dA.sum(), dK.sum()
            h = (Ai * Kj).sum(axis=1)
            u, v = Ai @ sK, Kj @ sA
            T, dot = h.sum(), sA @ sK
            tA, tK = trA - SA / nn, trK - SK / nn
            if tA == 0 or tK == 0:
                d = dtype(0)
            else:
                d = (T - 2 * dot / nn + (SA / nn) * (SK / nn)) / (tA * tK) - 1 / dtype(n - c)
            trAK_t = T - 2 * h + dA * dK
            sumA_t, sumK_t = (SA - 2 * sA + dA) / (nn - 1), (SK - 2 * sK + dK) / (nn - 1)
            sumAK_t = (dot - u - v + h - (sA - dA) * (sK - dK)) / (nn - 1)
            fa, fk = (trA - dA) - sumA_t, (trK - dK) - sumK_t
            ok = (fa != 0) & (fk != 0)
            den = np.where(ok, fa * fk, dtype(1))
            d_t = np.where(ok, (trAK_t - 2 * sumAK_t + sumA_t * sumK_t) / den - 1 / dtype(n - c - 1), dtype(0))
            m = d_t.sum() / nn
            Svar[i, j] = (nn - 1) * (((d_t - m) ** 2).sum() / nn)
            S[i, j] = nn * d - (nn - 1) * m if c == 1 else d
    return S, Svar


def brute_force(A, K, c):
    """compAKtoS followed by JackknifeAKtoS as the reference writes them, in np.longdouble (see the module docstring)."""
    R = np.longdouble
    A, K = A.astype(R), K.astype(R)
    n_vc, n = A.shape[0], A.shape[1]
    nn = R(n)
    S, Svar = np.zeros((n_vc, n_vc), dtype=R), np.zeros((n_vc, n_vc), dtype=R)
    # the per-matrix accumulators of JackknifeAKtoS (its first loop nest; the reference reads K_i there, as here)
    sumA, sumK, trA, trK, sA, sK = (np.zeros((n_vc, n), dtype=R) for _ in range(6))
    for i in range(n_vc):
        for l in range(n):
            for M, sumM, trM, sM in ((A[i], sumA, trA, sA), (K[i], sumK, trK, sK)):
                row = M[l]
                add = row.sum() - row  # every k except k == t ...
                add[l] = 0             # ... and nothing of row l for t == l
                sumM[i] += add
                tr = np.full(n, row[l], dtype=R)
                tr[l] = 0
                trM[i] += tr
                sM[i, l] = row.sum()
        sumA[i] /= nn - 1
        sumK[i] /= nn - 1
    for i in range(n_vc):
        for j in range(n_vc):
            # compAKtoS
            tr_AK = sum_AK = R(0)
            for l in range(n):
                tr_AK += (A[i, l] * K[j, l]).sum()
                sum_AK += A[i, l].sum() * K[j, l].sum()
            sum_A, sum_K = A[i].sum() / nn, K[j].sum() / nn
            sum_AK /= nn
            tr_A, tr_K = np.trace(A[i]) - sum_A, np.trace(K[j]) - sum_K
            d = tr_AK - 2 * sum_AK + sum_A * sum_K
            d = R(0) if (tr_A == 0 or tr_K == 0) else d / (tr_A * tr_K) - 1 / R(n - c)
            # JackknifeAKtoS
            trAK, sumAK = np.zeros(n, dtype=R), np.zeros(n, dtype=R)
            for l in range(n):
                prod = A[i, l] * K[j, l]
                add = prod.sum() - prod
                add[l] = 0
                trAK += add
                add = (sA[i, l] - A[i, l]) * (sK[j, l] - K[j, l])
                add[l] = 0
                sumAK += add
            sumAK /= nn - 1
            fa, fk = trA[i] - sumA[i], trK[j] - sumK[j]
            ok = (fa != 0) & (fk != 0)
            den = np.where(ok, fa * fk, R(1))
            d_t = np.where(ok, (trAK - 2 * sumAK + sumA[i] * sumK[j]) / den - 1 / R(n - c - 1), R(0))
            m = d_t.sum() / nn
            Svar[i, j] = (nn - 1) * (((d_t - m) ** 2).sum() / nn)  # around the mean: what mean(d^2) - m^2 means, without its cancellation
            S[i, j] = nn * d - (nn - 1) * m if c == 1 else d
    return S, Svar


def block_err(got, want):
    """worst relative error of a block (S or Svar) against a long-double reference; entries whose reference is 0 must be 0"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    nz = want != 0
    assert np.all(got[~nz] == 0)
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


# --------------------------------------------------------------------------------------------------------- fixture inputs
def read_matrix(path):
    return np.loadtxt(path, ndmin=2)


def fixture_S(tag):
    M = read_matrix(os.path.join(TXT, tag + ".S.txt"))
    n_vc = M.shape[1]
    size = np.loadtxt(os.path.join(TXT, tag + ".size.txt"))
    return M[:n_vc], M[n_vc:], size[:n_vc], int(size[n_vc])


def fixture_log(tag):
    return json.load(open(os.path.join(TXT, tag + ".log.json")))


CAT_FILE = {"2": "mqs_cat2.txt", "3": "mqs_cat3.txt"}
P_TAGS = ["G1", "G2", "G2c", "G3", "G3c", "Q2", "Q2c", "Q3", "Q3c"]
ALL_TAGS = P_TAGS + ["GB2"]


@functools.lru_cache(maxsize=None)
def case(tag):
    """Inputs of fixture `tag` as the device entry points take them: dict(kind 'plink' | 'bimbam', geno (rows of the analysed SNPs
    over all individuals), ni_total, indicator, W, cat, n_vc, rs, G_test (p x ni_test with NaN), mapRS2cat, beta (path or None))."""
    from gemma_amd import api
    from oracle import oracle as O
    if tag == "GB2":
        rs_all, G = O.read_bimbam_geno(os.path.join(TXT, "bxd_mean_genotypes.txt.gz"))
        with gzip.open(os.path.join(TXT, "bxd_trait.txt.gz"), "rt") as f:
            tok = [l.split()[0] for l in f if l.strip()]
        ind = np.array([0 if t == "NA" else 1 for t in tok], dtype=np.int32)
        # BimbamKinUncentered skips an individual that is not analysed BEFORE it takes the next token of the line
        # (src/gemma_io.cpp:2824-2828), so analysed individual j gets genotype column j: the reference's S of a BIMBAM file is
        # that of its first ni_test columns.  The fixture is the reference's number, so the case hands over that indicator.
        ind = np.array([1] * int(ind.sum()) + [0] * int((ind == 0).sum()), dtype=np.int32)
        W = np.ones((int(ind.sum()), 1))
        mapcat, n_vc = api.ReadFile_cat(os.path.join(TXT, "mqs_bcat2.txt"))
        kind, geno, ni, snps_tag, beta = "bimbam", G, G.shape[1], "GB2", None
    else:
        raw, ni, _, ind_ph = O.read_bed(os.path.join(TXT, "P"))
        rs_all = [l.split()[1] for l in open(os.path.join(TXT, "P.bim")) if l.strip()]
        if tag.endswith("c"):
            cvt, ind_c = O.read_cvt(os.path.join(TXT, "P.cov.txt"))
            ind, W = O.process_cvt_phen(ind_ph, cvt, ind_c)
        else:
            ind, W = O.process_cvt_phen(ind_ph)
        key = tag[1]
        mapcat, n_vc = api.ReadFile_cat(os.path.join(TXT, CAT_FILE[key])) if key in CAT_FILE else ({}, 1)
        kind, geno, snps_tag = "plink", raw, "G" + tag[1:]
        beta = os.path.join(TXT, "mqs_beta.txt") if tag[0] == "Q" else None
    with gzip.open(os.path.join(TXT, snps_tag + ".snps.txt.gz"), "rt") as f:
        analysed = set(f.read().split())
    in_beta = None
    if beta:
        in_beta = set(l.split()[0] for l in open(beta).read().splitlines()[1:] if l.strip())
    keep = [t for t, r in enumerate(rs_all) if r in analysed and (in_beta is None or r in in_beta)]
    if beta:  # UpdateSNP after ObtainWeight, src/gemma.cpp:2114-2116: a SNP outside every category leaves indicator_snp too
        keep = [t for t in keep if not mapcat or rs_all[t] in mapcat]
    rs = [rs_all[t] for t in keep]
    cat = np.array([(mapcat.get(r, -1) if mapcat else 0) for r in rs], dtype=np.int32)
    geno = np.ascontiguousarray(geno[keep])
    full = decode_bed(geno, ni) if kind == "plink" else geno
    return dict(kind=kind, geno=geno, ni_total=ni, indicator=np.ascontiguousarray(ind, dtype=np.int32), W=np.ascontiguousarray(W),
                cat=cat, n_vc=n_vc, rs=rs, G_test=full[:, ind != 0], mapRS2cat=mapcat, beta=beta)


@functools.lru_cache(maxsize=None)
def case_ref(tag):
    """numpy: (K centred + scaled, S, Svar, ns) of fixture `tag`"""
    c = case(tag)
    K, ns = kin_ref(c["G_test"], c["W"], c["cat"], None, c["n_vc"])
    K = center_scale(K)
    S, Svar = closed_form(K, K, c["W"].shape[1])
    return K, S, Svar, ns


def q_inputs(tag):
    """Calcq's inputs of a Q fixture, as src/gemma.cpp:2110-2162 forms them -> (vec dict of ReadFile_beta, n_block = 200)"""
    from gemma_amd import api
    c = case(tag)
    in_beta = set(l.split()[0] for l in open(c["beta"]).read().splitlines()[1:] if l.strip())
    w = api.ObtainWeight(c["rs"], in_beta, c["mapRS2cat"])
    return api.ReadFile_beta(c["beta"], c["mapRS2cat"], w), 200


# --------------------------------------------------------------------------------------------------------- synthetic sets
def synth_geno(rng, p, n, miss=0.02, maf_lo=0.1):
    f = rng.uniform(maf_lo, 0.5, size=p)
    G = rng.binomial(2, f[:, None], size=(p, n)).astype(np.float64)
    G[rng.random((p, n)) < miss] = np.nan
    return G


@functools.lru_cache(maxsize=None)
def synth_AK(n, c):
    """A != K on n individuals, n_vc = 3 with category 1 empty, c covariates: (A, K) centred + scaled"""
    rng = np.random.default_rng(1000 * n + c)
    p = 240
    G = synth_geno(rng, p, n)
    W = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
    cat = rng.choice([0, 2], size=p).astype(np.int32)
    K, _ = kin_ref(G, W, cat, None, 3)
    A, _ = kin_ref(G, W, cat, rng.uniform(0.3, 3.0, size=p), 3)
    return center_scale(A), center_scale(K)


@functools.lru_cache(maxsize=None)
def synth_errors(n, c):
    """(S_ld, Svar_ld, err_S, err_Svar): the long-double brute force on synth_AK(n, c) and the float64 closed form's worst relative
    error per block against it"""
    A, K = synth_AK(n, c)
    S_ld, V_ld = brute_force(A, K, c)
    S, V = closed_form(A, K, c)
    return S_ld, V_ld, block_err(S, S_ld), block_err(V, V_ld)


def bar16(err, n):
    """the device's bar per block: 16 x max(the float64 numpy error on the same inputs, 64 n eps)"""
    return 16.0 * max(err, 64.0 * n * EPS)

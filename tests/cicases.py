"""Numpy restatements of GEMMA's MQS confidence intervals (-ci 1 / -ci 2, src/gemma.cpp:2400-2554) and of the LDSC reweighting
of -vc 2 -beta (:2182-2212), shared by tests/test_ci_cpu.py and tests/test_gpu_ci.py:

* moments / pass1 / pass2   the two genotype passes (PlinkXwz, PlinkXtXwz, src/vc.cpp:2314-2437, :2568-2688) from decoded
                            genotypes, in any floating-point type, with the sums of absolute terms the error model needs;
* calc_ciss                 CalcCIss (src/vc.cpp:2727-2950) in any floating-point type;
* update_weight             PARAM::UpdateWeight (src/param.cpp:2300-2349) in any floating-point type.

Error model of the device passes: an entry that is a sum of L terms whose absolute values add up to T is
within (L + 8) 2^-53 T of the long-double value -- L roundings of the sum in any order, at most 8 more from mu, var, sqrt, the
division and the scaling.  For pass 2, L = n.  Pass 2 is held against the long-double product with the XWz it was given (the
float64 matrix pass 1 returned), so that its bar speaks of its own sums alone."""
import functools
import json
import os

import numpy as np

from mqscases import TXT, bar16, decode_bed, encode_bed, synth_geno  # noqa: F401  (re-exported for the tests)

U = 2.0 ** -53
R = np.longdouble


def moments(G, dtype=R):
    """G: p x n over the analysed individuals, NaN = missing -> (mu, isd = 1 / sqrt(var), skipped, X = g - mu with 0 where missing).
    A SNP without a called genotype or with var == 0 is skipped: mu = isd = 0 and a zero row of X."""
    G = np.asarray(G)
    p, n = G.shape
    miss = np.isnan(G)
    g = np.where(miss, 0.0, G).astype(dtype)
    cnt = (n - miss.sum(axis=1)).astype(dtype)
    some = cnt > 0
    mu = np.where(some, g.sum(axis=1) / np.where(some, cnt, 1), 0)
    var = ((g * g).sum(axis=1) + mu * mu * (dtype(n) - cnt)) / dtype(n) - mu * mu
    live = some & (var > 0)
    isd = np.where(live, 1 / np.sqrt(np.where(live, var, 1)), 0).astype(dtype)
    X = np.where(miss | ~live[:, None], 0, g - mu[:, None]).astype(dtype)
    return np.where(live, mu, 0).astype(dtype), isd, ~live, X


def pass1(G, cat, z, w, n_vc, dtype=R):
    """-> dict(Xz, XWz (n x n_vc), T_z, T_w (sums of the absolute terms), L (terms per column), skipped (p bools))"""
    mu, isd, skipped, X = moments(G, dtype)
    cat = np.asarray(cat)
    a = np.asarray(z).astype(dtype) * isd
    ww = np.ones(len(cat), dtype=dtype) if w is None else np.asarray(w).astype(dtype)
    n = X.shape[1]
    out = {k: np.zeros((n, n_vc), dtype=dtype) for k in ("Xz", "XWz", "T_z", "T_w")}
    L = np.zeros(n_vc, dtype=np.int64)
    for c in range(n_vc):
        rows = (cat == c) & ~skipped
        L[c] = int(rows.sum())
        terms = X[rows] * a[rows, None]
        out["Xz"][:, c] = terms.sum(axis=0)
        out["T_z"][:, c] = np.abs(terms).sum(axis=0)
        terms = terms * ww[rows, None]
        out["XWz"][:, c] = terms.sum(axis=0)
        out["T_w"][:, c] = np.abs(terms).sum(axis=0)
    out["L"], out["skipped"] = L, skipped
    return out


def pass2(G, XWz, dtype=R):
    """-> (XtXWz (p x n_vc), T (sums of the absolute terms)) for the XWz given"""
    mu, isd, skipped, X = moments(G, dtype)
    B = np.asarray(XWz).astype(dtype)
    return (X @ B) * isd[:, None], (np.abs(X) @ np.abs(B)) * isd[:, None]


def check_pass1(got_Xz, got_XWz, ref):
    """every entry within (L + 8) 2^-53 T; -> the worst ratio error / bar, for the report"""
    worst = 0.0
    for got, key, tk in ((got_Xz, "Xz", "T_z"), (got_XWz, "XWz", "T_w")):
        err = np.abs(np.asarray(got).astype(R) - ref[key])
        bar = (ref["L"][None, :] + 8) * R(U) * ref[tk]
        assert np.all(err <= bar), (key, float((err - bar).max()))
        nz = bar > 0
        if nz.any():
            worst = max(worst, float((err[nz] / bar[nz]).max()))
    return worst


def check_pass2(got, G, XWz_given, skipped):
    want, T = pass2(G, XWz_given)
    n = G.shape[1]
    err = np.abs(np.asarray(got).astype(R) - want)
    bar = (n + 8) * R(U) * T
    assert np.all(err <= bar), float((err - bar).max())
    assert not np.asarray(got)[skipped].any()  # the rows of the skipped SNPs are exactly 0
    nz = bar > 0
    return float((err[nz] / bar[nz]).max()) if nz.any() else 0.0


# --------------------------------------------------------------------------------------------------------- CalcCIss, UpdateWeight
def small_inv(S, dtype):
    """Gauss-Jordan with partial pivoting in `dtype` (np.linalg.inv has no long double)"""
    n = S.shape[0]
    M = np.hstack([S.astype(dtype), np.eye(n, dtype=dtype)])
    for k in range(n):
        p = k + int(np.argmax(np.abs(M[k:, k])))
        M[[k, p]] = M[[p, k]]
        M[k] = M[k] / M[k, k]
        for r in range(n):
            if r != k:
                M[r] = M[r] - M[r, k] * M[k]
    return M[:, n:]


def calc_ciss(Xz, XWz, XtXWz, S_mat, Svar_mat, w, z, s_vec, vec_cat, v_pve, dtype=np.float64):
    """src/vc.cpp:2727-2950, line for line, every operation in `dtype`"""
    f = lambda v: np.asarray(v).astype(dtype)  # noqa: E731
    Xz, XWz, XtXWz, S_mat, Svar_mat, w, z, s_vec, v_pve = map(f, (Xz, XWz, XtXWz, S_mat, Svar_mat, w, z, s_vec, v_pve))
    vec_cat = np.asarray(vec_cat, dtype=np.int64)
    ni_test, n_vc = XWz.shape
    one = dtype(1)
    zwz, zz = np.zeros(n_vc, dtype=dtype), np.zeros(n_vc, dtype=dtype)
    for c in range(n_vc):
        m = vec_cat == c
        zwz[c] = (w[m] * z[m] * z[m]).sum()
        zz[c] = (z[m] * z[m]).sum()
    s_pve, s_snp = v_pve.sum(), s_vec.sum()
    Xz_pve = Xz @ (v_pve / s_vec)
    w_pve = (v_pve / s_vec)[vec_cat]
    s0 = one - s_pve + (zz * v_pve / s_vec).sum()
    qvar = np.zeros((n_vc, n_vc), dtype=dtype)
    for i in range(n_vc):
        s1 = s0 - zwz[i] * (one - s_pve) / s_vec[i]
        WXtXWz = XtXWz[:, i] * w_pve
        s1 = s1 - (Xz_pve @ XWz[:, i]) / s_vec[i]
        for j in range(n_vc):
            s = s1 - zwz[j] * (one - s_pve) / s_vec[j]
            s = s + (WXtXWz @ XtXWz[:, j]) / (s_vec[i] * s_vec[j])
            s = s + (XWz[:, i] @ XWz[:, j]) / (s_vec[i] * s_vec[j]) * (one - s_pve)
            s = s - (Xz_pve @ XWz[:, j]) / s_vec[j]
            qvar[i, j] = s
    d = dtype(ni_test - 1)
    qvar = qvar * (dtype(2) / (d * d * d))
    Si = small_inv(S_mat, dtype)
    Var = np.zeros((n_vc, n_vc), dtype=dtype)
    for i in range(n_vc):
        for j in range(i, n_vc):
            Var[i, j] = Var[j, i] = Svar_mat[i, j] * (v_pve[i] * v_pve[j]) + qvar[i, j]
    Var = (Si @ Var) @ Si
    sigma2 = v_pve / s_vec
    enrich = v_pve / s_vec * s_snp / s_pve
    se_pve = np.sqrt(np.diag(Var))
    T = np.zeros((n_vc, n_vc), dtype=dtype)
    for i in range(n_vc):
        dd, d1 = v_pve[i] / s_pve, s_vec[i]
        for j in range(n_vc):
            T[i, j] = ((one - dd) if i == j else (-one * dd)) / d1 * s_snp / s_pve
    se_enrich = np.sqrt(np.diag((T @ Var) @ T.T))
    return dict(pve=v_pve, se_pve=se_pve, pve_total=s_pve, se_pve_total=np.sqrt(Var.sum()), sigma2=sigma2, se_sigma2=se_pve / s_vec,
                enrich=enrich, se_enrich=se_enrich)


def update_weight(pve_flag, rs_list, cat, wcat, ni_test, ns, v_pve, dtype=np.float64):
    """src/param.cpp:2300-2349: rs_list in the order of the map (sorted), cat[rs] per SNP (0 without categories), wcat n x n_vc"""
    wcat, ns, v_pve = np.asarray(wcat).astype(dtype), np.asarray(ns).astype(dtype), np.asarray(v_pve).astype(dtype)
    cat = np.asarray(cat, dtype=np.int64)
    n_vc = len(v_pve)
    d = np.ones(len(rs_list), dtype=dtype)
    for i in range(n_vc):
        if v_pve[i] >= 1 and pve_flag == 1:
            d = d + dtype(ni_test) / ns[i] * wcat[:, i]
        elif v_pve[i] <= 0 and pve_flag == 1:
            pass
        else:
            d = d + dtype(ni_test) / ns[i] * wcat[:, i] * v_pve[i]
    wA = 1 / (d * d)
    for c in range(n_vc):
        m = cat == c
        if m.any():
            wA[m] = wA[m] / (wA[m].sum() / dtype(m.sum()))
    return wA


# --------------------------------------------------------------------------------------------------------- synthetic sets
@functools.lru_cache(maxsize=None)
def synth(n_vc, ni_total=1030, n_drop=71, p=523, miss=0.02):
    """The synthetic set of the device tests: dict(G (p x ni_total with NaN), bed, indicator, G_test, cat, z, w, special).
    SNP 17 has no called genotype among the analysed individuals, SNP 230 is monomorphic there, SNP 411 has a single called
    genotype (so var == 0 as well: its mean is that genotype), SNP 300 is a singleton (one heterozygote, everybody called): the
    first three are skipped, the fourth is not.  The individuals outside the analysis keep ordinary calls in all four."""
    rng = np.random.default_rng(7000 + n_vc + ni_total)
    ind = np.ones(ni_total, dtype=np.int32)
    ind[rng.choice(ni_total, n_drop, replace=False)] = 0
    an = np.flatnonzero(ind)
    G = synth_geno(rng, p, ni_total, miss=miss)
    special = dict(all_missing=17 % p, monomorphic=230 % p, single_call=411 % p, singleton=300 % p)
    G[special["all_missing"], an] = np.nan
    G[special["monomorphic"], an] = np.where(np.isnan(G[special["monomorphic"], an]), np.nan, 1.0)
    G[special["single_call"], an] = np.nan
    G[special["single_call"], an[5]] = 2.0
    G[special["singleton"], an] = 0.0
    G[special["singleton"], an[11]] = 1.0
    if n_vc == 3:
        cat = rng.choice([0, 2], size=p).astype(np.int32)  # category 1 is empty
    else:
        cat = rng.integers(0, n_vc, size=p).astype(np.int32)
    z = rng.standard_normal(p) * 1.5
    w = rng.uniform(0.5, 20.0, size=p)
    return dict(G=G, bed=encode_bed(G), indicator=ind, G_test=np.ascontiguousarray(G[:, an]), cat=cat, z=z, w=w, special=special,
                n_vc=n_vc)


@functools.lru_cache(maxsize=None)
def synth_ref(n_vc, weighted):
    """long-double pass 1 of synth(n_vc), computed once"""
    c = synth(n_vc)
    return pass1(c["G_test"], c["cat"], c["z"], c["w"] if weighted else None, n_vc)


def fixture_log(tag):
    return json.load(open(os.path.join(TXT, tag + ".log.json")))


# --------------------------------------------------------------------------------------------------------- fixture runs
LOG_KEYS_CI = ("pve estimates", "se(pve)", "total pve", "se(total pve)", "sigma2 per snp", "se(sigma2 per snp)", "enrichment",
               "se(enrichment)")
LOG_KEYS_VC = ("pve estimates", "se(pve)", "total pve", "se(total pve)", "sigma2 estimates", "se(sigma2)", "enrichment", "se(enrichment)")
API_KEYS = ("pve", "se_pve", "pve_total", "se_pve_total", "sigma2", "se_sigma2", "enrich", "se_enrich")
# tag -> the switches of tests/golden/make_ci_fixtures.py; snps: the -gs fixture with the same individuals and categories, whose
# .snps.txt.gz lists the SNPs that pass the reference's filters
RUNS = {
    "C1_2": dict(cat="mqs_cat2.txt", cov=False, beta="mqs_beta.txt", wcat=None, ref="G2", pve=[0.3, 0.2], ci=1, snps="G2"),
    "C1_2c": dict(cat="mqs_cat2.txt", cov=True, beta="mqs_beta.txt", wcat=None, ref="G2", pve=[0.3, 0.2], ci=1, snps="G2c"),
    "C1_2a": dict(cat="mqs_cat2.txt", cov=False, beta="ci_beta_a1.txt", wcat=None, ref="G2", pve=[0.3, 0.2], ci=1, snps="G2"),
    "C2_2": dict(cat="mqs_cat2.txt", cov=False, beta="mqs_beta.txt", wcat="ci_wcat2.txt", ref="G2", pve=[0.3, 0.2], ci=2, snps="G2"),
    "C1_3": dict(cat="mqs_cat3.txt", cov=False, beta="mqs_beta.txt", wcat=None, ref="G3", pve=[0.25, 0.15, 0.1], ci=1, snps="G3"),
    "C2_3c": dict(cat="mqs_cat3.txt", cov=True, beta="mqs_beta.txt", wcat="ci_wcat3.txt", ref="G3c", pve=[0.25, 0.15, 0.1], ci=2,
                  snps="G3c"),
    "V2_2": dict(cat="mqs_cat2.txt", cov=False, beta="mqs_beta.txt", wcat="ci_wcat2.txt", snps="G2"),
    "V2_3c": dict(cat="mqs_cat3.txt", cov=True, beta="mqs_beta.txt", wcat="ci_wcat3.txt", snps="G3c"),
}
CI_TAGS = [t for t in RUNS if t[0] == "C"]
VC_TAGS = [t for t in RUNS if t[0] == "V"]


@functools.lru_cache(maxsize=None)
def case(tag):
    """What the reference holds when it reaches the -ci / -vc 2 block of src/gemma.cpp for run `tag`: dict(bed (rows of the
    analysed SNPs), rs, a_minor, indicator, W, ni_test, mapRS2cat, n_vc, mapRS2wcat, mapRS2wK, beta (path), run)."""
    import gzip
    from gemma_amd import api
    from oracle import oracle as O
    r = RUNS[tag]
    raw, ni, _, ind_ph = O.read_bed(os.path.join(TXT, "P"))
    bim = [l.split() for l in open(os.path.join(TXT, "P.bim")) if l.strip()]
    if r["cov"]:
        cvt, ind_c = O.read_cvt(os.path.join(TXT, "P.cov.txt"))
        ind, W = O.process_cvt_phen(ind_ph, cvt, ind_c)
    else:
        ind, W = O.process_cvt_phen(ind_ph)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    mapcat, n_vc = api.ReadFile_cat(os.path.join(TXT, r["cat"]))
    mapwcat = api.ReadFile_wcat(os.path.join(TXT, r["wcat"]), n_vc) if r["wcat"] else None
    with gzip.open(os.path.join(TXT, r["snps"] + ".snps.txt.gz"), "rt") as f:
        analysed = set(f.read().split())
    rows = [t for t, b in enumerate(bim) if b[1] in analysed]
    rs = [bim[t][1] for t in rows]
    beta = os.path.join(TXT, r["beta"])
    in_beta = set(l.split()[0] for l in open(beta).read().splitlines()[1:] if l.strip())
    wK = api.ObtainWeight(rs, in_beta, mapcat, mapwcat)
    return dict(bed=np.ascontiguousarray(raw[rows]), rs=rs, a_minor=[bim[t][4] for t in rows], indicator=ind, W=np.ascontiguousarray(W),
                ni_total=ni, ni_test=int(ind.sum()), mapRS2cat=mapcat, n_vc=n_vc, mapRS2wcat=mapwcat, mapRS2wK=wK, beta=beta, run=r)


def ci_inputs(tag):
    """src/gemma.cpp:2416-2475 -> dict(bed rows of the SNPs UpdateSNPnZ keeps, w, z, vec_cat, s_vec, S, Svar, pve, w_pass: the w of
    pass 1 (None for -ci 1))"""
    from gemma_amd import api
    c = case(tag)
    r, n_vc = c["run"], c["n_vc"]
    wK = c["mapRS2wK"]
    s_vec = np.zeros(n_vc)
    for rs in wK:
        s_vec[c["mapRS2cat"][rs]] += 1
    if r["ci"] == 1:
        wA = {rs: 1.0 for rs in wK}
    else:
        wA = api.UpdateWeight(0, wK, c["ni_test"], s_vec, r["pve"], c["mapRS2wcat"], c["mapRS2cat"])
    A1, zmap = api.ReadFile_beta_z(c["beta"], wA)
    keep, w, z, vec_cat = api.UpdateSNPnZ(c["rs"], c["a_minor"], wA, A1, zmap, c["mapRS2cat"])
    S, Svar, _, _ = api.ReadFile_ref(os.path.join(TXT, r["ref"]))
    return dict(bed=np.ascontiguousarray(c["bed"][keep]), w=w, z=z, vec_cat=vec_cat, s_vec=s_vec, S=S, Svar=Svar, pve=np.array(r["pve"]),
                w_pass=None if r["ci"] == 1 else w)


def numpy_passes(c, x, dtype=np.float64):
    """the two passes of ci_inputs x on case c from the decoded genotypes"""
    G = decode_bed(x["bed"], c["ni_total"])[:, c["indicator"] != 0]
    p1 = pass1(G, x["vec_cat"], x["z"], x["w_pass"], c["n_vc"], dtype)
    return p1["Xz"], p1["XWz"], pass2(G, p1["XWz"], dtype)[0]


def check_log(est, tag, keys):
    log = fixture_log(tag)
    for key, k in zip(keys, API_KEYS):
        np.testing.assert_allclose(np.atleast_1d(est[k]).astype(np.float64), [float(v) for v in log[key]], rtol=5e-6, atol=0,
                                   err_msg="%s: %s" % (tag, key))


def vc2_chain(tag, calc_S):
    """The a_mode 62 loop of src/gemma.cpp:2102-2220 with -beta: calc_S(case, bed rows, cat, weight or None, slot) -> (S, Svar, ns)
    stands for PARAM::CalcS (slot 0: K, and A = K; slot 2: A beside the kept K and on top of it -- PlinkKin adds to the matrix it is
    handed, src/gemma_io.cpp:3103-3137, and the second CalcS hands it the centred + scaled A of the first).
    -> (est, S (2 n_vc x n_vc), Vq, q, size)"""
    from gemma_amd import api
    c = case(tag)
    n_vc, mapcat, wK = c["n_vc"], c["mapRS2cat"], c["mapRS2wK"]
    keep = np.array([rs in wK for rs in c["rs"]])  # UpdateSNP, src/gemma.cpp:2116
    bed = np.ascontiguousarray(c["bed"][keep])
    rs = [r for r, k in zip(c["rs"], keep) if k]
    cat = np.array([mapcat[r] for r in rs], dtype=np.int32)
    b = api.ReadFile_beta(c["beta"], mapcat, wK)
    Vq, q, _ = api.Calcq(200, b["vec_cat"], b["vec_ni"], b["vec_weight"], b["vec_z2"], n_vc)
    S, Svar, ns = calc_S(c, bed, cat, None, 0)
    est = api.CalcVCss(Vq, S, Svar, q, ns, b["ni_total"])
    wA = api.UpdateWeight(1, wK, b["ni_total"], ns, est["pve"], c["mapRS2wcat"], mapcat)
    b = api.ReadFile_beta(c["beta"], mapcat, wA)
    Vq, q, _ = api.Calcq(200, b["vec_cat"], b["vec_ni"], b["vec_weight"], b["vec_z2"], n_vc)
    S, Svar, ns = calc_S(c, bed, cat, np.array([wA[r] for r in rs]), 2)
    est = api.CalcVCss(Vq, S, Svar, q, ns, b["ni_total"])
    return est, np.vstack([S, Svar]), Vq, q, np.append(ns, c["ni_test"])


def check_vc2_files(tag, S2, Vq, q, size):
    rd = lambda suf: np.loadtxt(os.path.join(TXT, tag + suf), ndmin=2)  # noqa: E731
    np.testing.assert_allclose(S2, rd(".S.txt"), rtol=1e-9, atol=0)
    np.testing.assert_allclose(Vq, rd(".Vq.txt"), rtol=1e-9, atol=0)
    np.testing.assert_allclose(q, rd(".q.txt").ravel(), rtol=1e-9, atol=0)
    assert np.array_equal(size, rd(".size.txt").ravel())

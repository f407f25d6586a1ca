"""Numpy restatements of GEMMA's ridge / BLUP fit (-bslmm 2, src/bslmm.cpp:1194-1221 with the genotype reader of
src/gemma_io.cpp:1956-2084 / :1742-1845) and of -predict (src/prdt.cpp), the inputs of the prediction fixtures
(tests/golden/prdt, tests/golden/make_prdt_fixtures.py) and the derived error bounds of the two genotype matrix-vector
kernels -- shared by tests/test_prdt_cpu.py and tests/test_gpu_prdt.py."""
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TXT = os.path.join(ROOT, "tests", "golden", "text")
FX = os.path.join(ROOT, "tests", "golden", "prdt")
RTOL_PRINTED = 5e-6  # the project's bound for numbers printed with six significant digits (tests/test_gpu_vc.py)
EPS = np.finfo(np.float64).eps
SETS = ("P", "B", "S", "Sb")


# ------------------------------------------------------------------------------------------------ 2-bit rows
def bed_pack(G):
    """SNP-major doubles (NaN = missing, values 0 / 1 / 2) -> .bed rows: code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing; individual i
    in bits 2 (i % 4) of byte i / 4 (src/gemma_io.cpp:2026-2041)"""
    p, n = G.shape
    code = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    c4 = np.hstack([code, np.zeros((p, (-n) % 4), dtype=np.uint8)]).reshape(p, -1, 4)
    return np.ascontiguousarray(c4[:, :, 0] | (c4[:, :, 1] << 2) | (c4[:, :, 2] << 4) | (c4[:, :, 3] << 6)).astype(np.uint8)


def bed_unpack(rows, ni_total):
    rows = np.asarray(rows, dtype=np.uint8)
    code = np.stack([(rows >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(rows.shape[0], -1)[:, :ni_total]
    return np.array([2.0, np.nan, 1.0, 0.0])[code]


# ------------------------------------------------------------------------------------------------ the four pieces in numpy
def centred_rows(G, ind=None):
    """The columns ReadFile_bed / ReadFile_geno hand over as UtX (before the rotation), SNP-major: over the analysed
    individuals, g - mean of the non-missing analysed calls, a missing call 0.  An all-missing SNP is all zero."""
    Ga = G if ind is None else G[:, np.asarray(ind) != 0]
    miss = np.isnan(Ga)
    cnt = (~miss).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(miss, 0.0, Ga).sum(1) / cnt
    return np.where(miss, 0.0, Ga - mean[:, None])


def xtr(G, r, ind=None):
    """(X_c' r, the componentwise bound 4 n eps sum_i |xc_si| |r_i| of an fp64 dot product of length n in any order)"""
    Xc = centred_rows(G, ind)
    return Xc @ r, 4 * Xc.shape[1] * EPS * (np.abs(Xc) @ np.abs(r))


def prdt_rows(G, ind):
    """PRDT::AnalyzePlink / AnalyzeBimbam per SNP, SNP-major over the test individuals: (x~ rows, used).  x_train_mean = 0 / 0 =
    NaN where no training call is there (src/prdt.cpp:283, :420)."""
    ind = np.asarray(ind)
    Gt, Gp = G[:, ind != 0], G[:, ind == 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        tm = np.where(np.isnan(Gt), 0.0, Gt).sum(1) / (~np.isnan(Gt)).sum(1)
        cnt = (~np.isnan(Gp)).sum(1)
        xm = np.where(np.isnan(Gp), 0.0, Gp).sum(1) / cnt
        X = np.where(np.isnan(Gp), (xm - tm)[:, None], Gp - tm[:, None])
    return X, cnt > 0


def xw(G, w, ind):
    """(X~ w over the used SNPs, used, the bound 4 l eps sum_s |x~_st| |w_s|)"""
    X, used = prdt_rows(G, ind)
    Xu, wu = X[used], np.asarray(w)[used]
    with np.errstate(invalid="ignore"):
        y = (Xu * wu[:, None]).sum(0) if Xu.size else np.zeros(X.shape[1])
        b = 4 * max(int(used.sum()), 1) * EPS * (np.abs(Xu) * np.abs(wu)[:, None]).sum(0) if Xu.size else np.zeros(X.shape[1])
    return y, used, b


def eigen_zeroed(K):
    """EigenDecomp_Zeroed, src/lapack.cpp:260-291: eigenvalues below 1e-10 zeroed; returns (U, eval, trace_G = mean eval)"""
    ev, U = np.linalg.eigh(K)
    ev = np.where(ev < 1e-10, 0.0, ev)
    return U, ev, ev.mean()


def reml_logl(lam, ev, UtW, Uty):
    """the REML log-likelihood of the null model up to a constant (LogRL_f, src/lmm.cpp:1011-1070)"""
    n, c = UtW.shape
    h = 1.0 / (lam * ev + 1.0)
    WHW = UtW.T @ (UtW * h[:, None])
    WHy = UtW.T @ (Uty * h)
    Pyy = Uty @ (Uty * h) - WHy @ np.linalg.solve(WHW, WHy)
    return -0.5 * np.log(lam * ev + 1.0).sum() - 0.5 * np.linalg.slogdet(WHW)[1] - 0.5 * (n - c) * np.log(Pyy)


def reml_lambda(ev, UtW, Uty, l_min=1e-5, l_max=1e5):
    """argmax of reml_logl on [l_min, l_max]: a dense grid on log lambda, then golden section between the neighbours of the best
    point (the bounded search the reference's CalcLambda does with Brent + Newton, src/lmm.cpp:1920-2060)"""
    UtW = UtW.reshape(len(ev), -1)
    x = np.linspace(np.log(l_min), np.log(l_max), 4001)
    f = np.array([reml_logl(np.exp(v), ev, UtW, Uty) for v in x])
    k = int(np.argmax(f))
    if k == 0 or k == len(x) - 1:
        return float(np.exp(x[k]))
    a, b = x[k - 1], x[k + 1]
    g = (np.sqrt(5.0) - 1) / 2
    c, d = b - g * (b - a), a + g * (b - a)
    fc, fd = reml_logl(np.exp(c), ev, UtW, Uty), reml_logl(np.exp(d), ev, UtW, Uty)
    for _ in range(200):
        if fc > fd:
            b, d, fd = d, c, fc
            c = b - g * (b - a)
            fc = reml_logl(np.exp(c), ev, UtW, Uty)
        else:
            a, c, fc = c, d, fd
            d = a + g * (b - a)
            fd = reml_logl(np.exp(d), ev, UtW, Uty)
    return float(np.exp((a + b) / 2))


def ridge(Xc, y, lam=None):
    """-bslmm 2 from the centred rows of the analysed SNPs (p x n) and the phenotypes of the analysed individuals:
    K = Xc' Xc / p (ReadFile_bed with calc_K), EigenDecomp_Zeroed, y centred, the REML lambda, BSLMM::RidgeR.
    Returns dict(alpha, bv, lam, pheno_mean, U, ev, Uty, trace_G)."""
    p, n = Xc.shape
    U, ev, trace_G = eigen_zeroed(Xc.T @ Xc / p)
    mean = y.mean()
    Uty = U.T @ (y - mean)
    if lam is None:
        lam = reml_lambda(ev, U.T @ np.ones((n, 1)), Uty)
    b = Uty / (lam * ev + 1.0)
    return dict(alpha=lam / p * (Xc @ (U @ b)), bv=U @ (lam * ev * b), lam=lam, pheno_mean=mean, U=U, ev=ev, Uty=Uty, trace_G=trace_G)


def center_matrix_weighted(G, w):
    """CenterMatrix(G, w), src/mathfunc.cpp:181-201 (upper triangle updated, then mirrored)"""
    wtw = w @ w
    Gw = G @ w
    A = np.triu(G) - (np.outer(Gw, w) + np.outer(w, Gw)) / wtw + (w @ Gw) / wtw ** 2 * np.outer(w, w)
    A = np.triu(A)
    return A + np.triu(A, 1).T


def add_bv(G, ind, u_hat):
    """PRDT::AddBV, src/prdt.cpp:133-205: what it adds to y_prdt"""
    ind = np.asarray(ind)
    Gc = center_matrix_weighted(np.array(G, dtype=np.float64), ind.astype(np.float64))
    o, f = ind == 1, ind == 0
    ev, U = np.linalg.eigh(Gc[np.ix_(o, o)])
    ev = np.where(ev < 1e-10, 0.0, ev)
    Utu = U.T @ u_hat
    nz = ev != 0
    Utu[nz] = Utu[nz] / ev[nz]
    return Gc[np.ix_(f, o)] @ (U @ Utu)


def predict(G, rs, ind, est, pheno_mean, G_kin=None, u_hat=None, probit=False):
    """the -predict block of src/gemma.cpp:1660-1729: (y_prdt, ignored SNPs)"""
    ind = np.asarray(ind)
    y = np.zeros(int((ind == 0).sum()))
    if G_kin is not None:
        y += add_bv(G_kin, ind, u_hat)
    sel = [i for i, r in enumerate(rs) if r in est]
    w = np.array([est[rs[i]] for i in sel])
    yy, used, _ = xw(G[sel], w, ind)
    y = y + yy + pheno_mean
    if probit:
        from math import erfc, sqrt
        y = np.array([0.5 * erfc(-v / sqrt(2.0)) for v in y])
    return y, [rs[sel[i]] for i in np.flatnonzero(~used)]


def center_matrix(G):
    """CenterMatrix(G), src/mathfunc.cpp:147-177"""
    n = G.shape[0]
    w = np.ones(n)
    Gw = G @ w
    return G - np.outer(Gw, w) / n - np.outer(w, Gw) / n + (w @ Gw) / n ** 2 * np.outer(w, w)


def mvnorm_prdt(G_full, ind, W_full, y_full, lam=None):
    """a_mode 43 for one phenotype, src/gemma.cpp:1732-1820 with PRDT::MvnormPrdt (src/prdt.cpp:448-553):
    dict(Y_full, vg, ve, lam, ev, UtW, Uty) -- lam: the REML lambda to use (None: the dense search)"""
    ind = np.asarray(ind)
    o, f = ind == 1, ind == 0
    W_full = np.asarray(W_full, dtype=np.float64).reshape(len(ind), -1)
    U, ev, _ = eigen_zeroed(center_matrix(G_full[np.ix_(o, o)]))
    W, y = W_full[o], np.asarray(y_full, dtype=np.float64)[o]
    UtW, Uty = U.T @ W, U.T @ y
    if lam is None:
        lam = reml_lambda(ev, UtW, Uty)
    h = 1.0 / (lam * ev + 1.0)
    WHW = UtW.T @ (UtW * h[:, None])
    beta = np.linalg.solve(WHW, UtW.T @ (Uty * h))
    n, c = UtW.shape
    ve = (Uty @ (Uty * h) - (UtW.T @ (Uty * h)) @ beta) / (n - c)  # CalcLmmVgVeBeta, src/lmm.cpp:2208-2280
    vg = ve * lam
    H = ve * np.eye(len(ind)) + vg * center_matrix(np.asarray(G_full, dtype=np.float64))
    Y = np.asarray(y_full, dtype=np.float64).copy()
    Y[f] = W_full[f] @ beta + H[np.ix_(f, o)] @ np.linalg.solve(H[np.ix_(o, o)], y - W @ beta)
    return dict(Y_full=Y, vg=vg, ve=ve, lam=lam, ev=ev, UtW=UtW, Uty=Uty)


def m43_inputs(name, cvt):
    """(tag of the fixture, W_full) of a kinship-only prediction: the intercept alone, or the columns of <name>.cvt.txt"""
    d = load_set(name)
    if not cvt:
        return name + "_m43", np.ones((d["ni_total"], 1))
    W = np.array([[float(v) for v in l.split()] for l in open(os.path.join(FX, name + ".cvt.txt")) if l.strip()])
    assert W.shape == (d["ni_total"], 2)
    return name + "_m43c", W


M43_CASES = (("B", False), ("Sb", False), ("Sb", True))


def parse_full(text):
    """the .prdt.txt of a_mode 43: one value (and a tab) per row"""
    return np.array([float(l.split()[0]) for l in text.splitlines() if l.strip()])


# ------------------------------------------------------------------------------------------------ the fixture sets
_SETS = {}


def load_set(name):
    """dict(kind 'plink' | 'bimbam', G (p x ni_total doubles, NaN = missing), rows (.bed rows, PLINK only), rs, chr, ps, ind
    (indicator_idv: 1 = phenotyped), y_all, snp (indicator_snp of the reference's first pass on the analysed individuals), n_miss)"""
    if name in _SETS:
        return _SETS[name]
    from oracle import oracle as O
    if name in ("P", "S"):
        prefix = os.path.join(TXT if name == "P" else FX, name)
        rows, ni, ph, ind = O.read_bed(prefix)
        bim = [l.split() for l in open(prefix + ".bim") if l.strip()]
        d = dict(kind="plink", rows=np.ascontiguousarray(rows), G=bed_unpack(rows, ni), rs=[b[1] for b in bim], chr=[b[0] for b in bim],
                 ps=[b[3] for b in bim], ind=ind, y_all=ph)
        Ga = d["G"][:, ind == 1]
        d["snp"] = O.qc_snps_bed(Ga, np.ones((int(ind.sum()), 1)))
        d["n_miss"] = np.isnan(Ga).sum(1)
    else:
        if name == "B":
            geno, phen, anno = (os.path.join(TXT, f) for f in ("bxd_mean_genotypes.txt.gz", "bxd_trait.txt.gz", "bxd_anno.txt.gz"))
        else:
            geno, phen, anno = (os.path.join(FX, f) for f in ("Sb.geno.txt.gz", "Sb.pheno.txt", "Sb.anno.txt"))
        rs, G = O.read_bimbam_geno(geno)
        op = gzip.open if phen.endswith(".gz") else open
        with op(phen, "rt") as f:
            tok = [l.split()[0] for l in f if l.strip()]
        ind = np.array([0 if t == "NA" else 1 for t in tok], dtype=np.int32)
        y_all = np.array([-9.0 if t == "NA" else float(t) for t in tok])
        op = gzip.open if anno.endswith(".gz") else open
        with op(anno, "rt") as f:
            an = {t[0]: t for t in (l.replace(",", " ").split() for l in f if l.strip())}
        d = dict(kind="bimbam", G=G, rs=rs, chr=[an[r][2] if r in an else "-9" for r in rs], ps=[an[r][1] if r in an else "-9" for r in rs],
                 ind=ind, y_all=y_all)
        d["snp"], _, d["n_miss"] = O.qc_snps(G, ind, np.ones((int(ind.sum()), 1)))
    d["ni_total"] = d["G"].shape[1]
    _SETS[name] = d
    return d


def snp_info(d):
    return [dict(chr=d["chr"][i], rs=d["rs"][i], ps=d["ps"][i], n_miss=int(d["n_miss"][i])) for i in np.flatnonzero(d["snp"] == 1)]


def fx_text(tag, ext):
    with gzip.open(os.path.join(FX, tag + ext + ".gz"), "rt") as f:
        return f.read()


def fx_log(tag):
    return json.load(open(os.path.join(FX, tag + ".log.json")))


def parse_param(text):
    rows = [l.split("\t") for l in text.splitlines()[1:] if l.strip()]
    return [r[1] for r in rows], np.array([float(r[4]) for r in rows])


def parse_column(text):
    """a one-column file with NA rows -> (values of the other rows, mask of the NA rows)"""
    tok = [l.strip() for l in text.splitlines() if l.strip()]
    na = np.array([t == "NA" for t in tok])
    return np.array([float(t) for t in tok if t != "NA"]), na


def assert_printed(got, ref, what):
    """rtol 5e-6 on every printed number whose reference value is non-zero at print precision; prints the largest difference"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    nz = ref != 0
    rel = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz]) if nz.any() else np.zeros(1)
    print("%s: %d numbers, %d non-zero in print, max relative difference %.3g" % (what, ref.size, int(nz.sum()), rel.max()))
    assert np.all(np.isfinite(got[nz])), what
    assert rel.max() <= RTOL_PRINTED, (what, float(rel.max()), int(np.argmax(rel)))


def kinship_all(d):
    """the -gk 1 kinship the fixture's -k file held: SNP filters on the analysed individuals, all individuals in the matrix,
    written with ten significant digits (PARAM::WriteMatrix) and read back"""
    from oracle import oracle as O
    return O.round10(O.calc_kin(d["G"][d["snp"] == 1], 1))


def mirror_driver(tmpdir):
    """tests/cpp/prdt_mirror_driver.cpp (class BSLMM / class PRDT of include/gemma_host.hpp) built against the library"""
    import subprocess
    from gemma_amd import build
    so = build.build()
    exe = os.path.join(str(tmpdir), "prdt_mirror_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "prdt_mirror_driver.cpp"), "-L" + os.path.dirname(so), "-lgemma_hip",
                           "-pthread", "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    return exe

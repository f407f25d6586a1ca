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


# -vc 2 on the fixtures: (tag of tests/golden/text/<tag>.log.json, tag of the inputs in HE_CASES, noconstrain)
REML_CASES = [("V1r", "V1", False), ("V1cr", "V1c", False), ("V2cr", "V2c", False), ("V3r", "V3", False),
              ("VB1r", "VB1", False), ("VB2r", "VB2", False), ("V1nr", "V1", True)]
# the reference's own -vc 2 dies on these: its first trial point (the full Gauss-Newton step on log sigma2) sends every sigma2
# to 0 or to infinity, H is singular and LUInvert raises "matrix is singular" (src/lapack.cpp:323-329)
REML_DIES = ("V2cr", "V3r")
ITER_CAP = 102
SPD_C = 0.01  # the SPD inverse's forward-error bound (tests/test_gpu_vc.py): ||X - A^-1||_max <= SPD_C n eps kappa ||A^-1||_max
_INPUTS = {}


def inputs(tag):
    """(Ks, W, y) of an HE_CASES tag, built once per process (callers must not modify them)"""
    if tag not in _INPUTS:
        _INPUTS[tag] = dict(HE_CASES)[tag]()
    return _INPUTS[tag]


def he_start(Ks, W, y, noconstrain=False):
    """the REML start of src/vc.cpp:1746-1758: the HE sigma2, log(0.1) for components <= 0 on the log scale"""
    h = he(Ks, W, y)["sigma2"]
    return h.copy() if noconstrain else np.log(np.where(h > 0, h, 0.1))


def ref_args(Ks, W, y):
    """the kinships one after the other, W and y as the ref_vc_* entry points of oracle/ref_bridge.cpp take them"""
    return (np.ascontiguousarray(np.stack(Ks)), np.ascontiguousarray(W, dtype=np.float64),
            np.ascontiguousarray(y, dtype=np.float64))


def ref_reml(call, Ks, W, y, noconstrain=False):
    """call('ref_vc_reml', ...) (a refcalls.ref of tests/test_reference_pin.py, live or replayed): the reference's
    VC::CalcVCreml at full precision.  status = -1 where the reference's run dies on a GSL error (iterations = those
    printed before it)."""
    n, nvc = len(y), len(Ks)
    K, W, y = ref_args(Ks, W, y)
    r = dict(sigma2=np.zeros(nvc + 1), se_sigma2=np.zeros(nvc + 1), pve=np.zeros(nvc), se_pve=np.zeros(nvc),
             totals=np.zeros(2), iter_sigma2=np.zeros((ITER_CAP, nvc + 1)), status=np.zeros(1))
    it = call("ref_vc_reml", int(noconstrain), n, nvc, K, W, W.shape[1], y, r["sigma2"], r["se_sigma2"], r["pve"], r["se_pve"],
              r["totals"], r["iter_sigma2"], ITER_CAP, r["status"])
    r["iterations"] = int(it)
    r["status"] = int(r["status"][0])
    r["pve_total"], r["se_pve_total"] = r["totals"]
    r["iter_sigma2"] = r["iter_sigma2"][:int(it) + 1]
    return r


def hybrid_drive_lib(tmpdir):
    """tests/cpp/hybrid_drive.cpp (GEMMA's -vc 2 loop around include/gemma_vc_hybrid.hpp) as a shared library"""
    import ctypes as C
    import subprocess
    so = os.path.join(str(tmpdir), "libhybrid_drive.so")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-shared", "-fPIC", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "hybrid_drive.cpp"), "-o", so])
    lib = C.CDLL(so)
    P = C.POINTER(C.c_double)
    lib.FDF = C.CFUNCTYPE(C.c_int, P, P, P)
    lib.hybrid_drive.restype = C.c_int
    lib.hybrid_drive.argtypes = [C.c_int, P, lib.FDF, C.c_int, C.c_double, P, C.c_int, C.POINTER(C.c_int)]
    return lib


def numpy_reml(lib, Ks, W, y, noconstrain=False, outside=False):
    """the numpy LogRL_dev12 (reml_dev / reml_log_dev) solved by the host hybridsj in GEMMA's loop, and the summary at the
    solution: the same fields as ref_reml.  An evaluation where H or W^T H^-1 W is singular fails, as the reference's does;
    with outside, a point where H is not positive definite (Cholesky fails) is a failed step instead, as on the device."""
    import ctypes as C
    m = len(Ks) + 1
    dev = (lambda z: reml_dev(z, Ks, W, y)) if noconstrain else (lambda z: reml_log_dev(z, Ks, W, y))

    def cb(xp, fp, jp):
        x = np.ctypeslib.as_array(xp, (m,)).copy()
        if outside:
            s2 = x if noconstrain else np.exp(x)
            with np.errstate(all="ignore"):
                H = sum(s * K for s, K in zip(s2, Ks)) + s2[-1] * np.eye(len(y))
            try:
                if not np.all(np.isfinite(H)):
                    return 2
                np.linalg.cholesky(H)
            except np.linalg.LinAlgError:
                return 2
        try:
            with np.errstate(all="ignore"):
                d1, d2 = dev(x)
        except np.linalg.LinAlgError:
            return 1
        np.ctypeslib.as_array(fp, (m,))[:] = d1
        np.ctypeslib.as_array(jp, (m * m,))[:] = d2.ravel()
        return 0

    fdf = lib.FDF(cb)
    x = np.ascontiguousarray(he_start(Ks, W, y, noconstrain))
    iters = np.zeros((ITER_CAP, m))
    st = C.c_int(0)
    P = C.POINTER(C.c_double)
    it = lib.hybrid_drive(m, x.ctypes.data_as(P), fdf, 100, 1e-3, iters.ctypes.data_as(P), ITER_CAP, C.byref(st))
    if st.value < 0:  # the failed iteration printed nothing
        it -= 1
    s2 = x if noconstrain else np.exp(x)
    r = dict(iterations=it, status=st.value, sigma2=s2,
             iter_sigma2=iters[:it + 1] if noconstrain else np.exp(iters[:it + 1]))
    if st.value >= 0:
        r.update(reml_summary(s2, Ks, W, y, noconstrain=noconstrain))
    return r


def spd_spectrum(n, kappa, seed, steps=1):
    """A = Q diag(ev) Q^T (symmetrised), ev geometric from 1 to kappa, and its inverse: np.linalg.inv refined by `steps`
    Newton steps X + X (I - A X), the residual I - A X formed in np.longdouble (the correction itself is ~ kappa eps smaller
    than X, so float64 carries it).  tests/test_vc_cpu.py holds both parts of the refined error -- what the Newton step leaves
    and the rounding floor of the long-double residual -- below 1 / 100 of the bound the GPU tests assert."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.geomspace(1.0, kappa, n)) @ Q.T
    A = (A + A.T) / 2
    X = np.linalg.inv(A)
    Al = A.astype(np.longdouble)
    for _ in range(steps):
        R = -(Al @ X.astype(np.longdouble))
        R[np.diag_indices(n)] += 1
        X = X + X @ R.astype(np.float64)
    return A, X

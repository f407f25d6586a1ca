"""Numpy restatements of GEMMA's kinship-only prediction for several phenotypes (a_mode 43 with n_ph > 1: the else branch of
src/gemma.cpp:1821-1871 with PRDT::MvnormPrdt, src/prdt.cpp:448-553) and the loaders of its fixtures (tests/golden/prdt_mv,
tests/golden/make_prdt_mv_fixtures.py) -- shared by tests/test_prdt_mv_cpu.py and tests/test_gpu_prdt_mv.py.

Entries are ordered i * d + a (individual-major), as KroneckerSym and MvnormPrdt order them."""
import gzip
import json
import os

import numpy as np

import prdtcases as P

FX = os.path.join(P.ROOT, "tests", "golden", "prdt_mv")
EPS = P.EPS
# tag -> (the -n columns, 0-based; with Sb.cvt.txt)
RUNS = {"Sb_mv2": ((0, 1), False), "Sb_mv3": ((0, 1, 2), False), "Sb_mv2c": ((0, 1), True)}


def mvnorm_prdt_multi_dense(G_full, ind, W_full, Y_full, Vg, Ve, B):
    """The way the reference does it: H_full = Gc (x) Vg + I (x) Ve in full, H_oo and H_mo by index, a dense solve.
    Returns Y_full with the unobserved entries filled."""
    ind = np.asarray(ind).reshape(len(ind), -1)
    ni, d = ind.shape
    Gc = P.center_matrix(np.asarray(G_full, dtype=np.float64))
    H = np.kron(Gc, Vg) + np.kron(np.eye(ni), Ve)
    o, m = np.flatnonzero(ind.ravel() != 0), np.flatnonzero(ind.ravel() == 0)
    Y_hat = (np.asarray(W_full, dtype=np.float64).reshape(ni, -1) @ np.asarray(B).T).ravel()
    y = np.where(ind != 0, np.asarray(Y_full, dtype=np.float64), 0.0).ravel()
    out = y.copy()
    out[m] = Y_hat[m] + H[np.ix_(m, o)] @ np.linalg.solve(H[np.ix_(o, o)], y[o] - Y_hat[o])
    return out.reshape(ni, d)


def h_oo(Gc, ind, Vg, Ve):
    """H_oo[(i,a),(j,b)] = Gc_ij Vg_ab + delta_ij Ve_ab from the index lists, and the lists (oi, oa)"""
    ind = np.asarray(ind).reshape(len(ind), -1)
    oi, oa = np.nonzero(ind != 0)  # row-major order = i * d + a order
    H = Gc[np.ix_(oi, oi)] * Vg[np.ix_(oa, oa)] + (oi[:, None] == oi[None, :]) * Ve[np.ix_(oa, oa)]
    return H, oi, oa


def mvnorm_prdt_multi(G_full, ind, W_full, Y_full, Vg, Ve, B):
    """The structured way: H_oo assembled directly, z = H_oo^-1 r, Z = z scattered, P = Gc Z Vg + Z Ve; H_full and H_mo are
    never formed."""
    ind = np.asarray(ind).reshape(len(ind), -1)
    ni, d = ind.shape
    Vg, Ve = np.asarray(Vg, dtype=np.float64), np.asarray(Ve, dtype=np.float64)
    Gc = P.center_matrix(np.asarray(G_full, dtype=np.float64))
    H, oi, oa = h_oo(Gc, ind, Vg, Ve)
    Y_hat = np.asarray(W_full, dtype=np.float64).reshape(ni, -1) @ np.asarray(B).T
    Y = np.where(ind != 0, np.asarray(Y_full, dtype=np.float64), 0.0)
    Z = np.zeros((ni, d))
    Z[oi, oa] = np.linalg.solve(H, (Y - Y_hat)[oi, oa])
    Pm = Gc @ Z @ Vg + Z @ Ve
    return np.where(ind != 0, Y, Y_hat + Pm)


# ------------------------------------------------------------------------------------------------ fixtures
_IN = {}


def inputs(tag):
    """dict(G_full: the -gk 1 kinship of Sb as the -k file held it, ind (300 x d), Y (300 x d, 0 where NA), W (300 x c))"""
    if tag in _IN:
        return _IN[tag]
    cols, cvt = RUNS[tag]
    if "K" not in _IN:
        _IN["K"] = P.kinship_all(P.load_set("Sb"))
        tok = [l.split() for l in open(os.path.join(FX, "Sb.pheno3.txt")) if l.strip()]
        _IN["ind3"] = np.array([[0 if t == "NA" else 1 for t in r] for r in tok], dtype=np.int32)
        _IN["Y3"] = np.array([[0.0 if t == "NA" else float(t) for t in r] for r in tok])
    ni = _IN["K"].shape[0]
    W = P.m43_inputs("Sb", True)[1] if cvt else np.ones((ni, 1))
    _IN[tag] = dict(G_full=_IN["K"], ind=np.ascontiguousarray(_IN["ind3"][:, cols]), Y=np.ascontiguousarray(_IN["Y3"][:, cols]),
                    W=np.ascontiguousarray(W))
    return _IN[tag]


def fx_log(tag):
    return json.load(open(os.path.join(FX, tag + ".log.json")))


def fx_prdt(tag):
    """the reference's .prdt.txt: ni x d"""
    with gzip.open(os.path.join(FX, tag + ".prdt.txt.gz"), "rt") as f:
        return np.array([[float(v) for v in l.split()] for l in f if l.strip()])


def lower(M):
    """the printed lower triangle, row by row"""
    M = np.asarray(M)
    return np.array([M[i, j] for i in range(M.shape[0]) for j in range(i + 1)])


def log_lower(rows):
    return np.array([v for r in rows for v in r])


def complete(ind):
    return np.flatnonzero(np.asarray(ind).reshape(len(ind), -1).all(1))


def oracle_fit(O, tag):
    """The null fit of src/gemma.cpp:1772-1830 with the C restatement's mvlmm_null: the complete individuals' centred kinship,
    eigenvalues below 1e-10 zeroed (prdtcases.eigen_zeroed).  dict(Vg, Ve, B)"""
    key = ("fit", tag)
    if key not in _IN:
        c = inputs(tag)
        pos = complete(c["ind"])
        U, ev, _ = P.eigen_zeroed(P.center_matrix(c["G_full"][np.ix_(pos, pos)]))
        UtW = np.ascontiguousarray((U.T @ c["W"][pos]).T)
        UtY = np.ascontiguousarray((U.T @ c["Y"][pos]).T)
        null = O.mvlmm_null(O.mv_cfg(), np.ascontiguousarray(ev), UtW, UtY)
        _IN[key] = dict(Vg=null["Vg_remle"], Ve=null["Ve_remle"], B=null["B_remle"])
    return _IN[key]


def synthetic(ni, d, c, seed, miss=0.2):
    """A kinship, an indicator with scattered missing entries (one individual without any trait, one with two missing traits),
    covariates, phenotypes and SPD Vg / Ve for the tests that need no reference file"""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((ni, 2 * ni))
    G = X @ X.T / (2 * ni)
    ind = (rng.random((ni, d)) >= miss).astype(np.int32)
    ind[ni // 3] = 0
    ind[ni // 2] = 1
    ind[ni // 2, :2] = 0
    W = np.column_stack([np.ones(ni)] + [rng.standard_normal(ni) for _ in range(c - 1)])
    Y = rng.standard_normal((ni, d)) * 2 + 1
    A, E = rng.standard_normal((d, d)), rng.standard_normal((d, d))
    Vg, Ve = A @ A.T / d + 0.3 * np.eye(d), E @ E.T / d + 0.5 * np.eye(d)
    B = rng.standard_normal((d, c))
    return dict(G_full=G, ind=ind, W=np.ascontiguousarray(W), Y=Y, Vg=Vg, Ve=Ve, B=B)

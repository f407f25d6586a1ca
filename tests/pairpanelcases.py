"""Cases and reference of the trait-pair panel tests (tests/test_pair_panel_cpu.py on one CPU lane, tests/test_gpu_pair_panel.py on
the GPU): the two-trait null fits of every pair of a panel with their variances and correlations, and the variances of the general
null block (gemma_hip_mvlmm_null_se).

Cases: make_case(257, 5, cw, 2, seed) for (cw, seed) in CASES.  n = 257 is four full trips of the 64-lane loop and a one-lane tail,
T = 5 gives 10 pairs: with GEMMA_HIP_MVPAIR_WAVES=4 two full four-wave workgroups and a ragged one.  (n = 131 is not usable:
several pairs end on the boundary of the positive-definite cone there, one with a negative variance diagonal.)  No seed had to be
replaced.

The reference is COMPOSED from the oracle's exported primitives (the oracle has no GLS export): mph_initial, then for 'R' and 'L'
mph_em, mph_nr -- whose returned matrix is already the variance matrix -H^-1 of MphNR's last CalcDev call -- and a dense numpy GLS
step B = (sum_k x_k x_k^T (x) H_k^-1)^-1 sum_k x_k (x) H_k^-1 y_k, H_k = delta_k V_g + V_e, the diagonal of that inverse being VB.
r and var_r follow from the returned matrix in numpy.  tests/test_pair_panel_cpu.py checks the composition against O.mvlmm_null.

Under FIXC (both tolerances 0: exactly 8 EM sweeps and 2 rounds of MphNR, i.e. one Newton step, per pass) every pair of the three
cases is interior: smallest eigenvalue of a fitted V >= 0.036, smallest diagonal of a variance matrix >= 0.0077, smallest of all
reported variances (VB and var_r included) 0.0019.

Worst one-lane-against-composition disagreement per field under FIXC over the 30 pairs, relative to the field's largest reference
entry of the pair -- for the scalars rg / re to the correlation itself (measured by test_one_lane_matches_the_composition, printed
with -s):
    Vg 1.4e-14  Ve 7.6e-15  logl 9.9e-16  B 9.5e-15  VVg 1.5e-14 (cw 6)  VVe 2.1e-14 (cw 3)  VB 7.6e-15 (cw 1)
    rg 2.4e-12 (cw 6: a correlation near zero)  var_rg 6.4e-14 (cw 1)  re 4.2e-13 (cw 3)  var_re 1.0e-14 (cw 1)
The general-d epilogue on (3, 2) and (2, 8): VV 7.6e-15, VB 2.8e-15.  All below CAP = 3e-11, so CAP is the cap of every field, new
ones included, and BAR = 32 x CAP holds the GPU."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from mvfixcases import BAR, CAP, NULL_N, null_case  # noqa: F401  (the project's caps; the null cases of the general-d checks)
from oracle import oracle as O
from test_oracle_mvlmm import MvNullArgs, make_case

HERE = os.path.dirname(os.path.abspath(__file__))
N, T = 257, 5
CASES = [(1, 4001), (3, 4003), (6, 4006)]            # (covariates, seed)
PAIRS = [(i, j) for i in range(T) for j in range(i + 1, T)]
FIXC = dict(em_iter=8, em_prec=0.0, nr_iter=2, nr_prec=0.0)
SE_SHAPES = [(3, 2), (2, 8)]                         # (d, covariates) of the general-d epilogue: a fixed and a run-time null fit
BLOCK_FIELDS = ("Vg", "Ve", "logl", "B", "VVg", "VVe", "VB", "rg", "var_rg", "re", "var_re")
IU = np.triu_indices(2)


class MvPairArgs(C.Structure):
    dp = C.POINTER(C.c_double)
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("m", C.c_long), ("eval", dp), ("Wt", dp), ("Yp", dp), ("pairs", C.POINTER(C.c_int)),
                ("start", dp), ("em_iter", C.c_int), ("nr_iter", C.c_int), ("em_prec", C.c_double), ("nr_prec", C.c_double), ("raw", dp)]


class PairBlock(C.Structure):
    _fields_ = [("Vg", C.c_double * 3), ("Ve", C.c_double * 3), ("VVg", C.c_double * 3), ("VVe", C.c_double * 3)] + \
               [(k, C.c_double) for k in ("rg", "var_rg", "re", "var_re", "logl")]


class PairFit(C.Structure):
    """ctypes mirror of gemma_mvpair_fit (include/gemma_hip.h)"""
    _fields_ = [("i", C.c_int), ("j", C.c_int), ("status", C.c_int), ("pad", C.c_int), ("remle", PairBlock), ("mle", PairBlock)]


@functools.lru_cache(maxsize=None)
def case(cw):
    c = make_case(N, T, cw, 2, dict(CASES)[cw])
    c["cw"] = cw
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def cfg_of(fixed):
    return O.mv_cfg(**FIXC) if fixed else O.mv_cfg()


def gls(ev, W, Y, Vg, Ve):
    """Dense GLS at (Vg, Ve): B (d x c) and VB (d x c), the diagonal of (sum_k w_k w_k^T (x) H_k^-1)^-1"""
    d, n = Y.shape
    c = W.shape[0]
    A, b = np.zeros((c * d, c * d)), np.zeros(c * d)
    for k in range(n):
        Hi = np.linalg.inv(ev[k] * Vg + Ve)
        w = W[:, k]
        A += np.kron(np.outer(w, w), Hi)
        b += np.kron(w, Hi @ Y[:, k])
    Ai = np.linalg.inv(A)
    return np.ascontiguousarray((Ai @ b).reshape(c, d).T), np.ascontiguousarray(np.diag(Ai).reshape(c, d).T)


def corr(V, S):
    """r = V01 / sqrt(V00 V11) and its delta-method variance from the 3 x 3 block S (order 00, 01, 11)"""
    r = V[0, 1] / np.sqrt(V[0, 0] * V[1, 1])
    g = np.array([-r / (2 * V[0, 0]), 1 / np.sqrt(V[0, 0] * V[1, 1]), -r / (2 * V[1, 1])])
    return r, float(g @ S @ g)


def compose(ev, W, Y, cfg):
    """The null block of (W, Y) composed from the oracle's primitives: {"remle": block, "mle": block}; a block holds Vg, Ve (d x d),
    logl, B, VB (d x c), VV (the full variance matrix) and for d = 2 the correlations"""
    ev, W, Y = np.array(ev), np.ascontiguousarray(W), np.ascontiguousarray(Y)
    d = Y.shape[0]
    v = d * (d + 1) // 2
    Vg, Ve, B = O.mph_initial(cfg, ev, W, Y)
    out = {}
    for func, tag in (("R", "remle"), ("L", "mle")):
        O.mph_em(func, cfg.em_iter, cfg.em_prec, ev, W, Y, Vg, Ve, B)
        logl, VV = O.mph_nr(func, cfg.nr_iter, cfg.nr_prec, ev, W, Y, Vg, Ve)
        B, VB = gls(ev, W, Y, Vg, Ve)
        b = {"Vg": Vg.copy(), "Ve": Ve.copy(), "logl": logl, "B": B.copy(), "VB": VB, "VV": VV.copy(),
             "VVg": np.diag(VV)[:v].copy(), "VVe": np.diag(VV)[v:].copy()}
        if d == 2:
            b["rg"], b["var_rg"] = corr(Vg, VV[:3, :3])
            b["re"], b["var_re"] = corr(Ve, VV[3:, 3:])
        out[tag] = b
    return out


_REF = {}


def reference(cw, fixed=True):
    """compose() of every pair of case(cw), computed once: list over PAIRS"""
    key = (cw, fixed)
    if key not in _REF:
        c = case(cw)
        _REF[key] = [compose(c["ev"], c["UtW"], c["UtY"][[i, j]], cfg_of(fixed)) for i, j in PAIRS]
    return _REF[key]


@functools.lru_cache(maxsize=None)
def se_reference(d, cw):
    c = null_case(d, cw)
    return compose(c["ev"], c["UtW"], c["UtY"], cfg_of(True))


def starts(c, cfg):
    """T x 8 like gemma_null_fit: [6] vg_remle, [7] ve_remle of each trait's univariate REML fit (MphInitial's diagonals)"""
    s = np.zeros((T, 8))
    for t in range(T):
        Vg, Ve, _ = O.mph_initial(cfg, np.array(c["ev"]), np.array(c["UtW"]), np.ascontiguousarray(c["UtY"][[t]]))
        s[t, 6], s[t, 7] = Vg[0, 0], Ve[0, 0]
    return s


def block_of(f, B, VB):
    """a PairBlock (ctypes or numpy record) with its B / VB (2 x c) as the dict compose() returns, the matrices as packed triangles"""
    o = {k: np.array(f[k] if isinstance(f, np.void) else getattr(f, k), dtype=float) for k in ("Vg", "Ve", "VVg", "VVe")}
    for k in ("rg", "var_rg", "re", "var_re", "logl"):
        o[k] = float(f[k] if isinstance(f, np.void) else getattr(f, k))
    o["B"], o["VB"] = np.array(B), np.array(VB)
    return o


def deviations(got, ref):
    """per field the deviation of a block from compose()'s, relative to the field's largest reference entry"""
    out = {}
    for k in BLOCK_FIELDS:
        r = ref[k][IU] if k in ("Vg", "Ve") else np.asarray(ref[k], dtype=float)
        g = np.asarray(got[k], dtype=float).reshape(np.shape(r))
        out[k] = float(np.abs(g - r).max() / np.abs(r).max()) if np.all(np.isfinite(g)) else float("nan")
    return out


def build_harness():
    src = os.path.join(HERE, "host", "mvpair_harness.cpp")
    so = os.path.join(HERE, "host", "libmvpair_harness.so")
    hdrs = [os.path.join(HERE, "..", "gemma_amd", "csrc", h) for h in ("mvlmm.hip.h", "mvlmm_pair.hip.h")]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", so, src])
    H = C.CDLL(so)
    for f in ("mvp_pair_args_size", "mvp_pair_fit_size", "mvp_null_args_size"):
        getattr(H, f).restype = C.c_size_t
    assert H.mvp_pair_args_size() == C.sizeof(MvPairArgs) and H.mvp_pair_fit_size() == C.sizeof(PairFit)
    assert H.mvp_null_args_size() == C.sizeof(MvNullArgs)
    return H


def harness_pairs(H, cw, fixed=True):
    """mv_pair_fit + mv_pair_finish on one CPU lane over PAIRS of case(cw): list of {"remle": block, "mle": block, "status": s}"""
    c, cfg = case(cw), cfg_of(fixed)
    m = len(PAIRS)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ev, W = np.array(c["ev"]), np.array(c["UtW"])
    Yp = np.ascontiguousarray(np.stack([c["UtY"][[i, j]] for i, j in PAIRS]))
    pairs = np.array(PAIRS, dtype=np.int32).ravel()
    st = starts(c, cfg)
    raw = np.zeros((m, H.mvp_raw_doubles(cw)))
    fit = (PairFit * m)()
    B, VB = np.zeros((m, 2, 2, cw)), np.zeros((m, 2, 2, cw))
    a = MvPairArgs()
    a.n, a.c, a.m = N, cw, m
    a.eval, a.Wt, a.Yp, a.start, a.raw = P(ev), P(W), P(Yp), P(st), P(raw)
    a.pairs = pairs.ctypes.data_as(C.POINTER(C.c_int))
    a.em_iter, a.nr_iter, a.em_prec, a.nr_prec = cfg.em_iter, cfg.nr_iter, cfg.em_prec, cfg.nr_prec
    assert H.mvp_pairs(C.byref(a), fit, P(B), P(VB)) == 0
    out = []
    for q, (i, j) in enumerate(PAIRS):
        assert (fit[q].i, fit[q].j) == (i, j)
        out.append({"remle": block_of(fit[q].remle, B[q, 0], VB[q, 0]), "mle": block_of(fit[q].mle, B[q, 1], VB[q, 1]),
                    "status": fit[q].status})
    return out


def harness_null_se(H, d, cw, with_se=True):
    """mv_null_fit<0, 0> with the epilogue on one CPU lane on null_case(d, cw) under FIXC -> (out, se): the raw blocks"""
    c, cfg = null_case(d, cw), cfg_of(True)
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    keep = [np.array(c[k]) for k in ("ev", "UtW", "UtY")]
    Vg0, Ve0, _ = O.mph_initial(cfg, *keep)
    a = MvNullArgs()
    a.g.n, a.g.eval, a.g.Wt, a.g.Yt = NULL_N, P(keep[0]), P(keep[1]), P(keep[2])
    a.g.nr_iter, a.g.nr_prec, a.g.d, a.g.c = cfg.nr_iter, cfg.nr_prec, d, cw
    a.em_iter, a.em_prec = cfg.em_iter, cfg.em_prec
    for i, x in enumerate(Vg0.ravel()):
        a.Vg0[i] = x
    for i, x in enumerate(Ve0.ravel()):
        a.Ve0[i] = x
    out = np.zeros(2 * (2 * d * d + d * cw + 1))
    se = np.zeros(2 * H.mvp_null_se_doubles(d, cw))
    a.out = P(out)
    assert (H.mvp_null_se_rt(C.byref(a), P(se)) if with_se else H.mvp_null_rt(C.byref(a))) == 0
    return out, se

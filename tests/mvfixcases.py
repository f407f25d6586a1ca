"""Cases and reference of the fixed-iteration-count tests of the multivariate LMM (tests/test_mvlmm_fixed_count_cpu.py on one
CPU lane, tests/test_gpu_mvlmm_instances.py on the GPU).

The per-SNP EM and Newton-Raphson loops stop on |delta logl| < prec, so two correct implementations may take a different number
of iterations and then agree to ~1e-4 only.  With both tolerances at 0 neither loop can stop early: every SNP takes exactly
em_iter / 10 = 8 EM sweeps and nr_iter / 10 = 2 rounds of MphNR (one Newton step), and with p_nr above every p value every SNP
takes every branch of the per-SNP flow (score, EM ML, NR, LRT, EM REML, NR, Wald, and with crt = 1 the Edgeworth factors).  The
starting point is synthetic and interior: a fitted null of so few individuals lands on the boundary of the positive-definite
cone, where every downstream number is conditioned like 1 / (smallest eigenvalue)."""
import ctypes as C
import functools

import numpy as np

from oracle import oracle as O
from test_oracle_mvlmm import MvArgs, make_case

# what the library promises: (d, rows of X = covariates + the SNP) with a fixed per-SNP kernel ...
FIXED_SNP = [(1, 2), (1, 3), (1, 4), (2, 2), (2, 3), (2, 4), (3, 2), (3, 3), (3, 4), (4, 2), (4, 3), (4, 4), (5, 2), (5, 3), (5, 4),
             (1, 5), (1, 6), (1, 7), (2, 5), (2, 6), (2, 7), (3, 5), (3, 6), (3, 7),
             (6, 2), (6, 3), (6, 4), (7, 2), (7, 3), (7, 4),
             (8, 2)]
# ... and (d, covariates) with a fixed null-fit kernel
FIXED_NULL = [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3), (3, 1), (3, 2), (3, 3), (4, 1), (4, 2), (4, 3), (5, 1), (5, 2), (5, 3),
              (1, 4), (1, 5), (1, 6), (2, 4), (2, 5), (2, 6), (3, 4), (3, 5), (3, 6)]
RT_SNP = [(4, 4), (5, 6), (2, 10), (8, 2), (8, 3), (6, 4)]   # (d, covariates): per-SNP shapes only the run-time kernel takes
RT_NULL = [(6, 1), (8, 2), (4, 5), (2, 8)]                   # (d, covariates): null fits only the run-time kernel takes
RT_TWINS = [(1, 1), (3, 3), (5, 3), (3, 6), (6, 1), (7, 3), (8, 1)]  # (d, covariates): fixed shapes also sent through the run-time kernel
MODE_SHAPES = [(2, 1), (3, 5), (6, 2), (4, 4)]               # (d, covariates) for a_mode 1, 2, 3: one per kernel family
GXE_SHAPES = [(2, 1), (3, 2)]                                # (d, covariates without the environment)

FIX = dict(em_iter=80, em_prec=0.0, nr_iter=20, nr_prec=0.0, p_nr=2.0)
FIELDS = ("beta", "Vbeta", "Vg", "Ve", "p_wald", "p_lrt", "p_score")
CAP = 3e-11   # oracle against the kernel source on one lane: the condition every committed case meets (CPU test)
BAR = 1e-9    # GPU against the oracle: 32 x CAP

# seeds: (d, covariates) -> seed; every other per-SNP case takes 100 * d + covariates.  A seed is replaced when the two CPU
# formulations disagree by more than CAP on its case (the case is then badly conditioned, not the code wrong).
SEEDS = {(2, 6): 10206, (3, 6): 10306, (6, 3): 30603}   # 206: 2.2e-9, 306: 2.3e-10, 603 / 10603 / 20603: 1e-8 .. 2.5e-10 (-crt factors near a pole)
GXE_SEEDS = {(2, 1): 21201, (3, 2): 1302}            # 1201: a V_g eigenvalue of 4.6e-5; 11201: 8.6e-11
NULL_N = 257
# (d, covariates) -> seed of a null case, default 2000 + 100 * d + covariates; replaced when the oracle's fit ends on the boundary
NULL_SEEDS = {(4, 1): 12401, (8, 2): 32802}   # smallest eigenvalue with 2401: 5.8e-5; with 2802 / 12802 / 22802: < 1e-14


def is_fixed(d, cw):
    return (d, cw + 1) in FIXED_SNP


def waves(d, cw, rt=False):
    """SNPs per workgroup of the kernel that takes (d, cw): one wavefront each"""
    if rt or not is_fixed(d, cw):
        return 1
    return 4 if d <= 5 else 2 if d == 6 else 1


def seed_of(d, cw):
    return SEEDS.get((d, cw), 100 * d + cw)


@functools.lru_cache(maxsize=None)
def case(d, cw, seed=None, l=None, rt=False, gxe=False):
    """make_case plus the synthetic interior starting point ("null": what gemma_hip_mvlmm_set takes).  n gives three trips of
    the 64-lane loop, the last with 3 (d <= 5) or 9 lanes; l = 2 * waves + 1 SNPs: two full workgroups and a ragged one.  gxe: an
    environment vector whose rotated row joins the covariates of the start (the null model of the interaction test)."""
    seed = seed_of(d, cw) if seed is None else seed
    n = 131 if d <= 5 else 137
    l = 2 * waves(d, cw, rt or gxe) + 1 if l is None else l
    c = make_case(n, d, cw, l, seed)
    rng = np.random.default_rng(seed + 1000)
    A, B = 0.3 * rng.standard_normal((d, d)), 0.3 * rng.standard_normal((d, d))
    Vg0, Ve0 = A @ A.T + np.eye(d), B @ B.T + 0.8 * np.eye(d)
    W = c["UtW"]
    if gxe:
        c["env"] = rng.standard_normal(n)
        W = np.ascontiguousarray(np.vstack([c["UtW"], (c["U"].T @ c["env"])[None, :]]))
        c["UtX2"] = np.ascontiguousarray((c["G"] * c["env"][None, :]) @ c["U"])
        assert np.all(c["G"].mean(1) <= 1)  # no allele switch (src/mvlmm.cpp:4232-4236)
    c["W_null"] = W
    B0 = np.ascontiguousarray(np.linalg.lstsq(W.T, c["UtY"].T, rcond=None)[0].T)
    logl_H0 = O.mph_em("L", 8, 0.0, c["ev"], W, c["UtY"], Vg0.copy(), Ve0.copy(), B0.copy())  # keeps the LRT statistics moderate
    c["null"] = {"Vg_mle": Vg0, "Ve_mle": Ve0, "B_mle": B0, "logl_mle": logl_H0}
    c["d"], c["cw"], c["n"], c["l"], c["seed"] = d, cw, n, l, seed
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)  # shared among the tests
    for v in c["null"].values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


_REF = {}


def reference(c, a_mode, crt, gxe=False, **over):
    """The oracle's per-SNP block under FIX, computed once per case"""
    key = (c["d"], c["cw"], c["seed"], c["l"], a_mode, crt, gxe, tuple(sorted(over.items())))
    if key not in _REF:
        cfg = O.mv_cfg(**{**FIX, **over}, crt=crt)
        null = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in c["null"].items()}
        if gxe:
            r = O.mvlmm_batch_gxe(a_mode, cfg, np.array(c["ev"]), np.array(c["W_null"]), np.array(c["UtY"]), np.array(c["UtX"]),
                                  np.array(c["UtX2"]), null)
        else:
            r = O.mvlmm_batch(a_mode, cfg, np.array(c["ev"]), np.array(c["UtW"]), np.array(c["UtY"]), np.array(c["UtX"]), null)
        for v in r.values():
            v.setflags(write=False)
        _REF[key] = r
    return _REF[key]


def split(out, d):
    v = d * (d + 1) // 2
    return {"beta": out[:, :d], "Vbeta": out[:, d:d + v], "Vg": out[:, d + v:d + 2 * v], "Ve": out[:, d + 2 * v:d + 3 * v],
            "p_wald": out[:, d + 3 * v], "p_lrt": out[:, d + 3 * v + 1], "p_score": out[:, d + 3 * v + 2]}


def harness_batch(H, c, a_mode, crt, fixed, gxe=False, **over):
    """The kernel source on one CPU lane (tests/host/mvlmm_harness.cpp) under FIX: fixed = 0 the run-time form, 1 the fixed
    instance of the shape; None where the harness holds no such instance."""
    d, n, l = c["d"], c["n"], c["l"]
    o = {**FIX, **over}
    out = np.zeros((l, 3 * (d * (d + 1) // 2) + d + 3))
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    keep = [np.array(c[k]) for k in ("UtX", "ev", "W_null", "UtY")]
    a = MvArgs()
    a.UtX, a.ld, a.l, a.n = P(keep[0]), n, l, n
    a.eval, a.Wt, a.Yt = P(keep[1]), P(keep[2]), P(keep[3])
    for dst, src in ((a.Vg_null, "Vg_mle"), (a.Ve_null, "Ve_mle"), (a.B_null, "B_mle")):
        for i, x in enumerate(c["null"][src].ravel()):
            dst[i] = x
    a.logl_H0, a.a_mode = c["null"]["logl_mle"], a_mode
    a.em_iter, a.em_prec, a.nr_iter, a.nr_prec, a.p_nr = o["em_iter"] // 10, o["em_prec"] * 10, o["nr_iter"] // 10, o["nr_prec"] * 10, o["p_nr"]
    a.out, a.stride, a.crt = P(out), out.shape[1], crt
    rows = keep[2].shape[0] + 1
    if gxe:
        keep.append(np.array(c["UtX2"]))
        a.UtX2 = P(keep[-1])
        rows += 1
    rc = H.mvh_batch2(d, rows, C.byref(a), fixed)
    if fixed and rc == 1:
        return None
    assert rc == 0
    return split(out, d)


def worst_rel(got, ref):
    """Largest relative deviation over all seven fields and ALL SNPs, each field scaled per SNP by its largest reference entry
    (the scaling of _compare in tests/test_gpu_mvlmm.py); nan if a value is not finite."""
    l = np.asarray(ref["p_wald"]).shape[0]
    worst = 0.0
    for k in FIELDS:
        g, r = np.asarray(got[k], dtype=float).reshape(l, -1), np.asarray(ref[k], dtype=float).reshape(l, -1)
        if not np.all(np.isfinite(g)):
            return float("nan")
        scale = np.maximum(np.abs(r).max(axis=1, keepdims=True), 1e-300)
        worst = max(worst, float((np.abs(g - r) / scale).max()))
    return worst


def min_eig(tri, d):
    """smallest eigenvalue over the l symmetric matrices given as packed upper triangles (row by row)"""
    iu = np.triu_indices(d)
    lo = np.inf
    for row in np.asarray(tri).reshape(-1, d * (d + 1) // 2):
        M = np.zeros((d, d))
        M[iu] = row
        M = M + M.T - np.diag(np.diag(M))
        lo = min(lo, float(np.linalg.eigvalsh(M).min()))
    return lo


# ------------------------------------------------------------------ null fits
@functools.lru_cache(maxsize=None)
def null_case(d, cw):
    c = make_case(NULL_N, d, cw, 2, NULL_SEEDS.get((d, cw), 2000 + 100 * d + cw))
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def null_reference(d, cw):
    c = null_case(d, cw)
    return O.mvlmm_null(O.mv_cfg(**FIX), np.array(c["ev"]), np.array(c["UtW"]), np.array(c["UtY"]))


def gls_B(ev, W, Y, Vg, Ve):
    """The GLS estimate of B (d x c) at (Vg, Ve) from the model's definition: per individual k the d x d block H_k = ev_k Vg + Ve,
    sum_k (w_k w_k^T (x) H_k^-1) vec(B) = sum_k vec(H_k^-1 y_k w_k^T)   (W: c x n, Y: d x n)."""
    d, n = Y.shape
    c = W.shape[0]
    A, b = np.zeros((c * d, c * d)), np.zeros(c * d)
    for k in range(n):
        Hi = np.linalg.inv(ev[k] * Vg + Ve)
        w = W[:, k]
        A += np.kron(np.outer(w, w), Hi)
        b += np.kron(w, Hi @ Y[:, k])
    return np.linalg.solve(A, b).reshape(c, d).T

"""Data of the whole-panel null-fit tests (tests/test_null_panel_cpu.py, tests/test_gpu_null_panel.py): trait panels of
multicases.panel with 17 heritabilities between 0 and 0.999 and two planted columns, and the oracle's null fit of every column."""
import json
import os

import numpy as np

import multicases as mc

ROOT = mc.ROOT
FX = os.path.join(ROOT, "tests", "golden", "null_panel")
H2S = [0, 0, .1, .25, .5, .75, .9, .97, .999, .5, .3, 0, .6, .05, .8, .999, .4]
T = len(H2S) + 2  # 19: ragged for every workgroup width
SPAN, ZERO = len(H2S), len(H2S) + 1  # the planted columns
# (n, c) -> seed of multicases.panel.  n below a wavefront at 37 and 61, never a multiple of 64; c = 1, 3, 2, 5: FixedC<0>, <2>, <1>,
# <4>; 6 and 16: the generic form; 18: the wide form
SEEDS = {(203, 1): 11, (203, 3): 12, (61, 2): 13, (37, 5): 15, (1031, 6): 14, (203, 18): 16, (203, 16): 19}
BIT_SHAPES = [(203, 1), (203, 3), (61, 2), (37, 5), (1031, 6), (203, 18)]
ORACLE_SHAPES = [(203, 1), (203, 3), (1031, 6)]
BETA_SHAPES = [(203, 1), (203, 3), (1031, 6), (203, 16)]
L_MIN, L_MAX = 1e-5, 1e5
FIELDS = ("l_mle_null", "logl_mle_H0", "l_remle_null", "logl_remle_H0", "pve", "pve_se", "vg_remle", "ve_remle")
COND_MAX = 1e4  # of UtW' H UtW where beta is compared: random normal covariates and an intercept give O(10)

_PANELS, _ORACLE = {}, {}


def panel(oracle, n, c):
    """(X (4, n), U, ev, UtW (n, c), UtY (n, 19)): the 17 traits, then UtW @ (1 .. c) -- a phenotype in the span of the covariates -- and zeros.
    The arrays are shared between the tests: read-only."""
    key = (n, c)
    if key not in _PANELS:
        X, U, ev, UtW, UtY = mc.panel(oracle, n, 4, c, H2S, SEEDS[key])
        UtY = np.ascontiguousarray(np.hstack([UtY, (UtW @ np.arange(1.0, c + 1.0))[:, None], np.zeros((n, 1))]))
        ev, UtW = np.ascontiguousarray(ev), np.ascontiguousarray(UtW)
        for a in (X, U, ev, UtW, UtY):
            a.setflags(write=False)
        _PANELS[key] = (X, U, ev, UtW, UtY)
    return _PANELS[key]


def oracle_fits(oracle, n, c):
    """(19, 4) array: l_mle, logl_mle, l_remle, logl_remle of every column from the oracle's CalcLambda"""
    key = (n, c)
    if key not in _ORACLE:
        _, _, ev, UtW, UtY = panel(oracle, n, c)
        out = np.empty((T, 4))
        for t in range(T):
            y = np.ascontiguousarray(UtY[:, t])
            out[t, :2] = oracle.calc_lambda_null("L", ev, UtW, y)
            out[t, 2:] = oracle.calc_lambda_null("R", ev, UtW, y)
        out.setflags(write=False)
        _ORACLE[key] = out
    return _ORACLE[key]


def ends(lam):
    """(at l_min, at l_max, strictly inside) counts over the 17 trait columns"""
    lam = np.asarray(lam)[:len(H2S)]
    return int((lam <= L_MIN).sum()), int((lam >= L_MAX).sum()), int(((lam > L_MIN) & (lam < L_MAX)).sum())


def gram_cond(ev, UtW, lam):
    h = 1.0 / (lam * ev + 1.0)
    return float(np.linalg.cond(UtW.T @ (UtW * h[:, None])))


def fx_log(t):
    return json.load(open(os.path.join(FX, "Sb_n%d.log.json" % t)))

"""Data of the score-panel tests (tests/test_score_panel_cpu.py, tests/test_gpu_score_panel.py): a long-double numpy restatement
of the closed form the device kernel evaluates, and trait panels built from multicases.panel with planted degenerate rows.

The closed form (per phenotype t at its null lambda, h_i = 1 / (lambda eval_i + 1), df = n - c - 1):
    S_ww = UtW^T diag(h) UtW = L L^T,  v = S_ww^-1 UtW^T (h . y),  r = y - UtW v,  w~ = UtW L^-T,
    P_yy = sum h y^2 - (UtW^T (h . y)) . v,
    P_xy = sum h x r,   P_xx = sum h x^2 - sum_a (sum h x w~_a)^2,
    beta = P_xy / P_xx,  se = safe_sqrt((P_yy - P_xy^2 / P_xx) / (df P_xx)),  p_score = F_Q(n P_xy^2 / (P_yy P_xx); 1, df)
which is CalcPab's one-covariate-at-a-time elimination (src/lmm.cpp:311-350) written as the full projection."""
import functools

import numpy as np

import multicases as mc

LD = np.longdouble
SCORE_DTYPE = np.dtype([(k, "f8") for k in ("beta", "se", "p_score")])
FIELDS = ("beta", "se", "p_score")
BLOCKS = (1, 1, 130, 130, 300, 300)  # l in {1, 130, 300}, each over two consecutive batches
RTOL = 1e-6  # the project's parity bar (tests/test_gpu_parity.py)
PXX_FLOOR = 1e-8  # a pair is compared unless P_xx < PXX_FLOOR * sum h x^2
# The condition on the inputs of a comparison with the oracle: the oracle's own fp64 recursion is within half the bar of the
# long-double restatement on every compared pair.  beta = P_xy / P_xx passes through zero, the recursion forms P_xy as a difference
# of terms of size 10 (sum h x y - (sum h x w)(sum h w y) / (sum h w w)), and on the pair with the smallest |z| of 86 200 its
# rounding alone is 1e-6 to 1e-5 of beta for most random panels at n = 203 once a null lambda sits at l_max = 1e5: there a relative
# bar against the oracle measures the oracle.  A panel is therefore taken from the first seed of a fixed sequence that meets the
# condition (SEED_STEP; found on the CPU from the oracle and the restatement alone, no device involved), and every test that holds
# the device to the oracle asserts the condition first.
REF_COND = RTOL / 2
# A seed is taken when the oracle's distance from long double is below SEED_MARGIN, 0.4 of the condition (the figure moves by a
# factor of two with the last bits of the inputs).  (n, c, T) -> steps of 100003 added to the panel's seed; every other panel is
# below the margin or meets the condition at step 0.  Along the sequence: (203, 1, 100): 2.6e-6, 6.4e-6, 4.5e-7, 1.8e-6, 7.4e-7,
# 1.6e-6, 1.7e-7 (step 6); (203, 16, 100): 2.3e-6, 4.1e-7, 3.4e-7, 2.6e-6, 3.4e-7, 1.3e-6, 3.0e-6, 1.7e-5, 9.9e-7, 6.1e-7, 3.1e-7,
# 2.5e-7, 3.7e-7, 8.4e-7, 3.2e-7, 4.8e-6, 8.0e-7, 6.3e-7, 1.3e-6, 3.1e-7, 1.2e-7 (step 20).
SEED_MARGIN = 2e-7
SEED_STEP = {(203, 1, 100): 6, (203, 16, 100): 20}


def _safe_sqrt(d):
    """src/mathfunc.cpp:116-131"""
    d = np.where(d < 0.001, np.abs(d), d)
    with np.errstate(invalid="ignore"):
        return np.sqrt(d)


def closed_form(O, ev, UtW, UtY, lams, UtX):
    """(T, l) SCORE_DTYPE records and the (T, l) ratio P_xx / sum h x^2, in long double (the F tail through the oracle's GSL)"""
    ev = np.asarray(ev, dtype=LD)
    W = np.asarray(UtW, dtype=LD).reshape(len(ev), -1)
    Y = np.asarray(UtY, dtype=LD).reshape(len(ev), -1)
    X = np.asarray(UtX, dtype=LD)
    n, c = W.shape
    T, l = Y.shape[1], X.shape[0]
    df = n - c - 1
    X2 = X * X
    out = np.zeros((T, l), dtype=SCORE_DTYPE)
    ratio = np.zeros((T, l))
    for t in range(T):
        h = 1 / (LD(lams[t]) * ev + 1)
        y = Y[:, t]
        S = (W * h[:, None]).T @ W
        Lc = np.zeros((c, c), dtype=LD)
        for j in range(c):
            Lc[j, j] = np.sqrt(S[j, j] - (Lc[j, :j] ** 2).sum())
            for i in range(j + 1, c):
                Lc[i, j] = (S[i, j] - (Lc[i, :j] * Lc[j, :j]).sum()) / Lc[j, j]
        b = W.T @ (h * y)
        z = np.zeros(c, dtype=LD)
        for a in range(c):
            z[a] = (b[a] - (Lc[a, :a] * z[:a]).sum()) / Lc[a, a]
        v = np.zeros(c, dtype=LD)
        for a in range(c - 1, -1, -1):
            v[a] = (z[a] - (Lc[a + 1:, a] * v[a + 1:]).sum()) / Lc[a, a]
        P_yy = (h * y * y).sum() - (z * z).sum()
        r = y - W @ v
        Wt = np.zeros((n, c), dtype=LD)
        for a in range(c):
            Wt[:, a] = (W[:, a] - Wt[:, :a] @ Lc[a, :a]) / Lc[a, a]
        shx2 = X2 @ h
        P_xy = X @ (h * r)
        G = X @ (Wt * h[:, None])
        P_xx = shx2 - (G * G).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            beta = P_xy / P_xx
            Px_yy = P_yy - P_xy * P_xy / P_xx
            se = _safe_sqrt(Px_yy / (df * P_xx))
            stat = n * P_xy * P_xy / (P_yy * P_xx)
            ratio[t] = (P_xx / shx2).astype(np.float64)
        out["beta"][t] = beta.astype(np.float64)
        out["se"][t] = se.astype(np.float64)
        out["p_score"][t] = [O.fdist_Q(float(s), 1.0, float(df)) for s in stat]
    return out, ratio


def h2s_of(T):
    return tuple(np.linspace(0.0, 0.95, T)) if T > 1 else (0.5,)


# blocks of BLOCKS: [0, 1) [1, 2) [2, 132) [132, 262) [262, 562) [562, 862); planted: starts 2, 132, 562, insides 57, 400, ends 131, 561, 861
# (8 of 862 rows: below the 1 % of pairs that may be left out)
PLANTED = (2, 57, 131, 132, 400, 561, 562, 861)


def plant(X):
    """monomorphic (even index) and all-missing (odd) rows at the start of a block, inside it and at its end"""
    X = X.copy()
    for s in PLANTED:
        X[s] = np.nan if s % 2 else 2.0
    return X


@functools.lru_cache(maxsize=None)
def panel(n, c, T, dosage=False, planted=False):
    """X (sum(BLOCKS), n) with NaN, U, eval, UtW, UtY of multicases.panel: heritabilities 0 ... 0.95 over the T traits"""
    from oracle import oracle as O
    O.lib()
    seed = 3000 * n + 10 * c + T + 100003 * SEED_STEP.get((n, c, T), 0)
    X, U, ev, UtW, UtY = mc.panel(O, n, sum(BLOCKS), c, h2s_of(T), seed=seed, dosage=dosage)
    if planted:
        X = plant(X)
    return X, U, ev, UtW, UtY


def cut(X, sizes=BLOCKS):
    out, s0 = [], 0
    for l in sizes:
        out.append(np.ascontiguousarray(X[s0:s0 + l]))
        s0 += l
    return out


def oracle_records(O, ev, UtW, UtY, lams, UtX):
    """(T, l) records of the oracle's mode 3 (CalcRLScore on CalcPab's recursion, fp64) on a given U^T x"""
    T = UtY.shape[1]
    out = np.zeros((T, UtX.shape[0]), dtype=SCORE_DTYPE)
    for t in range(T):
        rec = O.lmm_batch_UtX(3, ev, UtW, np.ascontiguousarray(UtY[:, t]), UtX, l_mle_null=float(lams[t]))
        for k in FIELDS:
            out[k][t] = rec[k]
    return out


def rel_err(got, want):
    """per field: |got - want| / |want| (0 where both are NaN, inf where one is)"""
    res = {}
    for k in FIELDS:
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        both = np.isnan(g) & np.isnan(w)
        with np.errstate(divide="ignore", invalid="ignore"):
            e = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        e = np.where(both, 0.0, e)
        res[k] = np.where(np.isnan(e), np.inf, e)
    return res


def nulls(O, ev, UtW, UtY):
    """the fitted null lambda (MLE) of every column, by the oracle: the same values on every machine"""
    return np.array([O.calc_lambda_null("L", ev, UtW, np.ascontiguousarray(UtY[:, t]))[0] for t in range(UtY.shape[1])])

"""The univariate LMM written from the model, not from CalcPab's recursion: the reference of tests/test_lmm_definition_cpu.py and
tests/test_gpu_lmm_definition.py.  Everything is numpy long double, vectorised over the SNPs of a case; the p-values are mpmath at
40 digits.

In the rotated basis (eval, UtW, Uty, rows of UtX), with h = 1 / (lambda eval + 1) and V = [UtW, x] (V = UtW for the null model):
    A = V' diag(h) V,  b = V' (h . y),  beta = A^-1 b (Cholesky elimination),  yPy = sum h y^2 - b . beta,
    se(beta_x) = sqrt(A^-1[x, x] yPy / df),  df = n - c - 1,
    REML log-likelihood = 1/2 d (log d - log 2 pi - 1) - 1/2 log|H| - 1/2 (log|A| - log|V'V|) - 1/2 d log yPy,  d = n - columns of V,
    ML   log-likelihood = 1/2 n (log n - log 2 pi - 1) - 1/2 log|H| - 1/2 n log yPy,
the additive constants as LogRL_f / LogL_f have them (src/lmm.cpp:799-864, :484-542), the V'V term being the reference's Iab.
Score statistic at the null lambda: n P_xy^2 / (P_yy P_xx) with P_xx = 1 / A^-1[x, x], P_xy = beta_x P_xx and P_yy the null
model's yPy.  The derivatives behind se(pve) come from the dense projection P = H^-1 - H^-1 W (W' H^-1 W)^-1 W' H^-1 itself:
    dl/dlambda = -1/2 tr(PK) + 1/2 d yPKPy / yPy,   d2l/dlambda2 = 1/2 tr(PKPK) - 1/2 d (2 yPKPKPy yPy - yPKPy^2) / yPy^2."""
import numpy as np

import multicases as mc

LD = np.longdouble
H2S = (0.0, 0.3, 0.999)
SCAN = 16  # scan points per grid interval
GOLD_ITERS = 90  # 0.618^90 = 1.5e-19 of two scan steps
FIELDS = ("beta", "se", "lambda_remle", "lambda_mle", "p_wald", "p_lrt", "p_score", "logl_H1")  # SUMSTAT order (src/param.h:54-66)
LOG2PI = np.log(8 * np.arctan(LD(1)))


def _ld(a):
    return np.asarray(a, dtype=LD)


def _chol(A):
    """lower Cholesky factors of the (L, m, m) stack A and log|A|"""
    L_, m, _ = A.shape
    F = np.zeros_like(A)
    for j in range(m):
        d = A[:, j, j] - (F[:, j, :j] ** 2).sum(axis=1)
        with np.errstate(invalid="ignore"):
            F[:, j, j] = np.sqrt(d)
        if j + 1 < m:
            F[:, j + 1:, j] = (A[:, j + 1:, j] - np.einsum("lik,lk->li", F[:, j + 1:, :j], F[:, j, :j])) / F[:, j, j, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        logdet = 2 * np.log(np.einsum("ljj->lj", F)).sum(axis=1)
    return F, logdet


def _chol_solve(F, B):
    """A^-1 B for the (L, m, k) stack B, A = F F'"""
    m = F.shape[1]
    Z = np.zeros_like(B)
    for i in range(m):
        Z[:, i] = (B[:, i] - np.einsum("lk,lkj->lj", F[:, i, :i], Z[:, :i])) / F[:, i, i, None]
    X = np.zeros_like(B)
    for i in range(m - 1, -1, -1):
        X[:, i] = (Z[:, i] - np.einsum("lk,lkj->lj", F[:, i + 1:, i], X[:, i + 1:])) / F[:, i, i, None]
    return X


class Model:
    """L problems over one (eval, UtW): row s has the phenotype Y[s] (or the one y) and, when X is given, the tested vector X[s]"""

    def __init__(self, ev, UtW, Uty, UtX=None):
        self.ev = _ld(ev)
        self.n = len(self.ev)
        self.W = _ld(UtW).reshape(self.n, -1)
        self.c = self.W.shape[1]
        Y = _ld(Uty)
        self.Y = Y.reshape(1, self.n) if Y.ndim == 1 else Y  # (1 or L, n)
        self.X = None if UtX is None else _ld(UtX)
        self.L = self.X.shape[0] if self.X is not None else self.Y.shape[0]
        self.m = self.c + (self.X is not None)
        iu = np.triu_indices(self.c)
        self._iu = iu
        self.WW = self.W[:, iu[0]] * self.W[:, iu[1]]  # (n, c (c + 1) / 2)
        self.Y2 = self.Y * self.Y
        if self.X is not None:
            self.X2, self.XY = self.X * self.X, self.X * self.Y
        self.df_wald = self.n - self.c - 1
        self.logdet_VV = self._gram(np.ones((1, self.n), dtype=LD))[3]

    def _gram(self, h):
        """A (L, m, m), b (L, m), sum h y^2 (L,), log|A| and the factor, for h of shape (1 or L, n)"""
        c, m, L_ = self.c, self.m, self.L
        A = np.zeros((L_, m, m), dtype=LD)
        b = np.zeros((L_, m), dtype=LD)
        S = h @ self.WW
        A[:, self._iu[0], self._iu[1]] = S
        A[:, self._iu[1], self._iu[0]] = S
        b[:, :c] = (h * self.Y) @ self.W
        if self.X is not None:
            g = (h * self.X) @ self.W
            A[:, c, :c] = g
            A[:, :c, c] = g
            A[:, c, c] = (h * self.X2).sum(axis=1)
            b[:, c] = (h * self.XY).sum(axis=1)
        yy = np.broadcast_to((h * self.Y2).sum(axis=1), (L_,))
        F, logdet = _chol(A)
        return A, b, yy, logdet, F

    def at(self, lam):
        """dict of (L,) long-double arrays at lambda (a scalar, or one value per row)"""
        lam = np.atleast_1d(_ld(lam)).reshape(-1, 1)
        v = lam * self.ev + 1
        h = 1 / v
        logdet_H = np.broadcast_to(np.log(np.abs(v)).sum(axis=1), (self.L,))
        A, b, yy, logdet_A, F = self._gram(h)
        m, n = self.m, self.n
        rhs = np.zeros((self.L, m, 2), dtype=LD)
        rhs[:, :, 0] = b
        rhs[:, m - 1, 1] = 1
        sol = _chol_solve(F, rhs)
        beta = sol[:, :, 0]
        yPy = yy - (b * beta).sum(axis=1)
        d = LD(n - m)
        with np.errstate(invalid="ignore", divide="ignore"):
            reml = d / 2 * (np.log(d) - LOG2PI - 1) - logdet_H / 2 - (logdet_A - self.logdet_VV) / 2 - d / 2 * np.log(yPy)
            ml = LD(n) / 2 * (np.log(LD(n)) - LOG2PI - 1) - logdet_H / 2 - LD(n) / 2 * np.log(yPy)
        out = {"beta_all": beta, "yPy": yPy, "reml": reml, "ml": ml, "F": F, "h": h}
        if self.X is not None:
            axx = sol[:, m - 1, 1]
            with np.errstate(invalid="ignore", divide="ignore"):
                out["beta"] = beta[:, m - 1]
                out["se"] = np.sqrt(axx * yPy / self.df_wald)
                out["wald"] = out["beta"] ** 2 / (axx * yPy / self.df_wald)
                out["P_xx"] = 1 / axx
                out["ratio"] = out["P_xx"] / A[:, m - 1, m - 1]  # P_xx / sum h x^2
        return out

    def score(self, lam_null, null_model):
        """beta, se at the null lambda and the score statistic n P_xy^2 / (P_yy P_xx)"""
        r = self.at(lam_null)
        P_yy = null_model.at(lam_null)["yPy"]
        r["score"] = self.n * r["beta"] ** 2 * r["P_xx"] / P_yy
        return r

    def maximise(self, reml, l_min=1e-5, l_max=1e5, n_region=10):
        """(lambda*, logl(lambda*), scan values (K + 1, L), scan lambdas): SCAN points per grid interval in log lambda and the
        ends, then golden section over the two scan steps around the best point"""
        key = "reml" if reml else "ml"
        K = SCAN * n_region
        t = np.log(LD(l_min)) + (np.log(LD(l_max)) - np.log(LD(l_min))) * np.arange(K + 1, dtype=LD) / K
        lams = np.exp(t)
        lams[0], lams[-1] = l_min, l_max
        vals = np.stack([self.at(lams[k])[key] for k in range(K + 1)])
        kb = np.argmax(np.where(np.isnan(vals), -np.inf, vals), axis=0)
        a, b = t[np.maximum(kb - 1, 0)].copy(), t[np.minimum(kb + 1, K)].copy()
        g = (np.sqrt(LD(5)) - 1) / 2
        x1, x2 = b - g * (b - a), a + g * (b - a)
        f1, f2 = self.at(np.exp(x1))[key], self.at(np.exp(x2))[key]
        for _ in range(GOLD_ITERS):
            left = f1 >= f2  # the maximum is in [a, x2]
            b = np.where(left, x2, b)
            a = np.where(left, a, x1)
            nx1, nx2 = b - g * (b - a), a + g * (b - a)
            # one new point per row: the kept inner point moves to the other slot
            x_new = np.where(left, nx1, nx2)
            f_new = self.at(np.exp(x_new))[key]
            f1, f2 = np.where(left, f_new, f2), np.where(left, f1, f_new)
            x1, x2 = nx1, nx2
        lam = np.exp((a + b) / 2)
        f = self.at(lam)[key]
        # an end of the grid is the maximiser when nothing inside its cell is higher
        for end, k_end in ((LD(l_min), 0), (LD(l_max), K)):
            take = (kb == k_end) & (vals[k_end] >= f)
            lam, f = np.where(take, end, lam), np.where(take, vals[k_end], f)
        return lam, f, vals, lams

    def derivs(self, lam):
        """(dl/dlambda, d2l/dlambda2) of the REML log-likelihood of the null model (X is None), per row, through the dense P"""
        assert self.X is None
        lam = np.broadcast_to(np.atleast_1d(_ld(lam)), (self.L,))
        d1, d2 = np.zeros(self.L, dtype=LD), np.zeros(self.L, dtype=LD)
        K, W, d = self.ev, self.W, LD(self.n - self.c)
        for s in range(self.L):
            h = 1 / (lam[s] * K + 1)
            hW = W * h[:, None]
            F, _ = _chol((W.T @ hW)[None])
            P = np.diag(h) - hW @ _chol_solve(F, hW.T[None])[0]
            y = self.Y[min(s, self.Y.shape[0] - 1)]
            Py = P @ y
            yPy, yPKPy = y @ Py, Py @ (K * Py)
            yPKPKPy = (K * Py) @ (P @ (K * Py))
            trPK = (np.diag(P) * K).sum()
            trPKPK = ((P * P) * np.outer(K, K)).sum()
            d1[s] = -trPK / 2 + d / 2 * yPKPy / yPy
            d2[s] = trPKPK / 2 - d / 2 * (2 * yPKPKPy * yPy - yPKPy * yPKPy) / (yPy * yPy)
        return d1, d2

    def null_fit(self, lam_remle, trace_G):
        """pve, pve_se, vg, ve, covariate beta (L, c) and se (L, c) at the REML lambda: CalcPve / CalcLmmVgVeBeta by definition"""
        assert self.X is None
        r = self.at(lam_remle)
        lam = np.broadcast_to(np.atleast_1d(_ld(lam_remle)), (self.L,))
        ve = r["yPy"] / (self.n - self.c)
        eye = np.broadcast_to(np.eye(self.c, dtype=LD), (self.L, self.c, self.c)).copy()
        Ainv = _chol_solve(r["F"], eye)
        _, d2 = self.derivs(lam)
        tg = LD(trace_G)
        with np.errstate(invalid="ignore", divide="ignore"):
            pve_se = tg / (tg * lam + 1) ** 2 * np.sqrt(-1 / d2)
            se = np.sqrt(np.einsum("ljj->lj", Ainv) * ve[:, None])
        return {"pve": tg * lam / (tg * lam + 1), "pve_se": pve_se, "vg": ve * lam, "ve": ve, "beta": r["beta_all"], "se": se, "d2": d2}


# ------------------------------------------------------------------------------------------------ p-values
_P = {}


def p_f(stat, df):
    """upper tail of F(1, df) at stat: I_{df / (df + F)}(df / 2, 1 / 2), mpmath at 40 digits"""
    import mpmath as mp
    key = ("f", float(stat), int(df))
    if key not in _P:
        with mp.workdps(40):
            x, d = mp.mpf(float(stat)), mp.mpf(int(df))
            _P[key] = mp.betainc(d / 2, mp.mpf(1) / 2, 0, d / (d + x), regularized=True)
    return _P[key]


def p_chi1(x):
    """upper tail of chi^2_1 at x: erfc(sqrt(x / 2))"""
    import mpmath as mp
    key = ("c", float(x))
    if key not in _P:
        with mp.workdps(40):
            _P[key] = mp.erfc(mp.sqrt(mp.mpf(float(x)) / 2))
    return _P[key]


def p_rel(got, want):
    """|got - want| / want for a double against an mpmath value"""
    import mpmath as mp
    with mp.workdps(40):
        return float(abs(mp.mpf(float(got)) - want) / want)


# ------------------------------------------------------------------------------------------------ lambda-hat criteria
LAM_A = 2e-5  # (a): the stopping rule |x_new - x_old| < 1e-5 |x_new| reports the iterate before the last; 2 x over the 9.9e-6 measured
LAM_B = 1e-9  # (b): no scan point above logl(lambda-hat) by more than this, relative
TWO_MAX = 1e-9  # two local maxima of the scan this close (relative): the SNP is left out
LEFT_OUT_MAX = 0.02


def local_maxima(vals):
    """per column of the scan: the values of its local maxima (ends included), best first -> (second best / nan, count)"""
    K1, L_ = vals.shape
    v = np.where(np.isnan(vals), -np.inf, vals)
    up = np.vstack([np.full((1, L_), True), v[1:] > v[:-1]])
    down = np.vstack([v[:-1] >= v[1:], np.full((1, L_), True)])
    is_max = up & down
    second = np.full(L_, -np.inf, dtype=LD)
    for s in range(L_):
        m = np.sort(v[is_max[:, s], s])[::-1]
        if len(m) > 1:
            second[s] = m[1]
    return second, is_max.sum(axis=0)


def lambda_criteria(lam_hat, logl_at_hat, lam_star, vals, lams, l_min, l_max):
    """(ok (L,), left_out (L,), text): criteria (a)-(c) on every row that is not left out -- a failed search (NaN) or two local
    maxima of the scan within TWO_MAX of each other"""
    lam_hat = np.asarray(lam_hat, dtype=np.float64)
    best = np.nanmax(np.where(np.isnan(vals), -np.inf, vals), axis=0)
    second, _ = local_maxima(vals)
    left = np.isnan(lam_hat) | (np.abs(best - second) <= TWO_MAX * np.abs(best))
    K = len(lams) - 1
    kb = np.argmax(np.where(np.isnan(vals), -np.inf, vals), axis=0)
    inside = (lam_hat > l_min) & (lam_hat < l_max)
    with np.errstate(invalid="ignore"):
        rel = np.abs(_ld(lam_hat) - lam_star) / lam_star
        a_ok = ~inside | (rel <= LAM_A)
        b_ok = (best - logl_at_hat) <= LAM_B * np.abs(logl_at_hat)
        c_ok = inside | ((lam_hat <= l_min) & (kb <= SCAN)) | ((lam_hat >= l_max) & (kb >= K - SCAN))
    ok = left | (a_ok & b_ok & c_ok)
    worst_a = float(np.max(np.where(inside & ~left, rel, 0))) if len(rel) else 0.0
    with np.errstate(invalid="ignore"):
        gap = np.where(left, 0, (best - logl_at_hat) / np.abs(logl_at_hat))
    text = "interior %d, at l_min %d, at l_max %d, left out %d; (a) worst %.3g; (b) worst %.3g; fails a/b/c %d/%d/%d" % (
        int((inside & ~left).sum()), int((lam_hat <= l_min).sum()), int((lam_hat >= l_max).sum()), int(left.sum()), worst_a,
        float(np.nanmax(gap)) if len(gap) else 0.0, int((~a_ok & ~left).sum()), int((~b_ok & ~left).sum()), int((~c_ok & ~left).sum()))
    return ok, left, text


# ------------------------------------------------------------------------------------------------ bars
# max over every case, trait and compared pair of |oracle - reference| / |reference| at the oracle's own lambda-hat (Wald at the
# REML lambda-hat and the score test's beta, se at the null ML lambda; REML and ML logl_H1), as measured by
# tests/test_lmm_definition_cpu.py on the cases below:
# beta 1.09e-11 (n = 129, c = 4, h2 = 0.3, one SNP whose beta passes near zero; 2.1e-12 on traits at lambda-hat = l_max, 1e-13
# elsewhere), se 5.40e-14, logl 2.45e-13.  That test allows the oracle twice these (another compiler's rounding of the
# oracle); the device's bars are 1e3 times these values themselves.
D_BETA = 1.1e-11
D_SE = 5.4e-14
D_LOGL = 2.5e-13
# the null fits of the tests/nullpanelcases.py panels (c = 1, 3, 6, 18), the oracle's CalcLambda / CalcPve / CalcLmmVgVeBeta at the
# oracle's own lambda-hat against Model.null_fit, measured by the same module: logl 1.37e-12 (ML fits at l_max; 1e-15 inside),
# se(pve) 3.29e-12 where the REML lambda-hat is inside the grid, pve 1.5e-16, vg and ve 2.2e-15, the covariates' beta 4.5e-15 of
# max(|beta|, se) (planted effects are near zero) and their se 1.9e-15
D_NULL = {"logl": 1.4e-12, "pve_se": 3.3e-12, "pve": 1.6e-16, "vg": 2.2e-15, "ve": 2.1e-15, "beta": 4.6e-15, "se": 2e-15}
DEV_FACTOR = 1e3  # the series' 6e-15 of a sum's scale is 60 x fp64 rounding, then the MFMA summation order and the 2-ulp recip
DEV_FLOOR = 1e-10
RTOL = 1e-6  # the project's parity bar (tests/test_gpu_parity.py)
RATIO_MIN = 1e-3  # pairs with P_xx / sum h x^2 below are counted, not compared: 6e-15 of the sum is then above 6e-12 of P_xx
# the oracle's tails against mpmath on df in {28, 57, 199, 1027}, x in [1e-8, 1e4], p >= 6e-300: 8.8e-13 (F) and 9.1e-14 (chi^2_1) were
# measured when the bars were set, 5.4e-13 and 8.0e-14 on the grid of that test
P_F_BAR = 2e-12
P_CHI_BAR = 2e-13

GRIDS = {"default": dict(l_min=1e-5, l_max=1e5, n_region=10), "region7": dict(l_min=1e-5, l_max=1e5, n_region=7),
         "region16": dict(l_min=1e-5, l_max=1e5, n_region=16), "shifted": dict(l_min=3e-5, l_max=3e5, n_region=10)}


def dev_bar(d_k):
    """the device's bar on a field from the oracle's distance d_k, never above the project's 1e-6"""
    return min(max(DEV_FACTOR * d_k, DEV_FLOOR), RTOL)


# ------------------------------------------------------------------------------------------------ cases
# (n, c) -> SNPs of the case.  The table + series path: n below a wavefront, at 64, one past, 129, 203 and 1031 (table_ksplit = 2);
# the generic kernel at c = 6 and 16 and the wide one at 18 with fewer SNPs (their long-double Gram matrices are 19 x 19)
DEFAULT_SHAPES = ((31, 1), (64, 2), (65, 3), (129, 4), (203, 1), (1031, 2))
SWITCH_SHAPE = (203, 3)
WIDE_SHAPES = ((203, 6), (203, 16), (203, 18))
N_SNPS = {(203, 6): 24, (203, 16): 16, (203, 18): 16, (1031, 2): 32}
PLANT = (8, 60, 160, 250)  # -log10 p aimed at by the planted rows (at most 0.75 df: x never comes closer to y than 1 - r^2 = 0.03)
_CASES, _REF = {}, {}


def n_snps(n, c):
    return N_SNPS.get((n, c), 64)


def _resid(W, v):
    return v - W @ np.linalg.lstsq(W, v, rcond=None)[0]


def case(oracle, n, c):
    """dict(U, ev, UtW, UtY (n, 3), UtX (l, n)), read-only: multicases.panel with heritabilities 0, 0.3, 0.999.

    The phenotypes and all SNP rows but the last of a 64-SNP case are centred (their component along U^T 1 is removed; the
    intercept is a covariate, so the model is unchanged).  Uncentred, sum h x^2 and sum h y^2 at lambda = l_max are one term of size
    n on the kinship's zero eigenvalue beside n - 1 terms of size 1e-5: P_xx / sum h x^2 is 1e-5 on every SNP of a trait whose
    lambda-hat is l_max, the oracle's own fp64 recursion is 1e-8 from long double there (measured: 9.6e-9 in logl, 3e-8 in se at
    n = 31), and neither the leave-out cap nor a bar from the oracle's distance could hold.  That regime stays with the 1e-6
    parity tests; the one raw row keeps the leave-out rule in use.

    The first 3 * len(PLANT) rows are planted on the traits in turn: x = y_t + s x with s from the aimed -log10 p and the residual
    norms after the covariates, so that p_wald, p_score and p_lrt run from 1 to far below 1e-150 without reaching 0."""
    key = (n, c)
    if key not in _CASES:
        l = n_snps(n, c)
        X, U, ev, UtW, UtY = mc.panel(oracle, n, l, c, H2S, seed=52000 + 10 * n + c)
        UtX = np.ascontiguousarray(oracle.impute_mean(X) @ U)
        q = U.T @ np.full(n, 1.0 / np.sqrt(n))
        keep_raw = l - 1 if l == 64 else l
        UtX[:keep_raw] -= np.outer(UtX[:keep_raw] @ q, q)
        UtY = UtY - np.outer(q, q @ UtY)
        df = n - c - 1
        for k in range(3 * len(PLANT)):
            y, z = UtY[:, k % 3], UtX[k].copy()
            one_minus_r2 = 10.0 ** (-2.0 * min(PLANT[k // 3], 0.75 * df) / df)
            yp, zp = _resid(UtW, y), _resid(UtW, z)
            UtX[k] = y + np.sqrt((yp @ yp) / (zp @ zp) * one_minus_r2 / (1.0 - one_minus_r2)) * z
        d = dict(U=np.ascontiguousarray(U), ev=np.ascontiguousarray(ev), UtW=np.ascontiguousarray(UtW), UtY=np.ascontiguousarray(UtY),
                 UtX=np.ascontiguousarray(UtX))
        for a in d.values():
            a.setflags(write=False)
        _CASES[key] = d
    return _CASES[key]


def models(oracle, n, c, t):
    """(alternative model over the case's SNPs, null model) of trait t, cached"""
    key = ("m", n, c, t)
    if key not in _REF:
        d = case(oracle, n, c)
        y = d["UtY"][:, t]
        _REF[key] = (Model(d["ev"], d["UtW"], y, d["UtX"]), Model(d["ev"], d["UtW"], y))
    return _REF[key]


def maximum(oracle, n, c, t, reml, l_min=1e-5, l_max=1e5, n_region=10):
    """Model.maximise of the alternative model of (case, trait), computed once"""
    key = ("x", n, c, t, bool(reml), l_min, l_max, n_region)
    if key not in _REF:
        _REF[key] = models(oracle, n, c, t)[0].maximise(reml, l_min, l_max, n_region)
    return _REF[key]


def null_model(oracle, n, c):
    """the null model over the 17 traits of the nullpanelcases panel (n, c), one row per trait, cached"""
    import nullpanelcases as nc
    key = ("n", n, c)
    if key not in _REF:
        _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
        _REF[key] = Model(ev, UtW, UtY[:, :len(nc.H2S)].T)
    return _REF[key]


def null_maximum(oracle, n, c, reml):
    key = ("nx", n, c, bool(reml))
    if key not in _REF:
        _REF[key] = null_model(oracle, n, c).maximise(reml)
    return _REF[key]


def rel(got, want):
    """|got - want| / |want| against a long-double reference, as float64"""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (np.abs(_ld(got) - want) / np.abs(want)).astype(np.float64)

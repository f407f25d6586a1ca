"""The per-SNP stage of -lmm 1..4 (LMM.setup + LMM.assoc on device tensors: the table product, the Chebyshev series in log lambda,
the search, the variant kernels and the device F / chi^2 tails) and the null fits (CalcLambdaNull, CalcLambdaNullPanel) against the
model's definition -- tests/lmmdefcases.py, long double and mpmath -- not against the oracle, which restates the same recursions
and the same GSL algorithms.  tests/test_lmm_definition_cpu.py establishes on the CPU what is asked here:

* at the DEVICE's own lambda-hat, beta, se and logl_H1 within dev_bar(d_k) = min(max(1e3 d_k, 1e-10), 1e-6) of the reference
  evaluated at that lambda-hat, d_k being the oracle's own distance (lmmdefcases.D_BETA, D_SE, D_LOGL, D_NULL): beta 1.1e-8, se 1e-10,
  logl 2.5e-10; pairs with P_xx / sum h x^2 < 1e-3 are counted, not compared, at most 2 % of a case;
* the device's lambda-hat under criteria (a)-(c) of lmmdefcases.lambda_criteria: GEMMA reports the Newton iterate before the one
  that met the stopping rule, so an interior lambda-hat is held to 2e-5 of the maximiser, no scan point may lie 1e-9 |logl| above
  logl(lambda-hat), and a lambda-hat at an end of the grid needs the scan's maximum in the outermost cell;
* p_wald, p_score and p_lrt against mpmath at the device's own statistic -- (beta / se)^2, n beta^2 / (df se^2 + beta^2) (which is
  n P_xy^2 / (P_yy P_xx) written in the beta and se of the score evaluation: P_yy cancels) and 2 (logl_H1 - logl_mle_H0) -- within
  16 x the oracle's bars (3.2e-11 for the F tail, 3.2e-12 for chi^2_1: at p = 1e-300 one ulp of the exponential's argument is
  7.6e-14).  In mode 4 beta and se are the Wald ones, so its p_score is held to the statistic of the mode 3 run of the same case.
  The planted rows take p from 1 to below 1e-150 on both sides of F = df.  df stays below 1030: the asymptotic branches of the
  incomplete beta function for a > 1e5 need df > 2e5 and are out of scope.

Observed on an MI355X (worst over all 172 comparisons of this module; every one is a line of the parity report that
test_gpu_parity._record appends to):
    Wald beta 6.4e-13, se 1.7e-14; score beta 1.07e-11 (the SNP whose beta passes near zero, where the oracle is at 1.09e-11), se 1.3e-14;
    logl_H1 5.6e-14 (REML), 6.5e-14 (ML); p_wald 3.4e-12, p_score 8.5e-13, p_lrt 7.5e-14; interior lambda-hat at most 9.94e-6
    (REML) and 9.92e-6 (ML) from the maximiser, no row fails (b) or (c), no search failed; the one uncentred row of a 64-SNP case
    is the only pair left out, where lambda is l_max;
    null fits: logl 8.7e-13, se(pve) 8.1e-13, pve 2.2e-16, vg 6.0e-16, ve 5.9e-16, beta 9.4e-16 of max(|beta|, se), se(beta) 3.2e-16,
    lambda-hat at most 9.91e-6 from the maximiser.
No bar was missed: the device is within a few ulp-scaled sums of the definition wherever the oracle is."""
import os

import numpy as np
import pytest

import lmmdefcases as D
import nullpanelcases as nc
from test_gpu_parity import _record
from test_lmm_definition_cpu import NULL_SHAPES, null_distances

pytestmark = pytest.mark.gpu
LD = np.longdouble
BAR = {"beta": D.dev_bar(D.D_BETA), "se": D.dev_bar(D.D_SE), "logl_H1": D.dev_bar(D.D_LOGL)}
P_BAR = {"f": 16 * D.P_F_BAR, "chi": 16 * D.P_CHI_BAR}
SWITCHES = {"cheb0": {"GEMMA_HIP_ASSOC_CHEB": "0"}, "grid0": {"GEMMA_HIP_ASSOC_GRID": "0"},
            "final_series0": {"GEMMA_HIP_ASSOC_FINAL_SERIES": "0"}, "force_generic": {"GEMMA_HIP_FORCE_GENERIC": "1"}}
_RUNS, _NULLS = {}, {}


def _dev(a):
    import torch
    return torch.tensor(np.array(a), dtype=torch.float64, device="cuda")


def _null(api, oracle, n, c, t, grid):
    """the device's own null fit of the trait: l_mle_null and logl_mle_H0 of the runs below"""
    key = (n, c, t, grid)
    if key not in _NULLS:
        d = D.case(oracle, n, c)
        _NULLS[key] = api.CalcLambdaNull(d["ev"], d["UtW"], np.ascontiguousarray(d["UtY"][:, t]), trace_G=float(d["ev"].mean()), **D.GRIDS[grid])
    return _NULLS[key]


def _run(api, oracle, n, c, t, mode, grid="default", switch=None, blocks=None):
    """(l, 8) records of LMM.setup + LMM.assoc on device tensors, the case's SNPs in one block or in the given blocks of row indices"""
    import torch
    key = (n, c, t, mode, grid, switch, None if blocks is None else tuple(map(tuple, blocks)))
    if key in _RUNS:
        return _RUNS[key]
    d = D.case(oracle, n, c)
    null = _null(api, oracle, n, c, t, grid)
    saved = {k: os.environ.get(k) for k in (SWITCHES[switch] if switch else {})}
    os.environ.update(SWITCHES[switch] if switch else {})
    try:
        lmm = api.LMM(a_mode=mode, l_mle_null=null["l_mle_null"], logl_mle_H0=null["logl_mle_H0"], **D.GRIDS[grid])
        lmm.setup(_dev(d["U"]), _dev(d["ev"]), _dev(d["UtW"]), _dev(d["UtY"][:, t]))
        try:
            outs = [lmm.assoc(_dev(d["UtX"][np.asarray(idx)])) for idx in (blocks or [np.arange(len(d["UtX"]))])]
            torch.cuda.synchronize()
            out = np.concatenate([o.cpu().numpy() for o in outs])
        finally:
            lmm.finish()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    out.setflags(write=False)
    _RUNS[key] = out
    return out


def _p_check(tag, kind, got, stats, df, keep, fails):
    """device p-values against mpmath at the given statistics; returns (worst, smallest p, largest p)"""
    worst, lo, hi = 0.0, 1.0, 0.0
    for s in np.flatnonzero(keep):
        x = float(stats[s])
        if kind == "chi" and x <= 0:
            want_one = got[s] == 1.0  # gsl_cdf_chisq_Q of a non-positive statistic
            if not want_one:
                fails.append("%s: p_lrt %r at statistic %r" % (tag, got[s], x))
            continue
        want = D.p_f(x, df) if kind == "f" else D.p_chi1(x)
        e = D.p_rel(got[s], want)
        worst, lo, hi = max(worst, e), min(lo, float(got[s])), max(hi, float(got[s]))
        if not (e <= P_BAR[kind]) or not (got[s] > 0):
            fails.append("%s: p %r, mpmath %s at statistic %r: rel %.3g > %.3g" % (tag, got[s], want, x, e, P_BAR[kind]))
    return worst, lo, hi


def _check(oracle, n, c, t, mode, out, grid="default", tag="", idx=None, score_out=None):
    """every assertion of this module on one block of records; `idx`: the case's rows behind the records"""
    d = D.case(oracle, n, c)
    g = D.GRIDS[grid]
    idx = np.arange(len(d["UtX"])) if idx is None else np.asarray(idx)
    y = d["UtY"][:, t]
    alt, nul = D.Model(d["ev"], d["UtW"], y, d["UtX"][idx]), D.models(oracle, n, c, t)[1]
    rec = {k: out[:, j] for j, k in enumerate(D.FIELDS)}
    df = n - c - 1
    fails, notes, seen = [], [], {}
    tag = "lmmdef[n=%d c=%d trait %d mode %d %s%s]" % (n, c, t, mode, grid, (" " + tag) if tag else "")

    def cmp(field, got, want, keep, what):
        e = D.rel(got, want)
        e = np.where(np.isnan(e), np.inf, e)[keep]
        worst = float(e.max()) if len(e) else 0.0
        seen[what] = worst
        if worst > BAR[field]:
            s = np.flatnonzero(keep)[int(np.argmax(e))]
            fails.append("%s: %s rel %.3g > %.3g at row %d (got %r, reference %.17g)" % (tag, what, worst, BAR[field], s, got[s], float(want[s])))

    def lam_check(reml, lam_hat, ref, failed):
        lam_star, _, vals, lams = D.maximum(oracle, n, c, t, reml, **g)
        # the leave-out share of the comparison on the reference alone, before anything of the device's is looked at
        assert (alt.at(lam_star[idx])["ratio"] < D.RATIO_MIN).mean() <= D.LEFT_OUT_MAX
        ok, left, text = D.lambda_criteria(np.where(failed, np.nan, lam_hat), ref["reml" if reml else "ml"], lam_star[idx], vals[:, idx], lams,
                                           g["l_min"], g["l_max"])
        notes.append("%s lambda-hat: %s" % ("REML" if reml else "ML", text))
        if left.mean() > D.LEFT_OUT_MAX:
            fails.append("%s: %d of %d lambda-hats left out" % (tag, int(left.sum()), len(idx)))
        if not ok.all():
            fails.append("%s: %s lambda-hat fails the criteria at rows %s: %s" % (tag, "REML" if reml else "ML", np.flatnonzero(~ok)[:8], text))

    def keep_of(ref, failed):
        low = np.asarray(ref["ratio"] < D.RATIO_MIN)
        if (low | failed).mean() > D.LEFT_OUT_MAX:
            fails.append("%s: %d of %d pairs left out" % (tag, int((low | failed).sum()), len(idx)))
        notes.append("left out %d" % int((low | failed).sum()))
        return ~(low | failed)

    if mode in (1, 4):
        failed = np.isnan(rec["lambda_remle"]) | np.isnan(rec["beta"])  # a failed search: NaN (src/lmm.cpp:2087-2094)
        lam = np.where(failed, 1.0, rec["lambda_remle"])
        ref = alt.at(lam)
        lam_check(True, rec["lambda_remle"], ref, failed)
        keep = keep_of(ref, failed)
        cmp("beta", rec["beta"], ref["beta"], keep, "beta")
        cmp("se", rec["se"], ref["se"], keep, "se")
        if mode == 1:
            cmp("logl_H1", rec["logl_H1"], ref["reml"], keep, "logl_H1(REML)")
        F = (rec["beta"].astype(LD) / rec["se"].astype(LD)) ** 2
        seen["p_wald"], lo, hi = _p_check(tag + " p_wald", "f", rec["p_wald"], F, df, keep, fails)
        notes.append("p_wald in [%.3g, %.3g]" % (lo, hi))
    if mode in (2, 4):
        failed = np.isnan(rec["lambda_mle"]) | np.isnan(rec["logl_H1"])
        lam = np.where(failed, 1.0, rec["lambda_mle"])
        ref = alt.at(lam)
        lam_check(False, rec["lambda_mle"], ref, failed)
        keep = keep_of(ref, failed)
        cmp("logl_H1", rec["logl_H1"], ref["ml"], keep, "logl_H1(ML)")
        logl0 = _NULLS[(n, c, t, grid)]["logl_mle_H0"]
        seen["p_lrt"], lo, hi = _p_check(tag + " p_lrt", "chi", rec["p_lrt"], 2.0 * (rec["logl_H1"] - logl0), df, keep, fails)
        notes.append("p_lrt in [%.3g, %.3g]" % (lo, hi))
    if mode in (3, 4):
        src = rec if mode == 3 else {k: score_out[:, j] for j, k in enumerate(D.FIELDS)}
        ref = alt.score(_NULLS[(n, c, t, grid)]["l_mle_null"], nul)
        keep = keep_of(ref, np.zeros(len(idx), dtype=bool))
        if mode == 3:
            cmp("beta", rec["beta"], ref["beta"], keep, "beta(score)")
            cmp("se", rec["se"], ref["se"], keep, "se(score)")
        b, s = src["beta"].astype(LD), src["se"].astype(LD)
        stat = n * b * b / (df * s * s + b * b)
        seen["p_score"], lo, hi = _p_check(tag + " p_score", "f", rec["p_score"], stat, df, keep, fails)
        notes.append("p_score in [%.3g, %.3g]" % (lo, hi))
    line = "%s %s; %s" % (tag, " ".join("%s %.3g" % kv for kv in seen.items()), "; ".join(notes))
    print(line)
    _record(line)
    assert not fails, "\n".join(fails)
    return seen


def _all_modes(api, oracle, n, c, t, grid="default", switch=None):
    score = _run(api, oracle, n, c, t, 3, grid, switch)
    for mode in (1, 2, 3, 4):
        out = _run(api, oracle, n, c, t, mode, grid, switch)
        _check(oracle, n, c, t, mode, out, grid, switch or "", score_out=score)


# ------------------------------------------------------------------------------------------------ the default table + series path
@pytest.mark.parametrize("t", range(3))
@pytest.mark.parametrize("n,c", D.DEFAULT_SHAPES)
def test_default_path_against_the_definition(gpu_api, oracle, n, c, t):
    """modes 1 to 4 on n below a wavefront (31), at 64, one past (65), 129, 203 and 1031 (table_ksplit = 2), c = 1 to 4 -- the
    FixedC kernels --, heritabilities 0, 0.3 and 0.999"""
    _all_modes(gpu_api, oracle, n, c, t)


def test_default_cases_cover_both_forms_both_ends_and_the_tails(gpu_api, oracle):
    """over the default cases: interior lambda-hats below 1e-3 (the Q form of the series) and above, lambda-hats at l_min and at
    l_max, p-values from above 0.5 to below 1e-150, Wald statistics on both sides of df"""
    low = high = at_min = at_max = below = above = 0
    p_lo, p_hi = 1.0, 0.0
    for n, c in D.DEFAULT_SHAPES:
        for t in range(3):
            out = _run(gpu_api, oracle, n, c, t, 4)
            for j in (2, 3):
                lam = out[:, j]
                inside = (lam > 1e-5) & (lam < 1e5)
                low, high = low + int((inside & (lam < 1e-3)).sum()), high + int((inside & (lam >= 1e-3)).sum())
                at_min, at_max = at_min + int((lam == 1e-5).sum()), at_max + int((lam == 1e5).sum())
            F = (out[:, 0] / out[:, 1]) ** 2
            below, above = below + int((F < n - c - 1).sum()), above + int((F > n - c - 1).sum())
            for j in (4, 5, 6):
                p_lo, p_hi = min(p_lo, float(np.nanmin(out[:, j]))), max(p_hi, float(np.nanmax(out[:, j])))
    print("interior lambda-hat < 1e-3: %d, >= 1e-3: %d, at l_min %d, at l_max %d; F < df %d, F > df %d; p from %.3g to %.3g" % (
        low, high, at_min, at_max, below, above, p_lo, p_hi))
    assert low >= 1 and high >= 100 and at_min >= 10 and at_max >= 10  # one REML lambda-hat of (65, 3), h2 = 0.3, is 5.4e-4
    assert below >= 100 and above >= 20 and 0 < p_lo < 1e-150 and p_hi > 0.5


@pytest.mark.parametrize("mode", [1, 4])
def test_block_lengths(gpu_api, oracle, mode):
    """one setup, blocks of 1, 5, 64 and 257 rows (the 64 SNPs four times and one more): every row against the reference"""
    n, c, t = 65, 3, 1
    blocks = [np.arange(1), np.arange(5, 10), np.arange(64), np.arange(257) % 64]
    out = _run(gpu_api, oracle, n, c, t, mode, blocks=blocks)
    score = _run(gpu_api, oracle, n, c, t, 3)
    s0 = 0
    for idx in blocks:
        _check(oracle, n, c, t, mode, out[s0:s0 + len(idx)], tag="block of %d" % len(idx), idx=idx, score_out=score[idx])
        s0 += len(idx)


# ------------------------------------------------------------------------------------------------ switches, grids, wide kernels
@pytest.mark.parametrize("t", range(3))
@pytest.mark.parametrize("switch", sorted(SWITCHES))
def test_environment_switches(gpu_api, oracle, switch, t):
    """(203, 3) with the series off, the table off, the final pass streaming, and the generic kernel forced"""
    _all_modes(gpu_api, oracle, *D.SWITCH_SHAPE, t, switch=switch)


@pytest.mark.parametrize("t", range(3))
@pytest.mark.parametrize("grid", ["default", "region7", "region16", "shifted"])
def test_grids(gpu_api, oracle, grid, t):
    """(203, 3) on the default grid, with n_region = 7 (intervals wider than 2.31: no series), n_region = 16 and (l_min, l_max) =
    (3e-5, 3e5)"""
    _all_modes(gpu_api, oracle, *D.SWITCH_SHAPE, t, grid=grid)


@pytest.mark.parametrize("t", range(3))
@pytest.mark.parametrize("n,c", D.WIDE_SHAPES)
def test_generic_and_wide_kernels(gpu_api, oracle, n, c, t):
    """c = 6 and 16: the generic multi-pass kernel; c = 18: the wide one"""
    _all_modes(gpu_api, oracle, n, c, t)


# ------------------------------------------------------------------------------------------------ null fits
@pytest.mark.parametrize("n,c", NULL_SHAPES)
def test_null_fits_against_the_definition(gpu_api, oracle, n, c):
    """CalcLambdaNullPanel (with the covariate effects for c <= 16) on the 17 traits of the null-panel cases and CalcLambdaNull on
    three of them: at the device's lambda-hats the log-likelihoods, pve, se(pve), vg, ve, beta and se(beta) within
    dev_bar(lmmdefcases.D_NULL) of the definition -- logl 1.4e-9, se(pve) 3.3e-9, the rest 1e-10 --; both lambda-hats under
    criteria (a)-(c), none left out"""
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    T = len(nc.H2S)
    tr = float(ev.mean())
    Y = np.ascontiguousarray(UtY[:, :T])
    if c <= 16:
        fit, beta, se = gpu_api.CalcLambdaNullPanel(ev, UtW, Y, trace_G=tr, want_beta=True)
    else:
        fit, beta, se = gpu_api.CalcLambdaNullPanel(ev, UtW, Y, trace_G=tr), None, None
    fit8 = np.ascontiguousarray(fit).view(np.float64).reshape(T, 8)
    singles = {t: gpu_api.CalcLambdaNull(ev, UtW, np.ascontiguousarray(Y[:, t]), trace_G=tr) for t in (0, 8, 12)}
    model = D.null_model(oracle, n, c)
    fails = []
    for name, rows, f8, b, s in [("panel", np.arange(T), fit8, beta, se)] + [
            ("single fit of trait %d" % t, np.array([t]), np.array([[v[k] for k in nc.FIELDS]]), None, None) for t, v in singles.items()]:
        sub = D.Model(ev, UtW, Y[:, rows].T)
        assert np.isfinite(f8).all(), name
        dist, ml, reml, n_inside = null_distances(sub, n, c, f8, b, s, tr)
        line = "lmmdef[null n=%d c=%d %s] %s (REML lambda-hat inside on %d of %d)" % (n, c, name, " ".join("%s %.3g" % kv for kv in dist.items()),
                                                                                    n_inside, len(rows))
        for k, v in dist.items():
            if not v <= D.dev_bar(D.D_NULL[k]):
                fails.append("%s: %s %.3g > %.3g" % (name, k, v, D.dev_bar(D.D_NULL[k])))
        for reml_flag, col, logl in ((False, 0, ml), (True, 2, reml)):
            lam_star, _, vals, lams = D.null_maximum(oracle, n, c, reml_flag)
            ok, left, text = D.lambda_criteria(f8[:, col], logl, lam_star[rows], vals[:, rows], lams, 1e-5, 1e5)
            line += "; %s lambda-hat: %s" % ("REML" if reml_flag else "ML", text)
            if left.any() or not ok.all():
                fails.append("%s: %s lambda-hat: %s" % (name, "REML" if reml_flag else "ML", text))
        print(line)
        _record(line)
    assert model.L == T
    assert not fails, "\n".join(fails)

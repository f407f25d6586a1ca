"""The definition-level reference of the univariate LMM (tests/lmmdefcases.py) against a dense GLS, against itself and against the
oracle -- no device.  What is established here is what tests/test_gpu_lmm_definition.py then asks of the device:

* the rotated long-double form equals GLS on the dense H = lambda K + I (Cholesky, long double) up to the orthogonality of U;
* at the oracle's own lambda-hat the oracle's beta, se and log-likelihoods are the reference's: the additive constants of
  LogRL_f / LogL_f, the degrees of freedom and P_ab are read the same way by two derivations.  The per-field maxima over all
  compared pairs are lmmdefcases.D_BETA, D_SE, D_LOGL; 1e3 times them is the device's bar;
* the oracle's lambda-hat meets criteria (a)-(c) of lmmdefcases.lambda_criteria on every case the GPU tests use -- GEMMA reports
  the Newton iterate before the one that met the stopping rule (src/lmm.cpp:2071-2096), so lambda-hat is up to 1e-5 from the
  maximiser and is held to 2e-5, not to 1e-6;
* the oracle's F and chi^2_1 tails against mpmath: P_F_BAR and P_CHI_BAR."""
import numpy as np
import pytest

import lmmdefcases as D
import scorecases as sc

LD = np.longdouble

D_BETA, D_SE, D_LOGL, RATIO_MIN, P_F_BAR, P_CHI_BAR, GRIDS = D.D_BETA, D.D_SE, D.D_LOGL, D.RATIO_MIN, D.P_F_BAR, D.P_CHI_BAR, D.GRIDS
ALL_SHAPES = D.DEFAULT_SHAPES + (D.SWITCH_SHAPE,) + D.WIDE_SHAPES
_WORST = {"beta": 0.0, "se": 0.0, "logl": 0.0}


# ------------------------------------------------------------------------------------------------ 1. dense
@pytest.mark.parametrize("lam", [1e-5, 0.37, 1e5])
def test_rotated_form_equals_dense_gls(oracle, lam):
    """n = 61, c = 2: K' = U diag(eval) U', H = lambda K' + I, W = U UtW, y = U Uty, x = U Utx; GLS through the Cholesky factor of the
    dense H in long double.  beta, se, yPy and both log-likelihoods equal the rotated form's to 1e3 max|U'U - I|, and that is
    below 1e-13: the orthogonality of U is the only source of difference."""
    d = D.case(oracle, 61, 2)
    n, c, l = 61, 2, 8
    U, ev = d["U"].astype(LD), d["ev"].astype(LD)
    orth = float(np.abs(U.T @ U - np.eye(n, dtype=LD)).max())
    assert orth < 1e-13
    tol = 1e3 * orth
    W, y = U @ d["UtW"].astype(LD), U @ d["UtY"][:, 1].astype(LD)
    X = d["UtX"][-l:].astype(LD) @ U.T  # the last rows: random SNPs and the uncentred one
    H = LD(lam) * (U * ev) @ U.T + np.eye(n, dtype=LD)
    F, logdet_H = D._chol(H[None])
    rot = D.Model(d["ev"], d["UtW"], d["UtY"][:, 1], d["UtX"][-l:]).at(lam)
    worst = {}
    for s in range(l):
        V = np.column_stack([W, X[s]])
        HiV = D._chol_solve(F, V[None])[0]
        Hiy = D._chol_solve(F, y[:, None][None])[0][:, 0]
        A, b = V.T @ HiV, V.T @ Hiy
        FA, logdet_A = D._chol(A[None])
        sol = D._chol_solve(FA, np.column_stack([b, np.eye(c + 1, dtype=LD)[:, c]])[None])[0]
        beta, axx = sol[:, 0], sol[c, 1]
        yPy = y @ Hiy - b @ beta
        df = n - c - 1
        _, logdet_VV = D._chol((V.T @ V)[None])
        reml = LD(df) / 2 * (np.log(LD(df)) - D.LOG2PI - 1) - logdet_H[0] / 2 - (logdet_A[0] - logdet_VV[0]) / 2 - LD(df) / 2 * np.log(yPy)
        ml = LD(n) / 2 * (np.log(LD(n)) - D.LOG2PI - 1) - logdet_H[0] / 2 - LD(n) / 2 * np.log(yPy)
        dense = {"beta": beta[c], "se": np.sqrt(axx * yPy / df), "yPy": yPy, "reml": reml, "ml": ml}
        for k, v in dense.items():
            e = float(abs(rot[k][s] - v) / abs(v))
            worst[k] = max(worst.get(k, 0.0), e)
    print("lambda %g: max|U'U - I| = %.3g, worst relative differences %s" % (lam, orth, worst))
    assert max(worst.values()) <= tol, (worst, tol)


def test_score_form_equals_the_closed_form_of_the_score_panel(oracle):
    """the score test's beta and se by this module's elimination against scorecases.closed_form (a Cholesky projection written
    for the score panel): two long-double derivations, equal to 1e-15 relative after rounding to double"""
    d = D.case(oracle, 203, 3)
    lams = [1e-5, 0.8, 1e5]
    rec, ratio = sc.closed_form(oracle, d["ev"], d["UtW"], d["UtY"], lams, d["UtX"])
    for t in range(3):
        alt, nul = D.models(oracle, 203, 3, t)
        r = alt.score(lams[t], nul)
        keep = ratio[t] >= RATIO_MIN
        assert keep.sum() >= 63
        for k in ("beta", "se"):
            assert D.rel(rec[k][t], r[k])[keep].max() <= 4 * np.finfo(np.float64).eps, (t, k)
        assert np.abs(ratio[t] - r["ratio"].astype(np.float64))[keep].max() <= 1e-14


# ------------------------------------------------------------------------------------------------ 2., 3. the oracle
def _oracle_runs(oracle, n, c, t, grid):
    d = D.case(oracle, n, c)
    y = np.ascontiguousarray(d["UtY"][:, t])
    l_mle, logl0 = oracle.calc_lambda_null("L", d["ev"], d["UtW"], y, **grid)
    kw = dict(l_mle_null=l_mle, logl_mle_H0=logl0, **grid)
    return l_mle, [oracle.lmm_batch_UtX(m, d["ev"], d["UtW"], y, d["UtX"], **kw) for m in (1, 2, 3)]


@pytest.mark.parametrize("t", range(3))
@pytest.mark.parametrize("n,c,grid", [(n, c, "default") for n, c in ALL_SHAPES] + [D.SWITCH_SHAPE + (g,) for g in GRIDS if g != "default"])
def test_oracle_is_the_reference_at_its_own_lambda_and_meets_the_lambda_criteria(oracle, n, c, grid, t):
    g = GRIDS[grid]
    l_mle, (r1, r2, r3) = _oracle_runs(oracle, n, c, t, g)
    alt, nul = D.models(oracle, n, c, t)
    l = alt.L
    evals = {"wald": (r1, alt.at(r1["lambda_remle"]), "reml"), "ml": (r2, alt.at(r2["lambda_mle"]), "ml"), "score": (r3, alt.score(l_mle, nul), None)}
    # the leave-out share of the comparison, on the reference alone
    for reml in (True, False):
        lam_star = D.maximum(oracle, n, c, t, reml, **g)[0]
        low = alt.at(lam_star)["ratio"] < RATIO_MIN
        assert low.mean() <= D.LEFT_OUT_MAX, (reml, int(low.sum()))
    assert (evals["score"][1]["ratio"] < RATIO_MIN).mean() <= D.LEFT_OUT_MAX
    # fixed-lambda identity
    seen = {"beta": 0.0, "se": 0.0, "logl": 0.0}
    for name, (rec, ref, logl_key) in evals.items():
        keep = (ref["ratio"] >= RATIO_MIN) & ~np.isnan(rec["logl_H1"])
        assert keep.mean() >= 1 - D.LEFT_OUT_MAX, name
        if name != "ml":
            seen["beta"] = max(seen["beta"], D.rel(rec["beta"], ref["beta"])[keep].max())
            seen["se"] = max(seen["se"], D.rel(rec["se"], ref["se"])[keep].max())
        if logl_key:
            seen["logl"] = max(seen["logl"], D.rel(rec["logl_H1"], ref[logl_key])[keep].max())
    for k in seen:
        _WORST[k] = max(_WORST[k], float(seen[k]))
    print("n=%d c=%d grid=%s trait %d: oracle against the reference at the oracle's lambda-hat: %s; maxima so far: %s" % (
        n, c, grid, t, " ".join("%s %.3g" % kv for kv in seen.items()), " ".join("%s %.3g" % kv for kv in _WORST.items())))
    assert seen["beta"] <= 2 * D_BETA and seen["se"] <= 2 * D_SE and seen["logl"] <= 2 * D_LOGL, seen
    # lambda-hat
    for reml, rec, key, ref in ((True, r1, "lambda_remle", evals["wald"][1]), (False, r2, "lambda_mle", evals["ml"][1])):
        lam_star, _, vals, lams = D.maximum(oracle, n, c, t, reml, **g)
        ok, left, text = D.lambda_criteria(rec[key], ref["reml" if reml else "ml"], lam_star, vals, lams, g["l_min"], g["l_max"])
        print("    %s lambda-hat: %s" % ("REML" if reml else "ML", text))
        assert left.mean() <= D.LEFT_OUT_MAX, text
        assert ok.all(), (text, np.flatnonzero(~ok))
    assert l == D.n_snps(n, c)


def test_lambda_criteria_reject_a_wrong_lambda(oracle):
    """what the criteria catch, on (203, 3), h2 = 0.3, REML: an interior lambda-hat moved by 1e-4 fails (a) on every SNP and by 3e-5 on
    every SNP too; one put at l_min or l_max although the maximum is inside fails (b) and (c); the oracle's own values pass"""
    n, c, t = D.SWITCH_SHAPE + (1,)
    d = D.case(oracle, n, c)
    rec = oracle.lmm_batch_UtX(1, d["ev"], d["UtW"], np.ascontiguousarray(d["UtY"][:, t]), d["UtX"])
    alt = D.models(oracle, n, c, t)[0]
    lam_star, _, vals, lams = D.maximum(oracle, n, c, t, True)
    lam = rec["lambda_remle"].copy()
    inside = (lam > 1e-5) & (lam < 1e5)
    assert inside.sum() >= 60

    def verdict(lam_hat):
        return D.lambda_criteria(lam_hat, alt.at(lam_hat)["reml"], lam_star, vals, lams, 1e-5, 1e5)[0]

    assert verdict(lam).all()
    for eps in (1e-4, -1e-4, 3e-5, -3e-5):
        assert not verdict(np.where(inside, lam * (1 + eps), lam))[inside].any(), eps
    for end in (1e-5, 1e5):
        assert not verdict(np.where(inside, end, lam))[inside].any(), end


NULL_SHAPES = ((203, 1), (203, 3), (1031, 6), (203, 18))


def null_distances(model, n, c, fit8, beta, se, trace_G):
    """per field: max relative distance of a null fit (rows of l_mle, logl_mle, l_remle, logl_remle, pve, pve_se, vg, ve; the
    covariates' beta and se or None; vg, ve all NaN: not compared) from the definition at the fit's own lambda-hats; se(pve) where the REML one is inside the grid"""
    fit8 = np.asarray(fit8, dtype=np.float64)
    rm, rr = model.at(fit8[:, 0]), model.at(fit8[:, 2])
    nf = model.null_fit(fit8[:, 2], trace_G)
    inside = (fit8[:, 2] > 1e-5) & (fit8[:, 2] < 1e5)
    d = {"logl": max(D.rel(fit8[:, 1], rm["ml"]).max(), D.rel(fit8[:, 3], rr["reml"]).max()), "pve": D.rel(fit8[:, 4], nf["pve"]).max()}
    if inside.any():
        d["pve_se"] = D.rel(fit8[:, 5], nf["pve_se"])[inside].max()
    if not np.isnan(fit8[:, 6:8]).all():
        d["vg"], d["ve"] = D.rel(fit8[:, 6], nf["vg"]).max(), D.rel(fit8[:, 7], nf["ve"]).max()
    if beta is not None:
        d["beta"] = float((np.abs(beta - nf["beta"]) / np.maximum(np.abs(nf["beta"]), nf["se"])).max())
        d["se"] = D.rel(se, nf["se"]).max()
    return {k: float(v) for k, v in d.items()}, rm["ml"], rr["reml"], int(inside.sum())


@pytest.mark.parametrize("n,c", NULL_SHAPES)
def test_oracle_null_fits_are_the_definition_at_their_own_lambda(oracle, n, c):
    """CalcLambda('L' / 'R'), CalcPve and CalcLmmVgVeBeta of the oracle on the 17 traits of the null-panel cases: the log-likelihoods,
    pve, se(pve) through the dense projection's second derivative, vg, ve and the covariate effects within twice
    lmmdefcases.D_NULL; both lambda-hats meet criteria (a)-(c)"""
    import nullpanelcases as nc
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    T = len(nc.H2S)
    fits = nc.oracle_fits(oracle, n, c)[:T]
    tr = float(ev.mean())
    fit8 = np.zeros((T, 8))
    fit8[:, :4] = fits
    beta = se = None
    if c <= 16:
        beta, se = np.zeros((T, c)), np.zeros((T, c))
    for t in range(T):
        y = np.ascontiguousarray(UtY[:, t])
        fit8[t, 4:6] = oracle.calc_pve(ev, UtW, y, fits[t, 2], tr)
        if c <= 16:
            fit8[t, 6], fit8[t, 7], beta[t], se[t] = oracle.calc_vg_ve_beta(ev, UtW, y, fits[t, 2])
    model = D.null_model(oracle, n, c)
    if c > 16:  # the oracle's CalcLmmVgVeBeta holds 16 covariates: no vg, ve, beta from it
        fit8[:, 6:8] = np.nan
    d, ml, reml, n_inside = null_distances(model, n, c, fit8, beta, se, tr)
    print("n=%d c=%d: oracle's null fits against the definition: %s (REML lambda-hat inside on %d of %d)" % (
        n, c, " ".join("%s %.3g" % kv for kv in d.items()), n_inside, T))
    assert n_inside >= 8
    for k, v in d.items():
        assert v <= 2 * D.D_NULL[k], (k, v)
    for reml_flag, col, logl in ((False, 0, ml), (True, 2, reml)):
        lam_star, _, vals, lams = D.null_maximum(oracle, n, c, reml_flag)
        ok, left, text = D.lambda_criteria(fits[:, col], logl, lam_star, vals, lams, 1e-5, 1e5)
        print("    %s lambda-hat: %s" % ("REML" if reml_flag else "ML", text))
        assert not left.any() and ok.all(), text


# ------------------------------------------------------------------------------------------------ 4. tails
def test_oracle_tails_against_mpmath(oracle):
    """gsl_cdf_fdist_Q(x; 1, df) and gsl_cdf_chisq_Q(x; 1) as the oracle restates them, df in {28, 57, 199, 1027}, x from 1e-8 to 1e4
    on both sides of x = df, p down to 6e-300"""
    xs = np.concatenate([np.logspace(-8, 4, 73), [27.9, 28.1, 56.5, 57.5, 198.0, 200.0, 1026.0, 1028.0]])
    worst_f = worst_c = 0.0
    n_f = n_c = 0
    p_min = 1.0
    for df in (28, 57, 199, 1027):
        for x in xs:
            want = D.p_f(x, df)
            if want < 6e-300:
                continue
            worst_f = max(worst_f, D.p_rel(oracle.fdist_Q(float(x), 1.0, float(df)), want))
            p_min = min(p_min, float(want))
            n_f += 1
    for x in np.concatenate([xs, np.linspace(100, 1370, 40)]):
        want = D.p_chi1(x)
        if want < 6e-300:
            continue
        worst_c = max(worst_c, D.p_rel(oracle.chisq_Q1(float(x)), want))
        p_min = min(p_min, float(want))
        n_c += 1
    print("F tail: %d points, worst %.3g; chi^2_1 tail: %d points, worst %.3g; smallest p %.3g" % (n_f, worst_f, n_c, worst_c, p_min))
    assert n_f > 250 and n_c > 80 and p_min < 1e-290
    assert worst_f <= P_F_BAR and worst_c <= P_CHI_BAR
    assert oracle.chisq_Q1(0.0) == 1.0 and oracle.chisq_Q1(-1e-9) == 1.0

"""-vc 1 / -vc 2 on the MI355X: the SPD inverse against numpy, Haseman-Elston against the reference's printed numbers
(tests/golden/text/V*.log.json) and the numpy restatement, REML against the reference's REML null (P4.log.json), GEMMA's own
stop rule and the numpy formulas at the returned sigma2."""
import numpy as np
import pytest

from vccases import HE_CASES, HE_KEYS, fixture, he, p_inputs, reml_dev, reml_log_dev, reml_summary

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def api():
    from gemma_amd import api as A
    A.init(0)
    return A


def spd(n, cond, seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.geomspace(1.0, cond, n)
    return (Q * ev) @ Q.T, ev


@pytest.mark.parametrize("n", [1, 63, 128, 257, 1000, 4097])
def test_spd_inverse_matches_numpy(api, n):
    A, ev = spd(n, 1e4, n)
    Ai, logdet = api.spd_inverse(A, return_logdet=True)
    ref = np.linalg.inv(A)
    kappa = ev[-1] / ev[0]
    err = np.abs(Ai - ref).max() / np.abs(ref).max()
    assert err < 50 * n * np.finfo(float).eps * kappa, err
    assert np.array_equal(Ai, Ai.T)
    assert abs(logdet - np.log(ev).sum()) < 1e-9 * max(1.0, abs(np.log(ev).sum()))
    assert np.abs(A @ Ai - np.eye(n)).max() < 50 * n * np.finfo(float).eps * kappa


def test_spd_inverse_not_pd_then_recovers(api):
    from gemma_amd import _lib as L
    A, _ = spd(300, 10.0, 3)
    A[200, 200] = -5.0
    with pytest.raises(L.GemmaHipError) as e:
        api.spd_inverse(A)
    assert e.value.code == L.ENOTPD and e.value.bad_pivot == 200  # leading minors up to 199 are those of an SPD matrix
    B, _ = spd(300, 10.0, 4)
    assert np.abs(api.spd_inverse(B) @ B - np.eye(300)).max() < 1e-10


@pytest.mark.parametrize("tag,inputs", HE_CASES, ids=[c[0] for c in HE_CASES])
def test_he_matches_reference_and_numpy(api, tag, inputs):
    """-k and -mk (two and three kinships, with and without -c, P and BXD; negative components included)"""
    Ks, W, y = inputs()
    got = api.VC().CalcVChe(Ks, W, y)
    ref = he(Ks, W, y)
    fx = fixture(tag)
    for key, fk in HE_KEYS:
        g = np.atleast_1d(getattr(got, "v_" + key) if hasattr(got, "v_" + key) else getattr(got, key))
        if fk in fx:
            assert np.allclose(g, np.array(fx[fk], dtype=float), rtol=5e-6, atol=0), (key, g, fx[fk])
        assert np.allclose(g, np.atleast_1d(ref[key]), rtol=1e-10, atol=0), (key, g)


def split_kinships(nvc, n=800, snps=400, seed=5):
    """nvc kinships from disjoint random SNP sets (CenterMatrix(G)-centred), a phenotype with a share of variance on each
    (pve 0.6 in all; every component away from the boundary) and an intercept plus one covariate"""
    from oracle import oracle as O
    import vccases as V
    rng = np.random.default_rng(seed)
    Ks, y = [], np.zeros(n)
    for _ in range(nvc):
        G = rng.integers(0, 3, size=(snps, n)).astype(float)
        Ks.append(V.center_matrix(O.calc_kin(G, 1)))
        y += (G - G.mean(1, keepdims=True)).T @ rng.standard_normal(snps) * np.sqrt(0.6 / nvc / snps / 0.5)
    W = np.column_stack([np.ones(n), rng.standard_normal(n)])
    y += rng.standard_normal(n) * np.sqrt(0.4) + W @ np.array([3.0, 0.5])
    return Ks, W, y


def test_he_multi_kinship_matches_numpy(api):
    Ks, W, y = split_kinships(3)
    got = api.VC().CalcVChe(Ks, W, y)
    ref = he(Ks, W, y)
    for key in ("sigma2", "se_sigma2", "pve", "se_pve"):
        assert np.allclose(getattr(got, "v_" + key), ref[key], rtol=1e-10, atol=1e-12), key
    assert abs(got.pve_total - ref["pve_total"]) < 1e-10


def test_reml_one_kinship_lands_on_reference_null(api):
    K, W, y, *_ = p_inputs(False)
    got = api.VC().CalcVCreml([K], W, y)
    fx = fixture("P4")
    assert got.status == 0
    assert abs(got.v_sigma2[0] / float(fx["vg estimate in the null model"]) - 1) < 1e-3
    assert abs(got.v_sigma2[1] / float(fx["ve estimate in the null model"]) - 1) < 1e-3
    assert abs(got.v_pve[0] / float(fx["pve estimate in the null model"]) - 1) < 1e-3


def check_reml(got, Ks, W, y, noconstrain=False, optimum=True):
    """GEMMA's stop rule at the returned sigma2, the numpy formulas there, and (optimum) the distance to a tightly converged
    numpy root within twice the Newton step the AI matrix gives at the returned point"""
    from scipy.optimize import root
    s2 = np.asarray(got.v_sigma2)
    assert got.status == 0 and got.iterations <= 100
    x = s2 if noconstrain else np.log(s2)
    dev = (lambda z: reml_dev(z, Ks, W, y)) if noconstrain else (lambda z: reml_log_dev(z, Ks, W, y))
    d1, d2 = dev(x)
    assert np.abs(d1).sum() < 1e-3, d1
    ref = reml_summary(s2, Ks, W, y, noconstrain=noconstrain)
    for key in ("se_sigma2", "pve", "se_pve", "pve_total", "se_pve_total"):
        g = np.atleast_1d(getattr(got, "v_" + key) if hasattr(got, "v_" + key) else getattr(got, key))
        r = np.atleast_1d(ref[key])
        # a component at the boundary (sigma2 -> 0 on the log scale) has no finite standard error on either side
        assert np.array_equal(np.isfinite(g), np.isfinite(r)), (key, g, r)
        fin = np.isfinite(r)
        assert np.allclose(g[fin], r[fin], rtol=1e-8, atol=1e-12), (key, g, r)
    assert got.evaluations == got.inverses and got.evaluations >= got.iterations
    if optimum:
        sol = root(lambda z: dev(z)[0], x, jac=lambda z: dev(z)[1], method="hybr", options={"xtol": 1e-13})
        step = np.linalg.solve(d2, d1)
        assert np.linalg.norm(x - sol.x) <= 2 * np.linalg.norm(step) + 1e-9, (x, sol.x, step)


@pytest.mark.parametrize("nvc", [1, 2, 3])
def test_reml_stop_rule_formulas_and_optimum(api, nvc):
    if nvc == 1:
        K, W, y, *_ = p_inputs(False)
        Ks = [K]
    else:
        Ks, W, y = split_kinships(nvc)
    got = api.VC().CalcVCreml(Ks, W, y)
    check_reml(got, Ks, W, y)
    h = he(Ks, W, y)["sigma2"]  # iteration 0 is the HE start, log(0.1) for components <= 0
    assert np.allclose(got.iter_sigma2[0], np.where(h > 0, h, 0.1), rtol=1e-10)


def test_reml_negative_he_start(api):
    """-mk of P's two SNP halves with -c: the HE fit has a negative component (the issue's yardstick), REML starts it at 0.1"""
    from vccases import p_mk
    Ks, W, y = p_mk([(0, 400), (400, 800)], True)
    got = api.VC().CalcVCreml(Ks, W, y)
    assert got.iter_sigma2[0][1] == pytest.approx(0.1, rel=1e-14)
    check_reml(got, Ks, W, y, optimum=False)


def test_reml_noconstrain(api):
    Ks, W, y = split_kinships(2)
    got = api.VC().CalcVCreml(Ks, W, y, noconstrain=True)
    check_reml(got, Ks, W, y, noconstrain=True)
    con = api.VC().CalcVCreml(Ks, W, y)
    assert np.allclose(got.v_sigma2, con.v_sigma2, rtol=1e-2)


def test_reml_bit_identical(api):
    Ks, W, y = split_kinships(2)
    a = api.VC().CalcVCreml(Ks, W, y)
    b = api.VC().CalcVCreml(Ks, W, y)
    assert np.array_equal(a.v_sigma2, b.v_sigma2) and np.array_equal(a.v_se_pve, b.v_se_pve)


def random_kinships(api, n, nvc, snps, seed):
    """nvc kinships of disjoint random SNP sets on the device path (CalcKin + CenterMatrix) and a phenotype with pve 0.5"""
    rng = np.random.default_rng(seed)
    Ks, y = [], np.zeros(n)
    for _ in range(nvc):
        G = rng.integers(0, 3, size=(snps, n)).astype(np.float64)
        Ks.append(api.CenterMatrix(api.CalcKin(G, 0, n, 1)))
        y += (G - G.mean(1, keepdims=True)).T @ rng.standard_normal(snps) * np.sqrt(0.5 / nvc / snps / 0.5)
    y += rng.standard_normal(n) * np.sqrt(0.5)
    return Ks, np.ones((n, 1)), y


def test_spd_inverse_at_20000(api):
    """n = 20 000 (157 diagonal blocks, the recursive inverse and product at full depth): A = X X^T / k + lam I, whose condition
    number the Marchenko-Pastur edge bounds; ||A A^-1 - I||_max within n eps kappa"""
    import torch
    n, k, lam = 20000, 5000, 1e-3
    g = torch.Generator(device="cuda").manual_seed(20000)
    X = torch.randn(n, k, device="cuda", dtype=torch.float64, generator=g)
    A = X @ X.T / k + lam * torch.eye(n, device="cuda", dtype=torch.float64)
    del X
    kappa = (lam + 1.1 * (1 + np.sqrt(n / k)) ** 2) / lam
    Ai = A.clone()
    _, logdet = api.spd_inverse(Ai, return_logdet=True)
    R = A @ Ai
    R.diagonal().sub_(1.0)
    err = R.abs().max().item()
    assert err < n * np.finfo(float).eps * kappa, (err, n * np.finfo(float).eps * kappa)
    assert torch.equal(Ai, Ai.T)
    # log det between the bounds of the spectrum: lam <= eigenvalue <= lam kappa
    assert n * np.log(lam) < logdet < n * np.log(lam * kappa)


def test_he_at_20000_three_kinships(api):
    n = 20000
    Ks, W, y = random_kinships(api, n, 3, 1500, 21)
    got = api.VC().CalcVChe(Ks, W, y)
    ref = he(Ks, W, y)
    for key in ("sigma2", "se_sigma2", "pve", "se_pve"):
        assert np.allclose(getattr(got, "v_" + key), ref[key], rtol=1e-10, atol=1e-14), key


def test_reml_at_8192_three_kinships(api):
    Ks, W, y = random_kinships(api, 8192, 3, 1500, 82)
    got = api.VC().CalcVCreml(Ks, W, y)
    check_reml(got, Ks, W, y, optimum=False)


def test_reml_at_20000_matches_lambda_null_and_is_bit_identical(api):
    """n = 20 000, one kinship: the AI-REML pve against the eigendecomposition-based REML null (CalcLambdaNull, a different
    algorithm on the same likelihood); a second fit bit-identical to the first"""
    import torch
    n = 20000
    Ks, W, y = random_kinships(api, n, 1, 3000, 2020)
    Kd = [torch.from_numpy(Ks[0]).cuda()]
    a = api.VC().CalcVCreml(Kd, W, y)
    b = api.VC().CalcVCreml(Kd, W, y)
    assert np.array_equal(a.v_sigma2, b.v_sigma2) and np.array_equal(a.v_se_sigma2, b.v_se_sigma2) and a.status == 0
    assert np.array_equal(a.iter_sigma2, b.iter_sigma2)
    del Kd
    U = np.empty_like(Ks[0])
    ev = np.empty(n)
    trace_G = api.EigenDecomp_Zeroed(Ks[0].copy(), U, ev)
    null = api.CalcLambdaNull(ev, U.T @ W, U.T @ y, trace_G=trace_G)
    assert abs(a.v_pve[0] - null["pve"]) < 1e-4, (a.v_pve[0], null["pve"])

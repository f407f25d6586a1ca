"""-vc 1 / -vc 2 on the MI355X: the SPD inverse against numpy, exact inverses and a refined high-precision reference, at block
edges, with failing pivots and through every device entry path; Haseman-Elston against the reference's printed numbers
(tests/golden/text/V*.log.json) and the numpy restatement; REML against the reference's own run (recorded in
tests/golden/ref_calls/, printed in tests/golden/text/V*r.log.json), the REML null (P4.log.json), GEMMA's own stop rule and the
numpy formulas at the returned sigma2; the fit at up to 8 kinships and 64 covariates, on padded device kinships, and the calls
the ABI rejects."""
import numpy as np
import pytest

from vccases import (HE_CASES, HE_KEYS, REML_CASES, REML_DIES, fixture, he, inputs, p_inputs, ref_reml, reml_dev, reml_log_dev,
                     reml_summary, SPD_C, spd_spectrum)

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



# ----------------------------------------------------------------------------- REML against the reference's own run
@pytest.fixture(scope="module")
def hybrid_lib(tmp_path_factory):
    from vccases import hybrid_drive_lib
    return hybrid_drive_lib(tmp_path_factory.mktemp("hybrid_drive"))


@pytest.mark.parametrize("tag,itag,noconstrain", REML_CASES, ids=[c[0] for c in REML_CASES])
def test_reml_matches_reference_run(api, hybrid_lib, tag, itag, noconstrain):
    """CalcVCreml against the reference's VC::CalcVCreml (oracle/ref_bridge.cpp ref_vc_reml, replayed from
    tests/golden/ref_calls/test_reference_vc_reml_<tag>.npz) and its binary's printout (tests/golden/text/<tag>.log.json).
    The recorded run's multiroot solver is oracle/gslshim's adaptor over include/gemma_vc_hybrid.hpp, the solver the device
    fit drives: what this pins is the device's H^-1, P, dev1, AI matrix and se / pve algebra on the reference's own, iterate
    by iterate.  Same status and iteration count; every iterate and every field within 5e-12 relative (measured spread:
    1e-14 on V1r / V1cr, 5e-14 on VB1r (56 iterations), 2e-13 on V1nr, 5e-13 on VB2r (38 iterations)); the printed digits
    within 5e-6.
    V2cr / V3r: the reference's run dies on its first trial point (every sigma2 -> 0 or infinity: H singular in LUInvert).
    The device takes that point as a failed step (HybridSJ::EVAL_OUTSIDE) and goes on; the numpy LogRL_dev12 driven the same
    way (vccases.numpy_reml with outside) must then give the same status, iteration count, iterates and fields: V2cr
    converges after 8 iterations on both.  V3r does not converge: a component runs to 0 and both stop with GSL_ENOPROG, after
    38 iterations on the device and 33 in numpy (the flat likelihood there turns rounding into trip count); only the status
    is compared."""
    from refcases import Calls
    Ks, W, y = inputs(itag)
    ref = ref_reml(Calls("test_reference_vc_reml[%s]" % tag, None, None).ref, Ks, W, y, noconstrain)
    got = api.VC().CalcVCreml(Ks, W, y, noconstrain=noconstrain)
    fx = fixture(tag)
    printed = np.array(fx["iterations"], dtype=float)
    assert np.allclose(got.iter_sigma2[0], ref["iter_sigma2"][0], rtol=1e-10, atol=0)
    assert np.allclose(got.iter_sigma2[:len(printed)], printed, rtol=5e-6, atol=0)
    keys = ("sigma2", "se_sigma2", "pve", "se_pve", "pve_total", "se_pve_total")
    if tag in REML_DIES:
        assert ref["status"] == -1 and ref["iterations"] == 0
        from vccases import numpy_reml
        ref = numpy_reml(hybrid_lib, Ks, W, y, noconstrain, outside=True)
        if tag == "V3r":  # the walk of a component to 0 (4e-160) flips the trip count between inverses: 33 numpy, 38 device
            assert got.status == ref["status"] == 2
            return
        tol = 1e-8  # numpy's LU inverse against the device's Cholesky, not the reference's LU
    else:
        assert ref["status"] == 0 and ref["iterations"] == len(printed) - 1
        tol = 5e-12
        for key, fk in (("sigma2", "sigma2 estimates"), ("se_sigma2", "se(sigma2)"), ("pve", "pve estimates"), ("se_pve", "se(pve)")):
            assert np.allclose(getattr(got, "v_" + key), np.array(fx[fk], dtype=float), rtol=5e-6, atol=0), (key, fx[fk])
    assert (got.status, got.iterations) == (ref["status"], ref["iterations"])
    assert np.allclose(got.iter_sigma2, ref["iter_sigma2"], rtol=tol, atol=0), np.abs(got.iter_sigma2 / ref["iter_sigma2"] - 1).max()
    for key in keys:
        g = np.atleast_1d(getattr(got, "v_" + key) if hasattr(got, "v_" + key) else getattr(got, key))
        r = np.atleast_1d(ref[key])
        assert np.array_equal(np.isfinite(g), np.isfinite(r)), (key, g, r)
        assert np.allclose(g[np.isfinite(r)], r[np.isfinite(r)], rtol=tol, atol=0), (key, g, r)


# ----------------------------------------------------------------------------- the SPD inverse against exact references
EPS = np.finfo(float).eps  # every forward-error bound below: ||X - A^-1||_max <= SPD_C n eps kappa ||A^-1||_max (vccases)


def tridiag(n, s=1.0):
    """s T, T = tridiag(-1, 2, -1): T^-1_ij = min(i,j) (n + 1 - max(i,j)) / (n + 1) (1-based), log det T = log(n + 1),
    kappa = (1 + cos(pi / (n + 1))) / (1 - cos(pi / (n + 1))) ~ 4 (n + 1)^2 / pi^2"""
    A = np.zeros((n, n))
    i = np.arange(n)
    A[i, i] = 2.0 * s
    A[i[:-1], i[:-1] + 1] = A[i[:-1] + 1, i[:-1]] = -1.0 * s
    c = np.cos(np.pi / (n + 1))
    return A, (1 + c) / (1 - c)


def tridiag_inverse(n):
    i = np.arange(1, n + 1, dtype=np.float64)
    return np.minimum.outer(i, i) * (n + 1 - np.maximum.outer(i, i)) / (n + 1)


def fwd_err(X, R):
    return np.abs(X - R).max() / np.abs(R).max()


@pytest.mark.parametrize("n", [127, 128, 129, 255, 256, 257, 383, 384, 385, 1151, 1153, 4097])
def test_spd_inverse_tridiagonal_exact(api, n):
    """sizes on each side of the 128-row block and of the recursive splits of spd_trtri_rec / spd_lauum_rec (measured: at
    most 2.6 % of the bound, at n = 127)"""
    A, kappa = tridiag(n)
    X, ld = api.spd_inverse(A, return_logdet=True)
    err = fwd_err(X, tridiag_inverse(n))
    assert err <= SPD_C * n * EPS * kappa, (err, SPD_C * n * EPS * kappa)
    assert np.array_equal(X, X.T)
    assert abs(ld - np.log(n + 1)) <= 64 * n * EPS, (ld, np.log(n + 1))


@pytest.mark.parametrize("n", [129, 385])
@pytest.mark.parametrize("s", [1e-150, 1e150])
def test_spd_inverse_tridiagonal_scaled(api, n, s):
    """s T at the ends of the exponent range: (s T)^-1 = T^-1 / s, log det shifts by exactly n log s"""
    A, kappa = tridiag(n, s)
    X, ld = api.spd_inverse(A, return_logdet=True)
    err = fwd_err(X * s, tridiag_inverse(n))
    assert err <= SPD_C * n * EPS * kappa, err
    want = np.log(n + 1) + n * np.log(s)
    assert abs(ld - want) <= 64 * n * EPS * (abs(np.log(s)) + 1), (ld, want)


def test_spd_inverse_tridiagonal_20000(api):
    """n = 20 000 (157 diagonal blocks; kappa ~ 1.6e8) on the device path, the exact inverse formed on the device"""
    import torch
    n = 20000
    c = np.cos(np.pi / (n + 1))
    kappa = (1 + c) / (1 - c)
    At = torch.zeros(n, n, device="cuda", dtype=torch.float64)
    At.diagonal().fill_(2.0)
    At.diagonal(1).fill_(-1.0)
    At.diagonal(-1).fill_(-1.0)
    _, ld = api.spd_inverse(At, return_logdet=True)
    i = torch.arange(1, n + 1, device="cuda", dtype=torch.float64)
    R = torch.minimum(i[:, None], i[None, :]) * (n + 1 - torch.maximum(i[:, None], i[None, :])) / (n + 1)
    err = ((At - R).abs().max() / R.abs().max()).item()
    del R
    assert err <= SPD_C * n * EPS * kappa, (err, SPD_C * n * EPS * kappa)
    assert torch.equal(At, At.T)
    assert abs(ld - np.log(n + 1)) <= 64 * n * EPS


@pytest.mark.parametrize("n", [127, 129, 256, 257, 385])
@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10])
def test_spd_inverse_prescribed_spectrum(api, n, kappa):
    """random SPD with a prescribed spectrum (vccases.spd_spectrum: the reference inverse refined in long double; both parts
    of its error, measured in tests/test_vc_cpu.py at n = 257 and 385, sit >= 100x below the bound): forward error within SPD_C n eps kappa (measured: at most 9.5 %
    of the bound, at kappa = 1e2), the inverse symmetric to the bit, log det within that bound (plus n eps |log det| for the
    sum) of the float64 LU's.  The sizes stop at 385 (three blocks and a 1-row block) because the long-double product costs
    n^3 on the host; the block edges near 1 152 are the tridiagonal family's."""
    A, R = spd_spectrum(n, kappa, n)
    X, ld = api.spd_inverse(A, return_logdet=True)
    err = fwd_err(X, R)
    assert err <= SPD_C * n * EPS * kappa, (err, SPD_C * n * EPS * kappa)
    assert np.array_equal(X, X.T)
    sign, want = np.linalg.slogdet(A)
    # the bound's share of the perturbation tr(A^-1 dA), plus the rounding of a sum of n logarithms
    assert sign == 1 and abs(ld - want) <= SPD_C * n * EPS * kappa + n * EPS * abs(want), (ld, want)


def _spd_fails(api, A):
    from gemma_amd import _lib as L
    with pytest.raises(L.GemmaHipError) as e:
        api.spd_inverse(A)
    assert e.value.code == L.ENOTPD, e.value.code
    return e.value.bad_pivot


def _spd_recovers(api):
    A, kappa = tridiag(300)
    assert fwd_err(api.spd_inverse(A), tridiag_inverse(300)) <= SPD_C * 300 * EPS * kappa


@pytest.mark.parametrize("row", [0, 127, 128, 129, 255, 256, 299])
def test_spd_inverse_negative_pivot_row(api, row):
    """a negative diagonal entry at row r of an otherwise SPD matrix: the leading minors up to r - 1 are SPD, so the first
    pivot that is not > 0 is r, in every diagonal block and at its edges"""
    A, _ = spd(300, 10.0, 11)
    A[row, row] = -0.5
    assert _spd_fails(api, A) == row
    _spd_recovers(api)


def test_spd_inverse_indefinite_minor_across_blocks(api):
    """every diagonal entry positive, the 2 x 2 minor of rows 127 / 128 indefinite: pivot 127 (last row of block 0) is
    positive, pivot 128 (first row of block 1) turns negative only through the trailing update"""
    B, _ = spd(300, 10.0, 12)
    A = np.eye(300) + 0.01 * B
    A[127, 128] = A[128, 127] = 2.0
    assert np.all(np.diag(A) > 0)
    assert _spd_fails(api, A) == 128
    _spd_recovers(api)


@pytest.mark.parametrize("i,j,v", [(5, 100, np.nan), (5, 200, np.nan), (130, 131, np.inf), (0, 299, -np.inf)])
def test_spd_inverse_nonfinite_upper(api, i, j, v):
    """NaN / Inf in the strict upper triangle (the half that is read): ENOTPD at a pivot no later than its column, never a
    returned matrix"""
    A, _ = spd(300, 10.0, 13)
    A[i, j] = v
    assert _spd_fails(api, A) <= j
    _spd_recovers(api)


def test_spd_inverse_nan_lower_is_not_read(api):
    """NaN in the strict lower triangle only: not read, the result is the inverse of the matrix symmetrised from the upper
    triangle (the NaN-free one), to the bit"""
    A, _ = spd(300, 10.0, 14)
    want = api.spd_inverse(A)
    B = A.copy()
    B[np.tril_indices(300, -1)] = np.nan
    got = api.spd_inverse(B)
    assert np.array_equal(got, want)
    _spd_recovers(api)


# ----------------------------------------------------------------------------- the device entry point (torch tensors)
def _padded(n, lda, offset, value):
    """an n x n view with leading dimension lda into a buffer filled with value, starting `offset` doubles in"""
    import torch
    buf = torch.full((offset + n * lda,), value, device="cuda", dtype=torch.float64)
    return buf, buf[offset:].view(n, lda)[:, :n]


@pytest.mark.parametrize("n,lda,offset", [(257, 257, 0), (300, 306, 0), (300, 306, 1), (385, 391, 0)],
                         ids=["odd_lda_copy", "even_lda_inplace", "8_byte_aligned_copy", "odd_lda_padded_copy"])
def test_spd_inverse_device_views(api, n, lda, offset):
    """odd lda and a pointer 8 but not 16 bytes aligned (through the aligned copy of spd_inverse_x), even lda > n (in place):
    the same bound as the host path, and the padding of the buffer untouched"""
    import torch
    A, kappa = tridiag(n)
    buf, V = _padded(n, lda, offset, -7.25)
    assert V.stride(0) == lda and (V.data_ptr() % 16 == 8) == (offset % 2 == 1)
    V.copy_(torch.from_numpy(A))
    _, ld = api.spd_inverse(V, return_logdet=True)
    torch.cuda.synchronize()
    err = fwd_err(V.cpu().numpy(), tridiag_inverse(n))
    assert err <= SPD_C * n * EPS * kappa, err
    assert abs(ld - np.log(n + 1)) <= 64 * n * EPS
    full = buf[offset:].view(n, lda)
    assert bool((full[:, n:] == -7.25).all()) and bool((buf[:offset] == -7.25).all())


def test_spd_inverse_device_side_stream(api):
    """the call runs on the torch stream it is handed.  The input is written on a side stream (non-blocking, as torch creates
    them) only after some tens of milliseconds of queued matrix products there, into a buffer that held the identity: work
    issued on any other stream (the null stream does not wait for a non-blocking one) would read the identity, or a
    half-written matrix, and fail the bound"""
    import torch
    n = 1153
    A, kappa = tridiag(n)
    src = torch.from_numpy(A).cuda()
    At = torch.eye(n, device="cuda", dtype=torch.float64)
    M = torch.randn(4096, 4096, device="cuda", dtype=torch.float64) / 64
    P = torch.empty_like(M)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for _ in range(24):
            torch.mm(M, M, out=P)
        At.copy_(src)
        api.spd_inverse(At)
        X = At.clone()
    s.synchronize()
    assert fwd_err(X.cpu().numpy(), tridiag_inverse(n)) <= SPD_C * n * EPS * kappa


_FRESH = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from gemma_amd import api
api.init(0)
Q, _ = np.linalg.qr(np.random.default_rng(385).standard_normal((385, 385)))
A = (Q * np.geomspace(1.0, 1e6, 385)) @ Q.T  # spd(385, 1e6, 385) of tests/test_gpu_vc.py
T = 2.0 * np.eye(1153) - np.eye(1153, k=1) - np.eye(1153, k=-1)
first = api.spd_inverse(A)  # a fresh process: the workspace is reserved for this order (ld = 386)
assert np.array_equal(api.spd_inverse(A), first)
api.spd_inverse(T)  # grows the kept workspace (ld = 1154)
assert np.array_equal(api.spd_inverse(A), first)
np.save(sys.argv[2], first)
"""


def test_spd_inverse_bit_identical_after_larger_order(api, tmp_path):
    """bit-identical from run to run (spd_inv.hip.h) whatever the kept workspace's history: in a fresh process, the first
    call at n = 385 (workspace of that order), a repeat, and a call after one at n = 1153 (a larger leading dimension);
    then, in this process, where earlier tests grew the workspace to n = 20 000, the same call once more"""
    import subprocess
    import sys
    from vccases import ROOT
    out = str(tmp_path / "first.npy")
    r = subprocess.run([sys.executable, "-c", _FRESH, ROOT, out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    A, _ = spd(385, 1e6, 385)
    assert np.array_equal(api.spd_inverse(A), np.load(out))


# ----------------------------------------------------------------------------- the fit at its widths
def wide_case(nvc, ncvt, n=1500, snps=300, seed=8):
    """nvc kinships of disjoint SNP sets, an intercept and ncvt - 1 random covariates, pve 0.6 spread over the kinships"""
    from oracle import oracle as O
    import vccases as V
    rng = np.random.default_rng(seed + nvc + ncvt)
    Ks, y = [], np.zeros(n)
    for _ in range(nvc):
        G = rng.integers(0, 3, size=(snps, n)).astype(float)
        Ks.append(V.center_matrix(O.calc_kin(G, 1)))
        y += (G - G.mean(1, keepdims=True)).T @ rng.standard_normal(snps) * np.sqrt(0.6 / nvc / snps / 0.5)
    W = np.column_stack([np.ones(n), rng.standard_normal((n, ncvt - 1))])
    y += rng.standard_normal(n) * np.sqrt(0.4) + W @ rng.standard_normal(ncvt) * 0.3
    return Ks, W, y


@pytest.mark.parametrize("nvc,ncvt", [(5, 7), (8, 64)])
def test_vc_wide(api, nvc, ncvt):
    """n_vc up to VC_MAX_K = 8 (9 vectors per REML mat-vec pass, 36 HE trace pairs) and n_cvt up to 64 (a rank-128 centring
    update, Xd at 2 c columns): HE against the numpy restatement, REML against GEMMA's stop rule and the numpy formulas"""
    Ks, W, y = wide_case(nvc, ncvt)
    got = api.VC().CalcVChe(Ks, W, y)
    ref = he(Ks, W, y)
    for key in ("sigma2", "se_sigma2", "pve", "se_pve"):
        assert np.allclose(getattr(got, "v_" + key), ref[key], rtol=1e-10, atol=1e-14), key
    assert abs(got.pve_total - ref["pve_total"]) <= 1e-10 * abs(ref["pve_total"])
    assert abs(got.se_pve_total - ref["se_pve_total"]) <= 1e-10 * abs(ref["se_pve_total"])
    r = api.VC().CalcVCreml(Ks, W, y)
    check_reml(r, Ks, W, y, optimum=False)


@pytest.mark.parametrize("pad", [3, 8], ids=["odd_ldk", "even_ldk"])
def test_vc_device_kinship_views(api, pad):
    """device kinships as views with ldk = n + pad: the HE and REML fits of the host kinships, to 1e-12"""
    import torch
    Ks, W, y = wide_case(3, 2, n=500, snps=200)
    n = len(y)
    views = []
    for K in Ks:
        buf = torch.full((n, n + pad), float("nan"), device="cuda", dtype=torch.float64)
        buf[:, :n] = torch.from_numpy(K).cuda()
        views.append(buf[:, :n])
    assert views[0].stride(0) == n + pad
    for fit in ("CalcVChe", "CalcVCreml"):
        h, d = getattr(api.VC(), fit)(Ks, W, y), getattr(api.VC(), fit)(views, W, y)
        for key in ("v_sigma2", "v_se_sigma2", "v_pve", "v_se_pve", "pve_total", "se_pve_total"):
            assert np.allclose(getattr(d, key), getattr(h, key), rtol=1e-12, atol=0), (fit, key)
        if fit == "CalcVCreml":
            assert (d.status, d.iterations) == (h.status, h.iterations) and h.status == 0


def test_vc_rejected_calls(api):
    """the argument and state errors of gemma_hip_vc_*; a good fit after each"""
    import ctypes as C
    from gemma_amd import _lib as L
    lib = L.lib()
    Ks, W, y = wide_case(2, 2, n=200, snps=100)
    n = len(y)
    keep = [np.ascontiguousarray(K) for K in Ks] * 5
    P = C.POINTER(C.c_double)

    def setup(nvc, ncvt=2, ldk=n, Wm=W, null_at=None, nn=n):
        arr = (C.c_void_p * max(nvc, 1))()
        for i in range(nvc):
            arr[i] = None if i == null_at else keep[i].ctypes.data
        Wc = np.ascontiguousarray(Wm[:nn, :ncvt] if Wm.shape[1] >= ncvt else np.tile(Wm, (1, 40))[:nn, :ncvt])
        return lib.gemma_hip_vc_setup(nn, nvc, C.cast(arr, C.POINTER(C.c_void_p)), ldk, Wc.ctypes.data_as(P), ncvt,
                                      np.ascontiguousarray(y[:nn]).ctypes.data_as(P))

    def he():
        o = [np.zeros(9), np.zeros(9), np.zeros(8), np.zeros(8)]
        return lib.gemma_hip_vc_he(*[a.ctypes.data_as(P) for a in o], C.byref(C.c_double()), C.byref(C.c_double()))

    def reml():
        o = [np.zeros(9), np.zeros(9), np.zeros(8), np.zeros(8)]
        return lib.gemma_hip_vc_reml(0, *[a.ctypes.data_as(P) for a in o], C.byref(C.c_double()), C.byref(C.c_double()),
                                     C.byref(C.c_int()), C.byref(C.c_int()), (C.c_long * 2)(), None, 0)

    good = api.VC().CalcVChe(Ks, W, y)

    def still_good():
        again = api.VC().CalcVChe(Ks, W, y)
        assert np.array_equal(again.v_sigma2, good.v_sigma2)

    lib.gemma_hip_vc_release()
    assert he() == L.ESTATE and reml() == L.ESTATE  # before any setup
    still_good()
    for kw in (dict(nvc=0), dict(nvc=9), dict(nvc=2, ncvt=0), dict(nvc=2, ncvt=65), dict(nvc=2, ncvt=10, nn=10),
               dict(nvc=2, ldk=n - 1), dict(nvc=2, null_at=1)):
        assert setup(**kw) == L.EINVAL, kw
        assert he() == L.ESTATE and reml() == L.ESTATE, kw  # a failed setup leaves no fit behind
        still_good()
    # a repeated column, as it is and in other units (W^T W singular: its equilibrated pivot is a rounding residual)
    for Wsing in (np.column_stack([W, W[:, 1]]), np.column_stack([W, 1e8 * W[:, 1]]), np.column_stack([1e-8 * W, W[:, 1]])):
        assert setup(2, 3, Wm=Wsing) == L.OK
        assert he() == L.EINVAL and reml() == L.EINVAL
        lib.gemma_hip_vc_release()
        still_good()
    assert setup(2) == L.OK and he() == L.OK
    lib.gemma_hip_vc_release()
    assert he() == L.ESTATE and reml() == L.ESTATE  # after vc_release
    still_good()


@pytest.mark.parametrize("scale", [1e8, 1e-8])
def test_vc_covariate_units(api, scale):
    """V1c with its first covariate in other units (x 1e8, x 1e-8): a full-rank W whatever the scale of its columns.  HE
    against the numpy restatement on the same inputs to 1e-10; REML to the reference's own run on the unscaled inputs
    (test_reference_vc_reml[V1cr]): the same trip count, every field within 1e-8 (the fit depends on W through its column
    space only)"""
    from refcases import Calls
    Ks, W, y = inputs("V1c")
    W2 = W.copy()
    W2[:, 1] *= scale
    got = api.VC().CalcVChe(Ks, W2, y)
    ref = he(Ks, W2, y)
    for key in ("sigma2", "se_sigma2", "pve", "se_pve", "pve_total", "se_pve_total"):
        g = np.atleast_1d(getattr(got, "v_" + key) if hasattr(got, "v_" + key) else getattr(got, key))
        assert np.allclose(g, np.atleast_1d(ref[key]), rtol=1e-10, atol=0), (key, g, ref[key])
    rr = ref_reml(Calls("test_reference_vc_reml[V1cr]", None, None).ref, Ks, W, y)
    r = api.VC().CalcVCreml(Ks, W2, y)
    assert (r.status, r.iterations) == (rr["status"], rr["iterations"]) == (0, 6)
    for key in ("sigma2", "se_sigma2", "pve", "se_pve", "pve_total", "se_pve_total"):
        g = np.atleast_1d(getattr(r, "v_" + key) if hasattr(r, "v_" + key) else getattr(r, key))
        assert np.allclose(g, np.atleast_1d(rr[key]), rtol=1e-8, atol=0), (key, g, rr[key])

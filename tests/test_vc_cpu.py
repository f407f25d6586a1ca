"""-vc 1 / -vc 2 without a GPU: the numpy restatements against the reference's printed numbers, the host hybridsj
restatement against scipy's MINPACK hybr, and the new entry points failing loudly without a device."""
import os
import subprocess

import numpy as np
import pytest

from vccases import HE_CASES, HE_KEYS, ROOT, fixture, he, p_inputs, reml_log_dev, reml_summary


@pytest.mark.parametrize("tag,inputs", HE_CASES, ids=[c[0] for c in HE_CASES])
def test_numpy_he_reproduces_reference(tag, inputs):
    Ks, W, y = inputs()
    fx = fixture(tag)
    assert int(fx["number of analyzed individuals"]) == len(y) and int(fx["number of covariates"]) == W.shape[1]
    assert int(fx["number of variance components"]) == len(Ks)
    r = he(Ks, W, y)
    for key, fk in HE_KEYS:
        if fk not in fx:  # the totals are printed for n_vc > 1 only
            continue
        ref = np.array(fx[fk], dtype=float)
        assert np.allclose(np.atleast_1d(r[key]), ref, rtol=5e-6, atol=0), (key, r[key], ref)


def test_numpy_reml_reproduces_reference_null():
    from scipy.optimize import root
    K, W, y, *_ = p_inputs(False)
    h = he([K], W, y)["sigma2"]
    x0 = np.log(np.where(h > 0, h, 0.1))
    sol = root(lambda x: reml_log_dev(x, [K], W, y)[0], x0, jac=lambda x: reml_log_dev(x, [K], W, y)[1], method="hybr")
    assert sol.success
    s2 = np.exp(sol.x)
    fx = fixture("P4")
    assert abs(s2[0] / float(fx["vg estimate in the null model"]) - 1) < 1e-3
    assert abs(s2[1] / float(fx["ve estimate in the null model"]) - 1) < 1e-3
    pve = reml_summary(s2, [K], W, y)["pve"][0]
    assert abs(pve / float(fx["pve estimate in the null model"]) - 1) < 1e-3


def _f(name, x):
    x = np.asarray(x, dtype=float)
    if name == "rosenbrock":
        return np.array([10 * (x[1] - x[0] ** 2), 1 - x[0]])
    if name == "powell_badly_scaled":
        return np.array([1e4 * x[0] * x[1] - 1, np.exp(-x[0]) + np.exp(-x[1]) - 1.0001])
    if name == "trig":
        n = len(x)
        return n - np.cos(x).sum() + np.arange(1, n + 1) * (1 - np.cos(x)) - np.sin(x)
    c = np.array([5.0, 7.0, 10.0])
    return x * x + x.sum() - c


@pytest.fixture(scope="module")
def hybrid_exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hybrid") / "hybrid_check")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "hybrid_check.cpp"), "-o", out])
    return out


@pytest.mark.parametrize("name,x0", [("rosenbrock", [-1.2, 1.0]), ("powell_badly_scaled", [0.0, 1.0]),
                                     ("trig", [0.1, 0.1, 0.1]), ("quadratic3", [1.0, 1.0, 1.0])])
def test_hybridsj_restatement_matches_scipy_hybr(hybrid_exe, name, x0):
    from scipy.optimize import root
    out = subprocess.run([hybrid_exe, name] + [str(v) for v in x0], capture_output=True, text=True, check=True).stdout.split()
    status, x = int(out[0]), np.array([float(v) for v in out[2:]])
    assert status == 0
    ref = root(lambda z: _f(name, z), x0, method="hybr", options={"xtol": 1e-14})
    assert ref.success
    assert np.abs(_f(name, x)).sum() < 1e-10
    assert np.allclose(x, ref.x, rtol=1e-6, atol=1e-9), (x, ref.x)


def test_new_entry_points_fail_without_device():
    """No CPU fallback: without a gfx950 device every new entry point returns an error (when the library is built here)."""
    from gemma_amd import _lib as L
    try:
        lib = L.lib()
    except ImportError:
        pytest.skip("library not built")
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is visible")
    except ImportError:
        pass
    from gemma_amd import api
    with pytest.raises(L.GemmaHipError) as e:
        api.spd_inverse(np.eye(4))
    assert e.value.code == L.ENODEV
    with pytest.raises(L.GemmaHipError):
        api.VC().CalcVChe([np.eye(4)], np.ones((4, 1)), np.arange(4.0))
    with pytest.raises(L.GemmaHipError):
        api.VC().CalcVCreml([np.eye(4)], np.ones((4, 1)), np.arange(4.0))
    assert lib.gemma_hip_vc_he(None, None, None, None, None, None) != L.OK
    assert lib.gemma_hip_strerror(L.ENOTPD).decode() == "matrix not positive definite"


@pytest.mark.parametrize("n", [257, 385])
@pytest.mark.parametrize("kappa", [1e2, 1e6, 1e10])
def test_spd_reference_sits_100x_below_the_bound(n, kappa):
    """the high-precision reference of tests/test_gpu_vc.py's prescribed-spectrum inverses (vccases.spd_spectrum), at its
    largest sizes.  Its error has two parts, each held below 1 / 100 of the bound SPD_C n eps kappa asserted there:
    - what one Newton step leaves: measured as the move of a second long-double step (observed: below 2e-3 of the bound);
    - the floor of the long-double residual I - A X itself, which a further step cannot reveal: estimated as the effect on X
      of the difference between the residual summed in forward and in reverse order (observed: below 4e-5 of the bound)."""
    from vccases import SPD_C, spd_spectrum
    bound = SPD_C * n * np.finfo(float).eps * kappa
    A, X1 = spd_spectrum(n, kappa, n)
    _, X2 = spd_spectrum(n, kappa, n, steps=2)
    moved = np.abs(X2 - X1).max() / np.abs(X2).max()
    Al, Xl = A.astype(np.longdouble), X1.astype(np.longdouble)
    d = (Al @ Xl - Al[:, ::-1] @ Xl[::-1, :]).astype(np.float64)
    floor = np.abs(X1 @ d).max() / np.abs(X1).max()
    assert moved <= bound / 100 and floor <= bound / 100, (moved / bound, floor / bound)

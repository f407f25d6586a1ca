"""The whole-panel null fit without a GPU: the conditions on the cases of tests/test_gpu_null_panel.py from the oracle alone, the
keys of the reference-log fixtures, the exported prototypes and the record layout, and no CPU fall-back."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nullpanelcases as nc

ROOT = nc.ROOT
NAMES = ("gemma_hip_lmm_null_panel", "gemma_hip_lmm_null_panel_d")


@pytest.mark.parametrize("n,c", nc.ORACLE_SHAPES)
def test_cases_reach_both_ends_of_the_lambda_range(oracle, n, c):
    """(203, 1) and (203, 3): ML fits at l_min, at l_max and inside, REML fits at l_min and inside; (1031, 6): interior but for one.
    The planted span column has no fit for c >= 2 and a fit at l_min for c = 1; the zero column has one."""
    ref = nc.oracle_fits(oracle, n, c)
    lo, hi, mid = nc.ends(ref[:, 0])
    rlo, rhi, rmid = nc.ends(ref[:, 2])
    print("n=%d c=%d: ML fits at l_min / l_max / inside %s, REML %s" % (n, c, (lo, hi, mid), (rlo, rhi, rmid)))
    assert np.isfinite(ref[:len(nc.H2S)]).all()
    if (n, c) == (1031, 6):
        assert lo + hi >= 1 and mid >= 15
    else:
        assert lo >= 1 and hi >= 1 and mid >= 1
        assert rlo >= 1 and rmid >= 1
    assert np.isnan(ref[nc.SPAN]).all() if c >= 2 else (ref[nc.SPAN, 0] == nc.L_MIN and np.isfinite(ref[nc.SPAN]).all())
    assert np.isfinite(ref[nc.ZERO]).all()


def test_small_panel_has_every_ml_fit_at_l_max(oracle):
    """(61, 2): every ML fit at l_max, REML fits at both ends"""
    ref = nc.oracle_fits(oracle, 61, 2)
    assert nc.ends(ref[:, 0]) == (0, len(nc.H2S), 0)
    rlo, rhi, rmid = nc.ends(ref[:, 2])
    assert rlo >= 1 and rhi >= 1 and rmid >= 1


@pytest.mark.parametrize("n,c", nc.BETA_SHAPES)
def test_gram_matrices_are_well_conditioned_where_beta_is_compared(oracle, n, c):
    """cond(UtW' H UtW) < 1e4 at the oracle's REML lambda of every trait column (random normal covariates and an intercept)"""
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    ref = nc.oracle_fits(oracle, n, c)
    conds = [nc.gram_cond(ev, UtW, ref[t, 2]) for t in range(len(nc.H2S))]
    print("n=%d c=%d: largest condition number %.3g" % (n, c, max(conds)))
    assert max(conds) < nc.COND_MAX
    _, _, b, s = oracle.calc_vg_ve_beta(ev, UtW, np.ascontiguousarray(UtY[:, 4]), ref[4, 2])
    assert np.isfinite(b).all() and (s > 0).all()


def test_shapes_cover_every_kernel_family():
    assert nc.T == 19 and all(nc.T % w for w in (2, 4, 8, 16))
    assert sorted(c for _, c in nc.BIT_SHAPES) == [1, 2, 3, 5, 6, 18]  # FixedC<0>, <1>, <2>, <4>, generic, wide
    assert all(n % 64 for n, _ in nc.BIT_SHAPES) and min(n for n, _ in nc.BIT_SHAPES) < 64
    assert max(c for _, c in nc.BETA_SHAPES) == 16


@pytest.mark.parametrize("t", [1, 2, 3])
def test_reference_log_fixtures(t):
    log = nc.fx_log(t)
    assert sorted(log) == ["beta", "logl_mle_H0", "logl_remle_H0", "pve", "pve_se", "se_beta", "ve", "vg"]
    assert len(log["beta"]) == len(log["se_beta"]) == 2
    vals = [float(log[k]) for k in ("logl_mle_H0", "logl_remle_H0", "pve", "pve_se", "vg", "ve")] + [float(v) for v in log["beta"] + log["se_beta"]]
    assert np.isfinite(vals).all()
    assert 1e-2 < float(log["vg"]) / float(log["ve"]) < 1e2  # the REML lambda is inside: se(pve) is well conditioned
    Y = np.loadtxt(os.path.join(nc.FX, "Sb3.pheno.txt"))
    assert Y.shape == (300, 3) and np.isfinite(Y).all()


def test_null_fit_layout():
    from gemma_amd import _lib, api
    assert C.sizeof(_lib.NullFit) == 64
    assert api.NULL_DTYPE.itemsize == 64 and api.NULL_DTYPE.names == nc.FIELDS == tuple(k for k, _ in _lib.NullFit._fields_)
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    assert re.search(r"typedef struct \{\s*double l_mle_null, logl_mle_H0, l_remle_null, logl_remle_H0, pve, pve_se, vg_remle, ve_remle;\s*\} "
                     r"gemma_null_fit;", hdr)
    assert "#define GEMMA_HIP_ABI_VERSION 4" in hdr


def test_null_panel_symbols_and_prototypes():
    from gemma_amd import _lib, build
    so = build.build()
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    lib = _lib.lib()
    raw = C.CDLL(so)
    kinds = {"size_t": C.c_size_t, "int": C.c_int, "double": C.c_double}
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/gemma_hip.h"
        assert hasattr(raw, name), name + " is not exported by the library"
        assert name in _lib.SYMBOLS
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        bound = getattr(lib, name).argtypes
        assert bound is not None and len(bound) == len(params) == (14 if name.endswith("_d") else 13), (name, len(params))
        for decl, ct in zip(params, bound):
            if "*" in decl:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, decl, ct)
            else:
                assert ct is kinds[decl.split()[-2]], (name, decl, ct)


def test_null_panel_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        return  # covered by tests/test_gpu_null_panel.py
    from gemma_amd import _lib, api
    n = 8
    with pytest.raises(_lib.GemmaHipError) as e:
        api.CalcLambdaNullPanel(np.ones(n), np.ones((n, 1)), np.ones((n, 2)))
    assert e.value.code == _lib.ENODEV

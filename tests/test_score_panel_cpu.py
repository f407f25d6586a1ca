"""The score panel without a GPU: the closed form the device kernel evaluates (tests/scorecases.py, long double) against the
oracle's mode 3 (CalcRLScore on CalcPab's recursion), the record layout, the exported prototypes, and no CPU fall-back."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import scorecases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gemma_hip_lmm_score_panel_setup", "gemma_hip_lmm_score_panel_setup_d", "gemma_hip_lmm_score_panel_setup_kept",
         "gemma_hip_lmm_score_panel_batch", "gemma_hip_lmm_score_panel_batch_d", "gemma_hip_lmm_score_panel_assoc_d")


@pytest.mark.parametrize("c", [1, 3, 16])
def test_closed_form_agrees_with_the_recursion(oracle, c):
    """n = 203, T = 5 with heritabilities 0 ... 0.95 and fitted nulls: 1e-7 relative on beta, se and p_score.  A condition on the
    inputs (well conditioned), not the device path's bar: the fp64 recursion and long double differ by <= 2e-9 even at lambda = 1e5."""
    X, U, ev, UtW, UtY = sc.panel(203, c, 5)
    lams = [oracle.calc_lambda_null("L", ev, UtW, np.ascontiguousarray(UtY[:, t]))[0] for t in range(5)]
    assert max(lams) > 100 * min(lams), lams  # the nulls spread over decades
    UtX = np.ascontiguousarray(oracle.impute_mean(X[:200]) @ U)
    want = sc.oracle_records(oracle, ev, UtW, UtY, lams, UtX)
    got, ratio = sc.closed_form(oracle, ev, UtW, UtY, lams, UtX)
    assert (ratio >= sc.PXX_FLOOR).all()  # maf >= 0.05, 1 % missing: no pair is left out
    err = sc.rel_err(got, want)
    worst = {k: float(err[k].max()) for k in sc.FIELDS}
    print("closed form vs recursion, c = %d:" % c, worst)
    assert max(worst.values()) <= 1e-7, worst


def test_closed_form_at_the_ends_of_the_lambda_range(oracle):
    X, U, ev, UtW, UtY = sc.panel(203, 3, 5)
    UtX = np.ascontiguousarray(oracle.impute_mean(X[:100]) @ U)
    lams = [1e-5, 1e-2, 1.0, 1e2, 1e5]
    err = sc.rel_err(sc.closed_form(oracle, ev, UtW, UtY, lams, UtX)[0], sc.oracle_records(oracle, ev, UtW, UtY, lams, UtX))
    assert max(float(err[k].max()) for k in sc.FIELDS) <= 1e-7


def test_score_rec_layout():
    from gemma_amd import _lib, api
    assert C.sizeof(_lib.ScoreRec) == 24
    assert api.SCORE_DTYPE.itemsize == 24 and api.SCORE_DTYPE.names == ("beta", "se", "p_score")
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    assert re.search(r"typedef struct \{\s*double beta, se, p_score;\s*\} gemma_score_rec;", hdr)


def test_score_panel_symbols_and_prototypes():
    from gemma_amd import _lib, build
    so = build.build()
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    lib = _lib.lib()
    raw = C.CDLL(so)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/gemma_hip.h"
        assert hasattr(raw, name), name + " is not exported by the library"
        assert name in _lib.SYMBOLS
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        bound = getattr(lib, name).argtypes
        assert bound is not None and len(bound) == len(params), (name, len(params))
        for decl, ct in zip(params, bound):
            if "*" in decl:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, decl, ct)
            else:
                assert ct is {"size_t": C.c_size_t, "int": C.c_int}[decl.split()[-2]], (name, decl, ct)


def test_score_panel_setup_needs_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_score_panel.py")
    from gemma_amd import _lib, api
    n = 8
    lmm = api.LMM(a_mode=3)
    with pytest.raises(_lib.GemmaHipError) as e:
        lmm.setup_score_panel(np.eye(n), np.ones(n), np.ones((n, 1)), np.ones((n, 2)), [1.0, 1.0])
    assert e.value.code == _lib.ENODEV

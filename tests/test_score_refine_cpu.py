"""The refinement of the score panel's hits without a device: the new declarations of include/gemma_hip.h against their ctypes
bindings, the cases of tests/scorerefinecases.py, and the oracle's own records on the pairs that tests/test_gpu_score_refine.py
holds to the definition -- the sample is chosen so that nothing of it is left out (lmmdefcases.LEFT_OUT_MAX)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import lmmdefcases as D
import scorerefinecases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"gemma_hip_lmm_score_panel_refine_setup": 2, "gemma_hip_lmm_score_panel_refine_setup_d": 3,
         "gemma_hip_lmm_score_panel_refine_assoc_d": 7, "gemma_hip_lmm_score_panel_refine_last_d": 4,
         "gemma_hip_lmm_score_panel_hits_refine_batch": 10}


def test_refine_symbols_and_prototypes():
    from gemma_amd import _lib, build
    so = build.build()
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    lib = _lib.lib()
    raw = C.CDLL(so)
    kinds = {"size_t": C.c_size_t, "int": C.c_int, "double": C.c_double}
    for name, arity in NAMES.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/gemma_hip.h"
        assert hasattr(raw, name), name + " is not exported by the library"
        assert name in _lib.SYMBOLS
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        bound = getattr(lib, name).argtypes
        assert bound is not None and len(bound) == len(params) == arity, (name, len(params))
        for decl, ct in zip(params, bound):
            if "*" in decl:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, decl, ct)
            else:
                assert ct is kinds[decl.split()[-2]], (name, decl, ct)
    assert "#define GEMMA_HIP_ABI_VERSION 4" in hdr
    # every refine declaration of the header is in the list above
    assert set(re.findall(r"\bint\s+(gemma_hip_lmm_score_panel_\w*refine\w*)\s*\(", hdr)) == set(NAMES)


def test_mirrors_keep_their_defaults():
    import inspect
    from gemma_amd import api
    sig = inspect.signature(api.LMM.AnalyzeScorePanelHits).parameters
    assert sig["refine"].default is False and sig["logl_mle_H0"].default is None
    assert inspect.signature(api.LMM.batch_score_panel_hits).parameters["refine"].default is False
    for name in ("setup_score_refine", "assoc_score_refine", "refine_last"):
        assert callable(getattr(api.LMM, name))


@pytest.mark.parametrize("n,c,T", R.SHAPES + (R.FORCED,))
def test_panels_and_lists(oracle, n, c, T):
    p = R.panel(oracle, n, c, T)
    d = D.case(oracle, n, c)
    assert p["UtX"].shape == (R.L_ROWS, n) and p["UtY"].shape == (n, T) and 1 <= c <= 16
    assert np.array_equal(p["UtX"][:R.MONO], d["UtX"][p["rows"]]) and np.array_equal(p["UtY"][:, :3], d["UtY"][:, :min(T, 3)][:, :3])
    if (n, c, T) in R.DEF_SHAPES:
        assert len(set(p["rows"])) == R.L_ROWS - 2  # the sampled rows are rows of the case, each once
    # the monomorphic row is a multiple of the rotated intercept (the last covariate of the case's W is not: find it by regression)
    x = p["UtX"][R.MONO]
    res = x - p["UtW"] @ np.linalg.lstsq(p["UtW"], x, rcond=None)[0]
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(x)
    assert np.isnan(p["UtX"][R.MISSING]).all() and np.isfinite(p["UtX"][:R.MISSING]).all() and np.isfinite(p["UtY"]).all()
    lists = R.pair_lists(n, c, T)
    assert ("all" in lists) == ((n, c, T) == R.SHAPES[0])
    for name, pairs in lists.items():
        assert pairs.ndim == 2 and pairs.shape[1] == 2
        assert (pairs[:, 0] >= 0).all() and (pairs[:, 0] < R.L_ROWS).all() and (pairs[:, 1] >= 0).all() and (pairs[:, 1] < T).all(), name
    assert len(lists["one"]) == 1 and len(lists["five"]) == 5 and len(lists["five"]) % 4 != 0
    assert {R.MONO, R.MISSING} <= set(lists["five"][:, 0])
    key = lists["reversed"][:, 1] * R.L_ROWS + lists["reversed"][:, 0]
    assert (np.diff(key) < 0).all()
    rep = [tuple(r) for r in lists["repeated"]]
    assert max(rep.count(r) for r in rep) == 3
    if "all" in lists:
        assert len(set(map(tuple, lists["all"]))) == T * R.L_ROWS


@pytest.mark.parametrize("n,c,T", R.DEF_SHAPES)
def test_the_oracle_leaves_no_sampled_pair_out(oracle, n, c, T):
    """on the sampled pairs the oracle's own records meet what the GPU test asks of the device: no failed search, no pair with
    P_xx / sum h x^2 below RATIO_MIN, no lambda-hat left out or failing criteria (a)-(c) -- within LEFT_OUT_MAX, which for 12 pairs
    per trait is none"""
    p = R.panel(oracle, n, c, T)
    g = D.GRIDS["default"]
    for t, rows in R.def_sample(n, c, T).items():
        assert (rows < R.MONO).all() and len(set(rows)) == R.DEF_PER_TRAIT
        idx = p["rows"][rows]
        y = np.ascontiguousarray(p["UtY"][:, t])
        UtX = np.ascontiguousarray(p["UtX"][rows])
        l_mle, logl0 = oracle.calc_lambda_null("L", p["ev"], p["UtW"], y, **g)
        kw = dict(l_mle_null=l_mle, logl_mle_H0=logl0, **g)
        r1, r2, r3 = (oracle.lmm_batch_UtX(m, p["ev"], p["UtW"], y, UtX, **kw) for m in (1, 2, 3))
        alt, nul = D.Model(p["ev"], p["UtW"], y, UtX), D.models(oracle, n, c, t)[1]
        for name, rec, ref in (("wald", r1, alt.at(r1["lambda_remle"])), ("ml", r2, alt.at(r2["lambda_mle"])), ("score", r3, alt.score(l_mle, nul))):
            out = np.asarray(ref["ratio"] < D.RATIO_MIN) | np.isnan(rec["logl_H1"] if name != "score" else rec["p_score"])
            assert out.mean() <= D.LEFT_OUT_MAX, (t, name, np.flatnonzero(out))
        for reml, rec, key in ((True, r1, "lambda_remle"), (False, r2, "lambda_mle")):
            lam_star, _, vals, lams = D.maximum(oracle, n, c, t, reml, **g)
            assert (alt.at(lam_star[idx])["ratio"] < D.RATIO_MIN).mean() <= D.LEFT_OUT_MAX
            ok, left, text = D.lambda_criteria(rec[key], alt.at(rec[key])["reml" if reml else "ml"], lam_star[idx], vals[:, idx], lams,
                                               g["l_min"], g["l_max"])
            assert left.mean() <= D.LEFT_OUT_MAX and ok.all(), (t, reml, text)

"""The trait-pair panel on the GPU (tests/pairpanelcases.py): gemma_hip_mvlmm_null_pairs / _d and gemma_hip_mvlmm_null_se through
gemma_amd.api.  The pair kernel is mv_null_fit<2, C> on the inputs gemma_hip_mvlmm_null(d = 2) gives it, so the fields both report
are compared in bits; the new fields (variances, correlations) are held to BAR against the reference composed from the oracle's
primitives at fixed iteration counts, where both sides take the same iterations.

Worst deviation from the composition measured on an MI355X over the 30 pairs (printed per case by -s):
    Vg 1.1e-14  Ve 7.2e-15  logl 8.5e-16  B 4.2e-15  VVg 1.4e-14  VVe 2.4e-14  VB 5.5e-15
    rg 8.5e-13 (cw 6: a correlation near zero)  var_rg 2.7e-14  re 2.9e-13 (cw 3)  var_re 9.9e-15
    gemma_hip_mvlmm_null_se: (3, 2) fixed VV 1.0e-14, VB 2.1e-15; (2, 8) run-time VV 7.8e-15, VB 1.8e-15"""
import ctypes as C

import numpy as np
import pytest

import pairpanelcases as P

pytestmark = pytest.mark.gpu


def _opt(fixed):
    from gemma_amd import _lib as L
    cfg = P.cfg_of(fixed)
    return L.MvOpt(cfg.em_iter, cfg.nr_iter, cfg.em_prec, cfg.nr_prec, cfg.p_nr, 0, 0)


def _inputs(cw, UtY=None):
    c = P.case(cw)
    return np.array(c["ev"]), np.array(c["UtW"].T, order="C"), np.array(c["UtY"].T, order="C") if UtY is None else UtY


_RUNS = {}


def _panel(api, cw, fixed):
    """the full host run of case(cw) with B and VB, once per (cw, fixed): (fit, B, VB), read-only"""
    if (cw, fixed) not in _RUNS:
        r = api.CalcMvNullPairs(*_inputs(cw), opt=_opt(fixed), want_beta=True)
        for a in r:
            a.setflags(write=False)
        _RUNS[(cw, fixed)] = r
    return _RUNS[(cw, fixed)]


def _same(a, b):
    """two results of CalcMvNullPairs (tuples of arrays) in bits"""
    return len(a) == len(b) and all(x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("cw,seed", P.CASES)
def test_bits_of_the_existing_entry(gpu_api, cw, seed):
    """pairs = NULL at the default tolerances: Vg, Ve, logl of both blocks and B equal gemma_hip_mvlmm_null(d = 2) on the two
    gathered columns, bit for bit"""
    fit, B, _ = _panel(gpu_api, cw, False)
    ev, UtW, UtY = _inputs(cw)
    assert [(f["i"], f["j"]) for f in fit] == P.PAIRS
    for q, (i, j) in enumerate(P.PAIRS):
        one = gpu_api.MVLMM().fit_null(ev, UtW, np.ascontiguousarray(UtY[:, [i, j]]))
        for p, tag in enumerate(("remle", "mle")):
            b = fit[q][tag]
            assert np.array_equal(b["Vg"], one["Vg_" + tag][P.IU]) and np.array_equal(b["Ve"], one["Ve_" + tag][P.IU]), (i, j, tag)
            assert one["Vg_" + tag][1, 0] == one["Vg_" + tag][0, 1]
            assert b["logl"] == one["logl_" + tag], (i, j, tag)
            assert np.array_equal(B[q, p], one["B_" + tag]), (i, j, tag)


@pytest.mark.parametrize("cw,seed", P.CASES)
def test_fixed_counts_against_the_composed_reference(gpu_api, cw, seed):
    """every field, the new ones included, within BAR = 32 x CAP of the composition; status 0 everywhere"""
    fit, B, VB = _panel(gpu_api, cw, True)
    ref = P.reference(cw)
    worst = dict.fromkeys(P.BLOCK_FIELDS, 0.0)
    for q, r in enumerate(ref):
        assert fit[q]["status"] == 0
        for p, tag in enumerate(("remle", "mle")):
            for k, v in P.deviations(P.block_of(fit[q][tag], B[q, p], VB[q, p]), r[tag]).items():
                worst[k] = max(worst[k], v) if v == v else v
    print("gpu pairs vs composition cw=%d: " % cw + "  ".join("%s %.1e" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v < P.BAR, (cw, k, v)


@pytest.mark.parametrize("cw", [1, 6])
def test_ways_in(gpu_api, monkeypatch, cw):
    """the _d form, an explicit list (the ten pairs reversed plus one repeated) and chunks of 3, 3, 3, 1: all the full host run in bits"""
    import torch
    full = _panel(gpu_api, cw, True)
    ev, UtW, UtY = _inputs(cw)
    dev = [torch.from_numpy(a).cuda() for a in (ev, UtW, UtY)]
    fit_d, B_d, VB_d = gpu_api.CalcMvNullPairs(*dev, opt=_opt(True), want_beta=True)
    got = (fit_d.cpu().numpy().view(gpu_api.MVPAIR_DTYPE).reshape(-1), B_d.cpu().numpy(), VB_d.cpu().numpy())
    assert _same(got, full)
    order = list(range(len(P.PAIRS)))[::-1] + [3]
    lst = np.array([P.PAIRS[q] for q in order], dtype=np.int32)
    got = gpu_api.CalcMvNullPairs(ev, UtW, UtY, pairs=lst, opt=_opt(True), want_beta=True)
    assert _same(got, tuple(a[order] for a in full))
    got_d = gpu_api.CalcMvNullPairs(*dev, pairs=lst, opt=_opt(True))
    assert _same((got_d.cpu().numpy().view(gpu_api.MVPAIR_DTYPE).reshape(-1),), (full[0][order],))
    monkeypatch.setenv("GEMMA_HIP_MVPAIR_CHUNK", "3")
    assert _same(gpu_api.CalcMvNullPairs(ev, UtW, UtY, opt=_opt(True), want_beta=True), full)
    fit_d = gpu_api.CalcMvNullPairs(*dev, opt=_opt(True))
    assert _same((fit_d.cpu().numpy().view(gpu_api.MVPAIR_DTYPE).reshape(-1),), (full[0],))
    monkeypatch.delenv("GEMMA_HIP_MVPAIR_CHUNK")
    monkeypatch.setenv("GEMMA_HIP_MVPAIR_WAVES", "4")  # four pairs per workgroup (two full workgroups and a ragged one): the same fits
    assert _same(gpu_api.CalcMvNullPairs(ev, UtW, UtY, opt=_opt(True), want_beta=True), full)


def test_a_non_finite_column(gpu_api):
    """NaN in one entry of column 2: its four pairs report status 1, the other six are the clean run in bits, the call returns OK"""
    cw = 3
    full = _panel(gpu_api, cw, True)
    ev, UtW, UtY = _inputs(cw)
    UtY = UtY.copy()
    UtY[17, 2] = np.nan
    got = gpu_api.CalcMvNullPairs(ev, UtW, UtY, opt=_opt(True), want_beta=True)
    hit = np.array([2 in p for p in P.PAIRS])
    assert hit.sum() == 4
    assert np.all(got[0]["status"][hit] == 1) and np.all(got[0]["status"][~hit] == 0)
    assert _same(tuple(a[~hit] for a in got), tuple(a[~hit] for a in full))
    m = gpu_api.mv_pair_matrices(got[0], P.T)
    assert np.all(np.isnan(m["rg"][2, [0, 1, 3, 4]])) and m["rg"][2, 2] == 1.0 and np.isfinite(m["rg"][0, 1]) and m["rg"][0, 1] == m["rg"][1, 0]


@pytest.mark.parametrize("d,cw,form", [(3, 2, "fixed"), (2, 8, "run-time")])
def test_null_se(gpu_api, d, cw, form):
    """gemma_hip_mvlmm_null_se: `out` in the bits of gemma_hip_mvlmm_null, the same kernel form reported, VV and VB within BAR of the
    reference under fixed counts"""
    from gemma_amd import _lib as L
    c = P.null_case(d, cw)
    ev, UtW, UtY = np.array(c["ev"]), np.ascontiguousarray(c["UtW"].T), np.ascontiguousarray(c["UtY"].T)
    names = {L.MV_KERNEL_FIXED: "fixed", L.MV_KERNEL_RUN_TIME: "run-time"}
    plain = dict(gpu_api.MVLMM(**P.FIXC).fit_null(ev, UtW, UtY))
    f, dd, rows = gpu_api.last_mvlmm_kernel(1)
    assert (names[f], dd, rows) == (form, d, cw)
    got = gpu_api.MVLMM(**P.FIXC).fit_null(ev, UtW, UtY, want_se=True)
    f, dd, rows = gpu_api.last_mvlmm_kernel(1)
    assert (names[f], dd, rows) == (form, d, cw)
    for k, v in plain.items():
        assert np.array_equal(got[k], v), k
    ref = P.se_reference(d, cw)
    v = d * (d + 1) // 2
    for tag in ("remle", "mle"):
        for k, g, r in (("VVg", got["VVg_" + tag], np.diag(ref[tag]["VV"])[:v]), ("VVe", got["VVe_" + tag], np.diag(ref[tag]["VV"])[v:]),
                        ("VB", got["VB_" + tag], ref[tag]["VB"])):
            w = float(np.abs(g - r).max() / np.abs(r).max())
            print("gpu null_se %s d=%d cw=%d %s %s: %.1e" % (form, d, cw, tag, k, w))
            assert w < P.BAR, (d, cw, tag, k, w)


def test_arguments_and_state(gpu_api):
    """every EINVAL of the header; a preceding lmm_setup is neither needed nor disturbed"""
    from gemma_amd import _lib as L
    lib = L.lib()
    cw = 1
    ev, UtW, UtY = _inputs(cw)
    c = P.case(cw)
    n, T = P.N, P.T
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    m = T * (T - 1) // 2
    fit = (L.MvPairFit * (m + 1))()
    B, VB = np.zeros((m + 1, 2, 2, cw)), np.zeros((m + 1, 2, 2, cw))
    good = np.array(P.PAIRS, dtype=np.int32)

    def call(n=n, c=cw, T=T, ev=dp(ev), W=dp(UtW), Y=dp(UtY), pairs=None, m=0, fit=fit, B=None, VB=None):
        return lib.gemma_hip_mvlmm_null_pairs(n, c, T, ev, W, Y, pairs, m, 1e-5, 1e5, 10, None, fit, B, VB)

    lmm = gpu_api.LMM(a_mode=1)
    lmm.setup(np.array(c["U"]), ev, UtW, np.ascontiguousarray(UtY[:, 0]))
    try:
        G = np.ascontiguousarray(c["G"], dtype=np.float64)
        before = lmm.batch(G, L.GENO_F64_SNP_MAJOR).copy()
        assert call(B=dp(B), VB=dp(VB)) == L.OK and call(pairs=ip(good), m=m) == L.OK and call(m=m) == L.OK
        bad = [dict(ev=None), dict(W=None), dict(Y=None), dict(fit=None), dict(B=dp(B)), dict(VB=dp(VB)), dict(T=1),
               dict(pairs=ip(good), m=0), dict(m=3), dict(n=cw + 1), dict(c=0), dict(c=7),
               dict(pairs=ip(np.array([[1, 1]], dtype=np.int32)), m=1), dict(pairs=ip(np.array([[2, 1]], dtype=np.int32)), m=1),
               dict(pairs=ip(np.array([[0, T]], dtype=np.int32)), m=1), dict(pairs=ip(np.array([[-1, 2]], dtype=np.int32)), m=1)]
        for kw in bad:
            assert call(**kw) == L.EINVAL, kw
        assert call(c=7) == L.EINVAL and b"1..6" in lib.gemma_hip_last_error()  # the message names the limit
        nf, se = L.MvNull(), L.MvNullSe()
        assert lib.gemma_hip_mvlmm_null_se(n, cw, 2, dp(ev), dp(UtW), dp(np.ascontiguousarray(UtY[:, :2])), 1e-5, 1e5, 10, None,
                                           C.byref(nf), None) == L.EINVAL
        after = lmm.batch(G, L.GENO_F64_SNP_MAJOR)
        assert np.array_equal(before.view(np.uint8), after.view(np.uint8))
    finally:
        lmm.finish()

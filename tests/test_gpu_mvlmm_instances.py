"""Every kernel instance of the multivariate LMM stage on the GPU, driven through the C ABI at fixed iteration counts
(tests/mvfixcases.py): the 31 fixed per-SNP instances and the 24 fixed null fits, each its own template instance with its own
registers and LDS layout, the run-time kernel on shapes of its own and on the twins of fixed shapes, a_mode 1 / 2 / 3, more SNPs
than run-time workgroups, and the interaction test.  gemma_hip_dbg_last_mvlmm_kernel must name the form that ran: a fixed instance
that is missing falls back to the run-time kernel with correct numbers, and nothing else would notice.

With the stopping rules off every SNP takes the same iterations in the oracle and on the GPU, so ALL SNPs are held to
BAR = 1e-9 on every field (tests/test_gpu_mvlmm.py: 97 % within 1e-6).  That is 32 x the 3e-11 to which the oracle and the kernel
source on one CPU lane agree on every one of these cases (tests/test_mvlmm_fixed_count_cpu.py): the GPU differs from the one-lane
run by the order of its 64-lane sums over ~131 terms and by fused multiply-adds, rounding-sized perturbations that pass through
the same conditioning as the difference of the two CPU formulations.

Worst deviation from the oracle measured on an MI355X, all SNPs, all fields (printed per case by -s):
    four wavefronts per workgroup (d <= 5)   3.9e-12  (2, 1)
    two (d = 6)                              1.6e-11  (6, 3)      [the oracle and one CPU lane differ by 1.6e-11 there]
    one (d = 7, 8)                           1.1e-11  (8, 1)
    run-time kernel                          6.2e-12  (8, 1) forced; 3.0e-12 (8, 2) among the shapes of its own
    run-time against fixed, same case        4.9e-12  (8, 1)
    a_mode 1 / 2 / 3                         3.9e-12  (2, 1), a_mode 2
    1030 SNPs on 1024 workgroups             3.9e-13
    interaction test                         3.7e-12  (2, 1)
    null fits: logl at the reported (Vg, Ve) 8.5e-16, B against the GLS estimate there 4.1e-15
"""
import ctypes as C

import numpy as np
import pytest

import mvfixcases as M

pytestmark = pytest.mark.gpu


def _run(api, c, a_mode, crt, gxe=False):
    """lmm_setup, mvlmm_set with the synthetic start, one mvlmm_batch on the fp64 SNP-major rows"""
    from gemma_amd import _lib as L
    lib = L.lib()
    d, n, l = c["d"], c["n"], c["l"]
    UtW, UtY = np.ascontiguousarray(c["UtW"].T), np.ascontiguousarray(c["UtY"].T)
    nf = L.MvNull()
    for dst, src in ((nf.Vg_mle, "Vg_mle"), (nf.Ve_mle, "Ve_mle"), (nf.B_mle, "B_mle")):
        for i, x in enumerate(c["null"][src].ravel()):
            dst[i] = x
    nf.logl_mle_H0 = c["null"]["logl_mle"]
    opt = L.MvOpt(M.FIX["em_iter"], M.FIX["nr_iter"], M.FIX["em_prec"], M.FIX["nr_prec"], M.FIX["p_nr"], crt, 1 if gxe else 0)
    G = np.ascontiguousarray(c["G"], dtype=np.float64)
    out = np.zeros((l, d + 3 * (d * (d + 1) // 2) + 3))
    lmm = api.LMM(a_mode=a_mode)
    lmm.setup(np.array(c["U"]), np.array(c["ev"]), UtW, np.ascontiguousarray(UtY[:, 0]))
    try:
        if gxe:
            env = np.ascontiguousarray(c["env"])
            L.check(lib.gemma_hip_lmm_set_env(env.ctypes.data_as(C.POINTER(C.c_double))), "lmm_set_env")
        L.check(lib.gemma_hip_mvlmm_set(d, UtY.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nf), C.byref(opt)), "mvlmm_set")
        L.check(lib.gemma_hip_mvlmm_batch(L.GENO_F64_SNP_MAJOR, C.c_void_p(G.ctypes.data), l, n,
                                          out.ctypes.data_as(C.POINTER(C.c_double))), "mvlmm_batch")
    finally:
        lmm.finish()
    return M.split(out, d)


def _ran(api, which):
    from gemma_amd import _lib as L
    form, d, rows = api.last_mvlmm_kernel(which)
    return {L.MV_KERNEL_NONE: "none", L.MV_KERNEL_FIXED: "fixed", L.MV_KERNEL_RUN_TIME: "run-time"}[form], d, rows


def _family(d, cw, rt=False):
    return "run-time" if rt or not M.is_fixed(d, cw) else "%d-wave" % M.waves(d, cw)


@pytest.mark.parametrize("d,cw,form", [(d, r - 1, "fixed") for d, r in M.FIXED_SNP] + [(d, cw, "run-time") for d, cw in M.RT_SNP])
def test_every_per_snp_instance(gpu_api, d, cw, form):
    c = M.case(d, cw)
    ref = M.reference(c, 4, 1)
    got = _run(gpu_api, c, 4, 1)
    assert _ran(gpu_api, 0) == (form, d, cw + 1)
    w = M.worst_rel(got, ref)
    print("gpu %s d=%d cw=%d: %.2e" % (_family(d, cw), d, cw, w))
    assert w < M.BAR, (d, cw, w)


@pytest.mark.parametrize("d,cw", M.RT_TWINS)
def test_fixed_shapes_through_the_run_time_kernel(gpu_api, monkeypatch, d, cw):
    """GEMMA_HIP_MVLMM_RT=1: the run-time kernel against the oracle where a fixed kernel exists, d > 5 included, and against the
    fixed run of the same case."""
    c = M.case(d, cw)
    ref = M.reference(c, 4, 1)
    fixed = _run(gpu_api, c, 4, 1)
    assert _ran(gpu_api, 0) == ("fixed", d, cw + 1)
    monkeypatch.setenv("GEMMA_HIP_MVLMM_RT", "1")
    rt = _run(gpu_api, c, 4, 1)
    assert _ran(gpu_api, 0) == ("run-time", d, cw + 1)
    w, w2 = M.worst_rel(rt, ref), M.worst_rel(rt, fixed)
    print("gpu run-time twin d=%d cw=%d: %.2e against the oracle, %.2e against the fixed kernel" % (d, cw, w, w2))
    assert w < M.BAR and w2 < M.BAR, (d, cw, w, w2)


@pytest.mark.parametrize("d,cw", M.MODE_SHAPES)
@pytest.mark.parametrize("a_mode", [1, 2, 3])
def test_single_modes(gpu_api, d, cw, a_mode):
    """-lmm 1 / 2 / 3: Wald alone (REML estimates), LRT alone (ML estimates), score alone (no estimates); what a mode does not
    compute stays exactly 0, as mv_one_snp leaves it."""
    c = M.case(d, cw)
    for crt in (0, 1):
        ref = M.reference(c, a_mode, crt)
        got = _run(gpu_api, c, a_mode, crt)
        assert _ran(gpu_api, 0) == ("fixed" if M.is_fixed(d, cw) else "run-time", d, cw + 1)
        w = M.worst_rel(got, ref)
        print("gpu %s d=%d cw=%d a_mode=%d crt=%d: %.2e" % (_family(d, cw), d, cw, a_mode, crt, w))
        assert w < M.BAR, (d, cw, a_mode, crt, w)
        for k in {1: ("p_lrt", "p_score"), 2: ("p_wald", "p_score"), 3: ("p_wald", "p_lrt")}[a_mode]:
            assert np.all(got[k] == 0), k
        if a_mode == 3:  # the estimates of the null, untouched
            iu = np.triu_indices(d)
            assert np.all(got["Vg"] == c["null"]["Vg_mle"][iu]) and np.all(got["Ve"] == c["null"]["Ve_mle"][iu])


def test_more_snps_than_run_time_workgroups(gpu_api, monkeypatch):
    """1030 SNPs on the 1024 workgroups of the run-time kernel: six workgroups take a second SNP on the scratch slab of their first"""
    c = M.case(2, 1, l=1030, rt=True)
    ref = M.reference(c, 4, 1)
    monkeypatch.setenv("GEMMA_HIP_MVLMM_RT", "1")
    got = _run(gpu_api, c, 4, 1)
    assert _ran(gpu_api, 0) == ("run-time", 2, 2)
    w = M.worst_rel(got, ref)
    print("gpu run-time d=2 cw=1 l=1030: %.2e" % w)
    assert w < M.BAR, w


@pytest.mark.parametrize("d,cw", M.GXE_SHAPES)
def test_gxe(gpu_api, d, cw):
    c = M.case(d, cw, seed=M.GXE_SEEDS[(d, cw)], gxe=True)
    for crt in (0, 1):
        ref = M.reference(c, 4, crt, gxe=True)
        got = _run(gpu_api, c, 4, crt, gxe=True)
        assert _ran(gpu_api, 0) == ("run-time", d, cw + 3)  # rows of X: covariates, env, the SNP, the interaction
        w = M.worst_rel(got, ref)
        print("gpu gxe d=%d cw=%d crt=%d: %.2e" % (d, cw, crt, w))
        assert w < M.BAR, (d, cw, crt, w)


@pytest.mark.parametrize("d,cw,form", [(d, cw, "fixed") for d, cw in M.FIXED_NULL] + [(d, cw, "run-time") for d, cw in M.RT_NULL])
def test_every_null_instance(gpu_api, d, cw, form):
    """The null fit starts from univariate lambda fits the test cannot inject, so against the oracle it keeps the bars of
    test_null_model_block; two properties of the result hold at any iteration count and are checked at 1e-9: the reported logl
    is the log-likelihood at the reported (Vg, Ve), and the reported B is the GLS estimate there."""
    c, ref = M.null_case(d, cw), M.null_reference(d, cw)
    ev, W, Y = np.array(c["ev"]), np.array(c["UtW"]), np.array(c["UtY"])
    mv = gpu_api.MVLMM(**M.FIX)
    got = mv.fit_null(ev, np.ascontiguousarray(W.T), np.ascontiguousarray(Y.T))
    assert _ran(gpu_api, 1) == (form, d, cw)
    for k in ("Vg_remle", "Ve_remle", "B_remle", "Vg_mle", "Ve_mle", "B_mle"):
        assert np.abs(got[k] - ref[k]).max() < 1e-6 * np.abs(ref[k]).max(), k
    assert got["logl_remle"] == pytest.approx(ref["logl_remle"], rel=1e-10)
    assert got["logl_mle"] == pytest.approx(ref["logl_mle"], rel=1e-10)
    for func, tag in (("R", "remle"), ("L", "mle")):
        Vg, Ve, B = got["Vg_" + tag], got["Ve_" + tag], got["B_" + tag]
        ll = M.O.mph_em(func, 1, 0.0, ev, W, Y, Vg.copy(), Ve.copy(), B.copy())
        gls = M.gls_B(ev, W, Y, Vg, Ve)
        wl, wb = abs(got["logl_" + tag] - ll) / abs(ll), np.abs(gls - B).max() / np.abs(B).max()
        print("gpu null %s d=%d cw=%d %s: logl %.2e, B %.2e" % (form, d, cw, tag, wl, wb))
        assert wl < M.BAR and wb < M.BAR, (d, cw, tag, wl, wb)

"""The fixed-iteration-count cases of tests/mvfixcases.py on the CPU: the oracle (oracle/mvlmm_oracle.c: explicit H_k^-1 blocks,
the full Q) against the kernel source on one lane (tests/host/mvlmm_harness.cpp: rotated basis, moment tables).  With the stopping
rules off the two formulations take the same iterations, and every committed case must be one on which they agree to CAP = 3e-11
on every field of every SNP: that is the condition on the REFERENCE which lets tests/test_gpu_mvlmm_instances.py hold the GPU to
1e-9.  A seed that misses it is replaced in mvfixcases.SEEDS, never the cap.

Worst oracle-against-one-lane disagreement per kernel family (crt 0 and 1; printed per case by -s):
    four wavefronts per workgroup (d <= 5)   4.3e-12  (2, 1)
    two (d = 6)                              1.6e-11  (6, 3)
    one (d = 7, 8)                           2.4e-12  (8, 1)
    run-time shapes                          1.4e-11  (8, 3)
    a_mode 1 / 2 / 3                         4.3e-12  (2, 1), a_mode 2
    interaction test                         3.8e-12  (2, 1)
Also checked here: that the cases do what they claim (every value finite, every reported V_g, V_e at least 1e-4 inside the
cone, -crt moving every Wald and LRT p value, a ragged last workgroup), that p_nr = 2.0 is taken by both sides, and that the null
cases of the GPU file end in the interior."""
import numpy as np
import pytest

import mvfixcases as M
from test_oracle_mvlmm import harness  # noqa: F401  (fixture)

O = M.O
P_KEYS = ("p_wald", "p_lrt", "p_score")


def _claims(c, ref, a_mode):
    d = c["d"]
    for k in M.FIELDS:
        assert np.all(np.isfinite(ref[k])), k
    if a_mode != 3:  # mode 3 reports the null's V_g, V_e: the synthetic start
        assert M.min_eig(ref["Vg"], d) >= 1e-4 and M.min_eig(ref["Ve"], d) >= 1e-4


def _both_forms(harness, c, a_mode, crt, **kw):
    rt = M.harness_batch(harness, c, a_mode, crt, 0, **kw)
    if not kw.get("gxe"):
        fx = M.harness_batch(harness, c, a_mode, crt, 1, **kw)
        assert (fx is not None) == M.is_fixed(c["d"], c["cw"])  # the harness instantiates the library's table of fixed shapes
        if fx is not None:  # one source, two forms: the same bits
            for k in M.FIELDS:
                assert np.array_equal(fx[k], rt[k], equal_nan=True), k
    return rt


@pytest.mark.parametrize("d,cw,fixed", [(d, r - 1, True) for d, r in M.FIXED_SNP] + [(d, cw, False) for d, cw in M.RT_SNP])
def test_oracle_and_one_lane_agree_on_every_case(harness, d, cw, fixed):
    assert M.is_fixed(d, cw) == fixed
    c = M.case(d, cw)
    wv = M.waves(d, cw)
    assert c["l"] == 2 * wv + 1 and (wv == 1 or c["l"] % wv != 0)  # a ragged last workgroup wherever a workgroup holds several SNPs
    assert c["n"] % 64 in (3, 9) and c["n"] // 64 == 2            # three trips of the lane loop, the last nearly empty
    refs = {}
    for crt in (0, 1):
        ref = refs[crt] = M.reference(c, 4, crt)
        _claims(c, ref, 4)
        got = _both_forms(harness, c, 4, crt)
        w = M.worst_rel(got, ref)
        print("cpu d=%d cw=%d crt=%d seed=%d: oracle vs one lane %.2e" % (d, cw, crt, c["seed"], w))
        assert w <= M.CAP, (d, cw, crt, w)
    # every SNP took the Newton-Raphson branch (p_nr above every p value), so -crt moved every Wald and LRT p value; PCRT's score
    # mode maps the statistic to itself (src/mvlmm.cpp:2966-2967): that p value only goes through chisq_Qinv and back
    for k in ("p_wald", "p_lrt"):
        live = refs[0][k] < 1.0
        assert np.all(np.abs(refs[1][k] - refs[0][k])[live] > 1e-9 * refs[0][k][live]), k
    assert np.all(np.abs(refs[1]["p_score"] - refs[0]["p_score"]) <= 1e-9 * refs[0]["p_score"])
    assert np.all(refs[1]["Vg"] == refs[0]["Vg"])  # the estimates themselves do not depend on -crt


def test_p_nr_above_one_sends_every_snp_down_the_newton_branch(harness):
    """p_nr = 2.0 is accepted by both sides and differs from p_nr = 1.0 only where a p value is exactly 1 (non-positive
    statistic): same numbers on a case without one, and the branch taken on a SNP whose statistic is negative."""
    c = M.case(2, 1)
    for crt in (0, 1):
        a, b = M.reference(c, 4, crt), M.reference(c, 4, crt, p_nr=1.0)
        ha, hb = M.harness_batch(harness, c, 4, crt, 0), M.harness_batch(harness, c, 4, crt, 0, p_nr=1.0)
        assert max(a[k].max() for k in P_KEYS) < 1.0
        for k in M.FIELDS:
            assert np.array_equal(a[k], b[k]) and np.array_equal(ha[k], hb[k]), k


@pytest.mark.parametrize("d,cw", M.MODE_SHAPES)
@pytest.mark.parametrize("a_mode", [1, 2, 3])
def test_single_modes_agree(harness, d, cw, a_mode):
    c = M.case(d, cw)
    for crt in (0, 1):
        ref = M.reference(c, a_mode, crt)
        _claims(c, ref, a_mode)
        got = _both_forms(harness, c, a_mode, crt)
        w = M.worst_rel(got, ref)
        print("cpu d=%d cw=%d a_mode=%d crt=%d: oracle vs one lane %.2e" % (d, cw, a_mode, crt, w))
        assert w <= M.CAP, (d, cw, a_mode, crt, w)
        untouched = {1: ("p_lrt", "p_score"), 2: ("p_wald", "p_score"), 3: ("p_wald", "p_lrt")}[a_mode]
        for k in untouched:
            assert np.all(ref[k] == 0) and np.all(got[k] == 0), k


def test_stride_case_agrees(harness):
    """(2, 1) with l = 1030: the case that gives the run-time kernel more SNPs than it has workgroups (the run-time twins of the
    GPU file run the cases of the first test)."""
    assert all(M.is_fixed(d, cw) for d, cw in M.RT_TWINS)
    c = M.case(2, 1, l=1030, rt=True)
    assert c["l"] > 1024
    ref = M.reference(c, 4, 1)
    _claims(c, ref, 4)
    w = M.worst_rel(M.harness_batch(harness, c, 4, 1, 0), ref)
    print("cpu d=2 cw=1 l=%d: oracle vs one lane %.2e" % (c["l"], w))
    assert w <= M.CAP, w


@pytest.mark.parametrize("d,cw", M.GXE_SHAPES)
def test_gxe_cases_agree(harness, d, cw):
    c = M.case(d, cw, seed=M.GXE_SEEDS[(d, cw)], gxe=True)
    for crt in (0, 1):
        ref = M.reference(c, 4, crt, gxe=True)
        _claims(c, ref, 4)
        w = M.worst_rel(M.harness_batch(harness, c, 4, crt, 0, gxe=True), ref)
        print("cpu gxe d=%d cw=%d crt=%d seed=%d: oracle vs one lane %.2e" % (d, cw, crt, c["seed"], w))
        assert w <= M.CAP, (d, cw, crt, w)


@pytest.mark.parametrize("d,cw", M.FIXED_NULL + M.RT_NULL)
def test_null_cases_end_in_the_interior(d, cw):
    ref = M.null_reference(d, cw)
    lo = min(np.linalg.eigvalsh(ref[k]).min() for k in ("Vg_remle", "Ve_remle", "Vg_mle", "Ve_mle"))
    print("cpu null d=%d cw=%d: smallest eigenvalue %.2e" % (d, cw, lo))
    assert lo >= 1e-4
    c = M.null_case(d, cw)
    ev, W, Y = np.array(c["ev"]), np.array(c["UtW"]), np.array(c["UtY"])
    for func, tag in (("R", "remle"), ("L", "mle")):  # the two definitions the GPU file checks the fit against, on the oracle's own fit
        Vg, Ve, B = ref["Vg_" + tag], ref["Ve_" + tag], ref["B_" + tag]
        assert O.mph_em(func, 1, 0.0, ev, W, Y, Vg.copy(), Ve.copy(), B.copy()) == pytest.approx(ref["logl_" + tag], rel=1e-9)
        assert np.abs(M.gls_B(ev, W, Y, Vg, Ve) - B).max() < 1e-9 * np.abs(B).max()

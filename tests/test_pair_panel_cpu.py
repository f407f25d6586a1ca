"""The trait-pair panel on the CPU (tests/pairpanelcases.py): the composed reference against the oracle's own null block, the pair
body and the variance epilogue of gemma_amd/csrc/mvlmm_pair.hip.h / mvlmm.hip.h on one lane (tests/host/mvpair_harness.cpp) against
the composition, and the header / ABI mirrors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pairpanelcases as P

O = P.O
ROOT = os.path.join(P.HERE, "..")
NEW_SYMBOLS = ("gemma_hip_mvlmm_null_se", "gemma_hip_mvlmm_null_pairs", "gemma_hip_mvlmm_null_pairs_d")


@pytest.fixture(scope="module")
def pair_harness():
    return P.build_harness()


@pytest.mark.parametrize("cw,seed", P.CASES)
@pytest.mark.parametrize("fixed", [False, True])
def test_composition_is_the_oracles_null_block(cw, seed, fixed):
    """mph_initial + mph_em + mph_nr + numpy GLS reproduces O.mvlmm_null (d = 2) on every pair to 1e-12: the reference is valid"""
    c = P.case(cw)
    worst = 0.0
    for (i, j), ref in zip(P.PAIRS, P.reference(cw, fixed)):
        o = O.mvlmm_null(P.cfg_of(fixed), np.array(c["ev"]), np.array(c["UtW"]), np.ascontiguousarray(c["UtY"][[i, j]]))
        for tag in ("remle", "mle"):
            for k, r in (("Vg", o["Vg_" + tag]), ("Ve", o["Ve_" + tag]), ("B", o["B_" + tag]), ("logl", o["logl_" + tag])):
                worst = max(worst, float(np.abs(np.asarray(ref[tag][k]) - r).max() / np.abs(r).max()))
    print("composition vs O.mvlmm_null cw=%d fixed=%d: %.2e" % (cw, fixed, worst))
    assert worst <= 1e-12


@pytest.mark.parametrize("cw,seed", P.CASES)
def test_fixed_count_pairs_are_interior(cw, seed):
    lo_eig, lo_var = np.inf, np.inf
    for ref in P.reference(cw):
        for tag in ("remle", "mle"):
            b = ref[tag]
            lo_eig = min(lo_eig, np.linalg.eigvalsh(b["Vg"]).min(), np.linalg.eigvalsh(b["Ve"]).min())
            lo_var = min(lo_var, np.diag(b["VV"]).min(), b["VB"].min(), b["var_rg"], b["var_re"])
    print("cw=%d: smallest V eigenvalue %.3g, smallest variance %.3g" % (cw, lo_eig, lo_var))
    assert lo_eig >= 0.03 and lo_var > 0


@pytest.mark.parametrize("cw,seed", P.CASES)
def test_one_lane_matches_the_composition(pair_harness, cw, seed):
    """Fixed counts, all ten pairs: every field of both blocks, the new ones included, within CAP; status 0"""
    got, ref = P.harness_pairs(pair_harness, cw), P.reference(cw)
    worst = dict.fromkeys(P.BLOCK_FIELDS, 0.0)
    for g, r in zip(got, ref):
        assert g["status"] == 0
        for tag in ("remle", "mle"):
            for k, v in P.deviations(g[tag], r[tag]).items():
                worst[k] = max(worst[k], v) if v == v else v
    print("one lane vs composition cw=%d: " % cw + "  ".join("%s %.1e" % kv for kv in worst.items()))
    for k, v in worst.items():
        assert v <= P.CAP, (cw, k, v)


@pytest.mark.parametrize("d,cw", P.SE_SHAPES)
def test_general_epilogue_of_the_run_time_instance(pair_harness, d, cw):
    """(3, 2) and (2, 8) at NULL_N with the null seeds of mvfixcases: VV against mph_nr's matrix, VB against the numpy GLS; and the
    defaulted argument leaves `out` bit for bit what it is with the epilogue"""
    ref = P.se_reference(d, cw)
    out, se = P.harness_null_se(pair_harness, d, cw)
    out0, _ = P.harness_null_se(pair_harness, d, cw, with_se=False)
    assert np.array_equal(out, out0)
    v, blk, seb = d * (d + 1) // 2, 2 * d * d + d * cw + 1, pair_harness.mvp_null_se_doubles(d, cw)
    assert seb == 2 * v + d * cw + (18 if d == 2 else 0)
    for p, tag in enumerate(("remle", "mle")):
        r, s, o = ref[tag], se[p * seb:(p + 1) * seb], out[p * blk:(p + 1) * blk]
        for k, g, rr in (("VV", s[:2 * v], np.diag(r["VV"])), ("VB", s[2 * v:2 * v + d * cw], r["VB"].ravel()),
                         ("Vg", o[:d * d], r["Vg"].ravel()), ("B", o[2 * d * d:2 * d * d + d * cw], r["B"].ravel())):
            w = float(np.abs(g - rr).max() / np.abs(rr).max())
            print("epilogue d=%d cw=%d %s %s: %.1e" % (d, cw, tag, k, w))
            assert w <= P.CAP, (d, cw, tag, k, w)
        if d == 2:  # the two 3 x 3 blocks the correlations use
            cov = s[2 * v + d * cw:].reshape(2, 3, 3)
            for g, rr in ((cov[0], r["VV"][:3, :3]), (cov[1], r["VV"][3:, 3:])):
                assert np.abs(g - rr).max() <= P.CAP * np.abs(rr).max()


def test_correlation_of_a_bad_diagonal_is_nan(pair_harness):
    """a non-positive or non-finite diagonal gives NaN in r and var_r and status 1, not a trap: a trait whose start is NaN"""
    cw = 1
    c = P.case(cw)
    real = P.starts

    def poisoned(cc, cfg):
        s = real(cc, cfg)
        s[2, 6] = np.nan
        return s
    P.starts = poisoned
    try:
        got = P.harness_pairs(pair_harness, cw)
    finally:
        P.starts = real
    clean = P.harness_pairs(pair_harness, cw)
    for (i, j), g, k in zip(P.PAIRS, got, clean):
        if 2 in (i, j):
            assert g["status"] == 1 and np.isnan(g["remle"]["rg"]) and np.isnan(g["mle"]["var_re"])
        else:
            assert g["status"] == 0
            for tag in ("remle", "mle"):
                for f in P.BLOCK_FIELDS:
                    assert np.array_equal(g[tag][f], k[tag][f]), (i, j, tag, f)
    assert c["UtY"].shape == (P.T, P.N)


def test_header_and_python_mirrors():
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    lib = open(os.path.join(ROOT, "gemma_amd", "_lib.py")).read()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % s, hdr), s
        assert '"%s"' % s in lib, s
    assert re.search(r"^#define GEMMA_HIP_ABI_VERSION 4$", hdr, re.M)
    for s in ("gemma_mvpair_block", "gemma_mvpair_fit", "gemma_mvlmm_null_se"):
        assert re.search(r"\}\s*%s;" % s, hdr), s


def test_struct_sizes_match_the_header(tmp_path):
    """sizeof(gemma_mvpair_fit) / gemma_mvlmm_null_se as a C compiler sees the header equal the ctypes mirrors"""
    import subprocess
    from gemma_amd import _lib as L
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "gemma_hip.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(gemma_mvpair_fit), '
                   'sizeof(gemma_mvpair_block), sizeof(gemma_mvlmm_null_se)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    a, b, c = map(int, subprocess.check_output([str(exe)]).split())
    assert a == C.sizeof(L.MvPairFit) == C.sizeof(P.PairFit) == 288
    assert b == C.sizeof(L.MvPairBlock) == 136
    assert c == C.sizeof(L.MvNullSe)

"""The case lists of tests/gemmcases.py, checked without a GPU: the exactness bound of every case, numpy's own fp64 product against
the int64 reference, the launch plan each case claims against a restatement of launch_dgemm_t's conditions, the guard check's own
teeth, and numpy's fp64 product under the rounding bar that the GPU test uses."""
import numpy as np
import pytest

import gemmcases as gc


def test_every_case_is_exact_in_fp64():
    """K * 64 * |alpha| + |beta| * 64 < 2^53 and operands / C0 in range; numpy's fp64 matmul (any BLAS, any order) equals the int64
    reference bit for bit."""
    worst = 0
    products = {}  # per shape: numpy's fp64 op(A) op(B), from row-major and from transposed storage
    for c in gc.ALL_CASES:
        assert (c.alpha, c.beta) in gc.AB_PAIRS and c.K <= 1100 and gc.bound_ok(c), gc.case_id(c)
        opA, opB, C0, P = gc.exact_problem(c.M, c.N, c.K)
        if (c.M, c.N, c.K) not in products:
            assert opA.shape == (c.M, c.K) and opB.shape == (c.K, c.N) and C0.shape == (c.M, c.N)
            assert max(np.abs(opA).max(initial=0), np.abs(opB).max(initial=0)) <= 8
            assert np.abs(C0).max() <= 64 and not (C0 % 4).any()
            worst = max(worst, int(np.abs(P).max(initial=0)))
            A, B = opA.astype(np.float64), opB.astype(np.float64)
            products[(c.M, c.N, c.K)] = {"N": A @ B, "T": np.ascontiguousarray(A.T).T @ np.ascontiguousarray(B.T).T}
            for Pf in products[(c.M, c.N, c.K)].values():
                assert np.array_equal(Pf, P), gc.case_id(c)
        got = c.alpha * products[(c.M, c.N, c.K)][c.ta] + c.beta * C0.astype(np.float64)
        assert np.array_equal(got, gc.exact_reference(c)), gc.case_id(c)
    print("largest |sum| over the lists: %d" % worst)
    assert worst * 2 + 64 < 2 ** 18 < gc.SENTINEL and gc.SENTINEL * 8 % 2 == 1  # no result is the sentinel: an odd multiple of 1/8


def test_every_case_reaches_the_plan_it_claims():
    for c in gc.ALL_CASES:
        assert gc.case_plan(c) == c.plan, (gc.case_id(c), gc.case_plan(c))
        if c.layout.endswith("off") and c.layout != "c_off":
            assert c.routes == ("device",), gc.case_id(c)  # the host entry point stages operands to an aligned base


def test_every_plan_is_claimed_in_every_form():
    seen = {(c.plan.split("+")[0], c.ta + c.tb) for c in gc.ALL_CASES}
    inner = {(c.plan.split("+")[1], c.ta + c.tb) for c in gc.ALL_CASES if "+" in c.plan}
    for p in gc.PLANS:
        for ta, tb in gc.FORMS:
            assert (p, ta + tb) in seen, (p, ta + tb)
    for p in ("interior", "clamped", "strips"):  # what the first launch of a K-tail call can be
        for ta, tb in gc.FORMS:
            assert (p, ta + tb) in inner, (p, ta + tb)
    # the lists the switch children run (no side-stream group) still hold every plan but the side-stream one
    seen = {(c.plan.split("+")[0], c.ta + c.tb) for g in gc.EXACT_GROUPS.values() for c in g}
    assert {p for p, _ in seen} == set(gc.PLANS) - {"strips_side"}


def test_issue_shapes_are_in_the_lists():
    """The shapes that matter, spelled out once more: an edited list cannot drop one unnoticed."""
    def has(group, M, N, K, beta, forms=4):
        return len([c for c in gc.ALL_CASES if (c.group, c.M, c.N, c.K, c.beta) == (group, M, N, K, beta)]) >= forms
    for K in (16, 32, 48, 64, 80, 144):
        assert has("pipeline", 128, 128, K, 0.0) and has("pipeline", 128, 128, K, 0.25)
    for M, N in ((768, 384), (128, 1152), (1152, 128)):
        assert has("raster", M, N, 32, 0.0)
    for M, N in ((130, 258), (131, 258), (130, 259), (131, 259), (255, 129), (129, 129)):
        assert has("ragged", M, N, 48, 0.0) and has("ragged", M, N, 48, 0.25)
    for M, N in ((128, 128), (131, 259), (256, 130)):
        for K in (65, 79, 81):
            assert has("ktail", M, N, K, 0.0) and has("ktail", M, N, K, 0.25)
    assert has("ktail", 131, 259, 1031, 0.0) and has("ktail", 131, 259, 1031, 0.25)
    for M, N, K in ((127, 300, 64), (300, 127, 64), (128, 128, 63), (128, 128, 15), (200, 200, 1), (128, 130, 0)):
        assert has("checked", M, N, K, 0.0)
    assert {c.layout for c in gc.CHECKED if (c.M, c.N, c.K) == (256, 256, 64)} == {"a_off", "a_ld", "b_off", "b_ld", "c_off"}
    assert has("side", 4099, 2049, 48, 1.0) and has("side", 4100, 2050, 48, 0.0)


def test_plan_under_the_switches():
    """What the switches do to the plan: PIPE < 2 and CLAMP=0 turn the clamped plan into strips, SIDE_STREAM=0 keeps the strips on
    the caller's stream."""
    assert gc.plan("N", "T", 131, 259, 48, 0.0) == "clamped"
    assert gc.plan("N", "T", 131, 259, 48, 0.0, pipe=1) == "strips"
    assert gc.plan("N", "T", 131, 259, 48, 0.0, clamp=False) == "strips"
    assert gc.plan("N", "N", 4099, 2049, 48, 1.0) == "strips_side"
    assert gc.plan("N", "N", 4099, 2049, 48, 1.0, side_stream=False) == "strips"
    assert gc.plan("N", "N", 4095, 2049, 48, 1.0) == "strips"  # 31 x 16 complete tiles


def test_kinship_blocks_reach_the_syrk_branches():
    for n in gc.KIN_N:
        for blocks, kind in gc.KIN_BLOCKS.items():
            total = sum(blocks)
            assert total & (total - 1) == 0 and total * 64 < 2 ** 53
            for l in blocks:
                tail = "interior" if n % 128 == 0 else "strips"  # SYRK: a right strip, never a bottom one
                want = {"fast": tail, "ktail": "ktail+" + tail, "checked": "checked"}[kind]
                assert gc.kin_plan(n, l) == want, (n, l)
    n = max(gc.KIN_N)
    T = -(-n // 128)
    assert T == 11 and T * (T + 1) // 2 == 66
    G, S = gc.kin_problem(131, 128)
    assert np.array_equal(S, S.T) and np.array_equal((G.astype(np.float64) @ G.T.astype(np.float64)) / 128.0, S / 128.0)


def test_the_guard_check_bites():
    """check() on hand-made buffers: clean, one wrong entry, one unwritten entry, one guard element touched."""
    c = gc.Case("t", "N", "N", 5, 7, 3, 1.0, 0.0, "checked", "plain", gc.BOTH)
    opA, opB, C0, _ = gc.exact_problem(c.M, c.N, c.K)
    ref = gc.exact_reference(c)
    for route in gc.BOTH:
        (bA, oA, cA), (bB, oB, cB), (bC, r0, c0) = gc.build(c, route, opA, opB, C0)
        assert bC.shape == (c.M + 4, c.N + (3 if route == "host" else 4)) and np.all(bC == gc.SENTINEL)
        assert bA.shape[1] % 2 == 0 and np.array_equal(bA[:, oA:oA + cA], opA) and np.all(bA[:, oA + cA:] == gc.SENTINEL)
        assert len(gc.check(bC, r0, c0, ref, "x")) == 1  # nothing written: every entry is still the sentinel
        bC[r0:r0 + c.M, c0:c0 + c.N] = ref
        assert gc.check(bC, r0, c0, ref, "x") == []
        bC[r0 + 4, c0 + 6] += 0.25
        assert len(gc.check(bC, r0, c0, ref, "x")) == 1
        bC[r0 + 4, c0 + 6] = ref[4, 6]
        for i, j in ((r0 - 1, c0), (r0 + c.M, c0 + c.N - 1), (r0, c0 - 1), (r0 + c.M - 1, c0 + c.N), (0, 0)):
            old = bC[i, j]
            bC[i, j] = 0.0
            assert len(gc.check(bC, r0, c0, ref, "x")) == 1, (i, j)
            bC[i, j] = old
    odd = gc.build(c._replace(layout="a_ld"), "device", opA, opB, C0)[0][0]
    assert odd.shape[1] % 2 == 1
    assert gc.build(c._replace(layout="b_off"), "device", opA, opB, C0)[1][1] == 1


@pytest.mark.parametrize("shape", gc.ROUNDING_SHAPES)
def test_numpy_fp64_is_within_the_rounding_bar(shape):
    M, N, K = shape
    opA, opB, C0, _, _ = gc.rounding_problem(M, N, K)
    worst = 0.0
    for alpha, beta in gc.AB_PAIRS:
        worst = max(worst, gc.rounding_ratio(alpha * (opA @ opB) + beta * C0, M, N, K, alpha, beta))
    print("numpy fp64 at %s: worst |err| / bar = %.4f" % (shape, worst))
    assert worst <= 1.0
    # the bar is no blank cheque: one entry off by 2^-40 of its |op A| |op B| is 8192 / (K + 4) bars out
    bad = opA @ opB
    bad[3, 5] += 2.0 ** -40 * gc.rounding_problem(M, N, K)[4][3, 5]
    assert gc.rounding_ratio(bad, M, N, K, 1.0, 0.0) > 1.0

"""Case lists, exact references and the runner for the fp64 GEMM's dispatch tests (test_gemmcases_cpu.py, test_gpu_dgemm.py).

numpy only at import (torch is imported inside the device route), so the lists and references are checked without a GPU.

Exact reference.  Operands are integers in [-8, 8] held as doubles, C0 holds multiples of 4 in [-64, 64], (alpha, beta) is one
of (1, 0), (2, 1), (-0.5, 0.25).  With K <= 1100 every product, every partial sum in any order (FMA-contracted or not) and the
scaled result is an integer or a quarter-integer of magnitude < 2^18: the right answer is ONE bit pattern whatever the summation
order.  The reference is an int64 matmul scaled in integer arithmetic (units of 1/4); the comparison is np.array_equal.

Guards.  C is an interior view of a buffer with two guard rows above and below and guard columns left and right (ldc = N + 3 for
host arrays, N + 4 for device tensors), filled with SENTINEL -- an odd multiple of 1/8, which no result can be.  Operands live in
padded buffers too (even leading dimension unless the case asks for an odd one), the padding holds SENTINEL as well: a read
past a row's end shows in the result.  With beta == 0 the interior of C starts as SENTINEL, so an unwritten tile is a mismatch.

plan() restates the conditions of launch_dgemm_t (gemma_amd/csrc/dgemm_mfma.hip.h); every case carries the plan it is meant to
reach, written down by hand below, and test_gemmcases_cpu.py holds the two against each other.
"""
import collections
import functools

import numpy as np

FORMS = (("N", "N"), ("T", "N"), ("N", "T"), ("T", "T"))
AB_PAIRS = ((1.0, 0.0), (2.0, 1.0), (-0.5, 0.25))
AB0, AB1, ABQ = AB_PAIRS
SENTINEL = 2.0 ** 40 + 0.125
BM = BN = 128
BK = 16
PLANS = ("interior", "clamped", "strips", "strips_side", "ktail", "checked")

# layout: "plain" | "a_off" / "b_off" (operand view at an odd column offset: device tensors only -- the host entry point stages
# operands to a fresh, aligned device base) | "a_ld" / "b_ld" (odd leading dimension) | "c_off" (C at an odd column offset)
Case = collections.namedtuple("Case", "group ta tb M N K alpha beta plan layout routes")


def case_id(c):
    return "%s-%s%s-%dx%dx%d-a%g-b%g-%s" % (c.group, c.ta, c.tb, c.M, c.N, c.K, c.alpha, c.beta, c.layout)


# ----------------------------------------------------------------------------------------------------------- the launch plan
def plan(ta, tb, M, N, K, beta, aligned=True, syrk=False, pipe=2, clamp=True, side_stream=True):
    """Which branch of launch_dgemm_t a call takes.  "ktail" is returned as "ktail+<plan of the first floor(K/16)*16 of K>"."""
    a_km, b_kn = ta == "T", tb == "N"
    Tm, Tn = -(-M // BM), -(-N // BN)
    Fm, Fn = M // BM, N // BN
    if aligned and K > 4 * BK and K % BK != 0 and Fm > 0 and Fn > 0:
        return "ktail+" + plan(ta, tb, M, N, (K // BK) * BK, beta, aligned, syrk, pipe, clamp, side_stream)
    if not (aligned and K % BK == 0 and K > 0 and Fm > 0 and Fn > 0):
        return "checked"
    if (pipe >= 2 and not syrk and beta == 0.0 and (Tm > Fm or Tn > Fn) and clamp and (not a_km or M % 2 == 0)
            and (not b_kn or N % 2 == 0)):
        return "clamped"
    if not (Tn > Fn or (Tm > Fm and not syrk)):
        return "interior"
    return "strips_side" if side_stream and Fm * Fn >= 512 else "strips"


def case_aligned(c):
    return c.layout in ("plain", "c_off")


def case_plan(c, **switches):
    return plan(c.ta, c.tb, c.M, c.N, c.K, c.beta, aligned=case_aligned(c), **switches)


# ----------------------------------------------------------------------------------------------------------- the case lists
BOTH = ("host", "device")


def _all_forms(group, M, N, K, ab, plan_of, layout="plain", routes=BOTH):
    return [Case(group, ta, tb, M, N, K, ab[0], ab[1], plan_of if isinstance(plan_of, str) else plan_of[ta + tb], layout, routes)
            for ta, tb in FORMS]


def _pipeline():
    """The interior pipeline over 1, 2, 3, 4, 5 and 9 K-tiles: prologue alone, prologue + last, then 1, 2, 3 steady steps, beyond."""
    out = []
    for K in (16, 32, 48, 64, 80, 144):
        for ab in (AB0, ABQ):
            out += _all_forms("pipeline", 128, 128, K, ab, "interior")
    return out


def _raster():
    """Tile raster: 6 x 3 tiles (groups of 4 + 2 tile rows, 18 % 8 == 2), one tile row, one tile column (groups 4, 4, 1)."""
    out = []
    for M, N, K in ((768, 384, 32), (128, 1152, 32), (1152, 128, 32)):
        for ab in (AB0, AB1):
            out += _all_forms("raster", M, N, K, ab, "interior")
    return out


# beta == 0: the forms (TransA TransB) whose ragged tiles are clamped; the [k][m] operand of a shifted tile must stay 16-byte
# aligned: A^T needs an even M, B (untransposed) an even N.  Every other form takes the strip plan.
RAGGED_CLAMPED = {
    (130, 258): ("NN", "TN", "NT", "TT"),
    (131, 258): ("NN", "NT"),
    (130, 259): ("NT", "TT"),
    (131, 259): ("NT",),
    (255, 129): ("NT",),
    (129, 129): ("NT",),
    (256, 130): ("NN", "TN", "NT", "TT"),
}


def _beta0_plan(M, N):
    return {f: ("clamped" if f in RAGGED_CLAMPED[(M, N)] else "strips") for f in ("NN", "TN", "NT", "TT")}


def _ragged():
    """Ragged edges at K = 48: clamped or strips by parity with beta == 0, always right strip + bottom strip + corner otherwise."""
    out = []
    for M, N in ((130, 258), (131, 258), (130, 259), (131, 259), (255, 129), (129, 129)):
        out += _all_forms("ragged", M, N, 48, AB0, _beta0_plan(M, N))
        out += _all_forms("ragged", M, N, 48, ABQ, "strips")
    return out


def _ktail():
    """K tail: the last K % 16 columns by a second, bounds-checked launch with beta = 1 on top of the first."""
    out = []
    shapes = [(M, N, K) for (M, N) in ((128, 128), (131, 259), (256, 130)) for K in (65, 79, 81)] + [(131, 259, 1031)]
    for M, N, K in shapes:
        if (M, N) == (128, 128):
            p0, pq = "ktail+interior", "ktail+interior"
        else:
            p0 = {f: "ktail+" + p for f, p in _beta0_plan(M, N).items()}
            pq = "ktail+strips"
        out += _all_forms("ktail", M, N, K, AB0, p0)
        out += _all_forms("ktail", M, N, K, ABQ, pq)
    return out


def _checked():
    """Everything through the bounds-checked kernel: no complete tile in M or N, K < 64 and no multiple of 16, K == 0 (cblas: C =
    beta C), and (256, 256, 64) -- otherwise the fast path -- with an unaligned operand."""
    out = []
    for M, N, K in ((127, 300, 64), (300, 127, 64), (128, 128, 63), (128, 128, 15), (200, 200, 1)):
        for ab in (AB0, ABQ):
            out += _all_forms("checked", M, N, K, ab, "checked")
    for ab in AB_PAIRS:
        out += _all_forms("checked", 128, 130, 0, ab, "checked")
    for layout in ("a_off", "a_ld", "b_off", "b_ld"):
        for ab in (AB0, AB1):
            out += _all_forms("checked", 256, 256, 64, ab, "checked", layout, ("device",) if layout.endswith("off") else BOTH)
    for ab in (AB0, AB1):  # C's alignment is no condition of the fast path: its stores are scalar
        out += _all_forms("checked", 256, 256, 64, ab, "interior", "c_off", ("device",))
    return out


def _side():
    """At least 512 complete tiles: the strips go to the library's second stream (beta != 0), or ride clamped (beta == 0)."""
    return (_all_forms("side", 4099, 2049, 48, AB1, "strips_side", routes=("device",)) +
            _all_forms("side", 4100, 2050, 48, AB0, "clamped", routes=("device",)))


PIPELINE, RASTER, RAGGED, KTAIL, CHECKED, SIDE = _pipeline(), _raster(), _ragged(), _ktail(), _checked(), _side()
EXACT_GROUPS = {"pipeline": PIPELINE, "raster": RASTER, "ragged": RAGGED, "ktail": KTAIL, "checked": CHECKED}
ALL_CASES = PIPELINE + RASTER + RAGGED + KTAIL + CHECKED + SIDE

# SYRK through the kinship: n individuals, SNP blocks whose total is a power of two (kin_end's 1 / ns is then exact); the plan of
# each block's K += X^T X (form T,N, syrk, beta = 1).  n = 1300: 11 tile rows, 66 triangle tiles through the square-root index map.
KIN_N = (128, 131, 647, 1300)
KIN_BLOCKS = {(48, 80): "fast", (100, 156): "ktail", (40, 24): "checked"}


def kin_plan(n, l):
    return plan("T", "N", n, n, l, 1.0, aligned=True, syrk=True)


# rounding: real-valued operands against a long-double product
ROUNDING_SHAPES = ((131, 259, 79), (386, 259, 1031), (256, 256, 64))


# ----------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=8)
def exact_problem(M, N, K):
    """op(A) (M x K), op(B) (K x N), C0 (M x N) as int64 and P = op(A) op(B) in int64; the same for the four forms (a form only
    changes how the operand is stored).  Treat as read-only."""
    rng = np.random.default_rng([M, N, K, 20])
    opA = rng.integers(-8, 9, size=(M, K), dtype=np.int64)
    opB = rng.integers(-8, 9, size=(K, N), dtype=np.int64)
    C0 = 4 * rng.integers(-16, 17, size=(M, N), dtype=np.int64)
    P = opA @ opB
    for a in (opA, opB, C0, P):
        a.setflags(write=False)
    return opA, opB, C0, P


def exact_reference(c):
    """alpha op(A) op(B) + beta C0 exactly: integer arithmetic in units of 1/4, then one exact conversion and division by 4."""
    _, _, C0, P = exact_problem(c.M, c.N, c.K)
    a4, b4 = int(round(4 * c.alpha)), int(round(4 * c.beta))
    assert a4 == 4 * c.alpha and b4 == 4 * c.beta
    return (a4 * P + b4 * C0).astype(np.float64) / 4.0


def bound_ok(c):
    return c.K * 64 * abs(c.alpha) + abs(c.beta) * 64 < 2.0 ** 53


@functools.lru_cache(maxsize=4)
def rounding_problem(M, N, K):
    """Standard-normal op(A), op(B), C0; P = op(A) op(B) in long double and |op(A)| |op(B)| for the error bar.  Read-only."""
    rng = np.random.default_rng([M, N, K, 21])
    opA, opB, C0 = rng.standard_normal((M, K)), rng.standard_normal((K, N)), rng.standard_normal((M, N))
    P = opA.astype(np.longdouble) @ opB.astype(np.longdouble)
    absP = np.abs(opA) @ np.abs(opB)
    for a in (opA, opB, C0, P, absP):
        a.setflags(write=False)
    return opA, opB, C0, P, absP


def rounding_ratio(got, M, N, K, alpha, beta):
    """max over C of |got - ref| / bar with bar = (K + 4) 2^-53 (|alpha| |op A| |op B| + |beta| |C0|): the any-order dot-product bound
    (gamma_K, first order) plus the three roundings of the epilogue (alpha *, beta *, +).  Derived, not measured."""
    _, _, C0, P, absP = rounding_problem(M, N, K)
    ref = np.longdouble(alpha) * P + np.longdouble(beta) * C0.astype(np.longdouble)
    bar = (K + 4) * 2.0 ** -53 * (abs(alpha) * absP + abs(beta) * np.abs(C0))
    return float(np.max(np.abs(got.astype(np.longdouble) - ref) / bar))


@functools.lru_cache(maxsize=4)
def kin_problem(n, total):
    """n x total integer genotypes in [-8, 8] (individual-major: SNP j is column j, taken as already centred) and S = G G^T."""
    rng = np.random.default_rng([n, total, 22])
    G = rng.integers(-8, 9, size=(n, total), dtype=np.int64)
    S = G @ G.T
    G.setflags(write=False)
    S.setflags(write=False)
    return G, S


# ----------------------------------------------------------------------------------------------------------- the runner
def _even(x):
    return x + (x & 1)


def _operand(op, trans, off, odd_ld):
    """Padded host buffer and the slice of it that stores `op` (transposed when trans): (buffer, column offset, columns)."""
    S = np.ascontiguousarray(op.T if trans else op, dtype=np.float64)
    r, c = S.shape
    ld = _even(c) + 2 + (1 if odd_ld else 0)
    o = 1 if off else 0
    buf = np.full((r, ld), SENTINEL)
    buf[:, o:o + c] = S
    return buf, o, c


def build(c, route, opA, opB, C0):
    """Host buffers of one call: ((bufA, oA, cA), (bufB, oB, cB), (bufC, r0, c0)); C's interior holds C0, or SENTINEL for beta == 0."""
    A = _operand(opA, c.ta == "T", c.layout == "a_off", c.layout == "a_ld")
    B = _operand(opB, c.tb == "T", c.layout == "b_off", c.layout == "b_ld")
    if route == "host":
        ldc, c0 = c.N + 3, 1
    else:
        ldc, c0 = c.N + 4, (1 if c.layout == "c_off" else 2)
    bufC = np.full((c.M + 4, ldc), SENTINEL)
    if c.beta != 0.0:
        bufC[2:2 + c.M, c0:c0 + c.N] = C0
    return A, B, (bufC, 2, c0)


def check(bufC, r0, c0, ref, tag):
    """Mismatches of the interior against ref (bit for bit) and of every guard element against SENTINEL, as a list of strings."""
    M, N = ref.shape
    errs = []
    inner = bufC[r0:r0 + M, c0:c0 + N]
    if not np.array_equal(inner, ref):
        bad = np.argwhere(inner != ref)
        i, j = bad[0]
        errs.append("%s: %d of %d entries differ; rows %d..%d cols %d..%d; first at (%d, %d): got %r, want %r" % (
            tag, len(bad), M * N, bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(), i, j, inner[i, j], ref[i, j]))
    return errs + check_guards(bufC, r0, c0, M, N, tag)


def check_guards(bufC, r0, c0, M, N, tag):
    errs = []
    guard = np.ones(bufC.shape, dtype=bool)
    guard[r0:r0 + M, c0:c0 + N] = False
    hit = guard & (bufC.view(np.uint64) != np.float64(SENTINEL).view(np.uint64))
    if hit.any():
        i, j = np.argwhere(hit)[0]
        errs.append("%s: %d guard elements overwritten, first at buffer (%d, %d) = %r (C starts at (%d, %d))" % (
            tag, int(hit.sum()), i, j, bufC[i, j], r0, c0))
    return errs


def call(api, c, route, opA, opB, C0):
    """One GEMM through the public entry point; returns the whole C buffer (guards included) on the host, and where C lies in it."""
    (bA, oA, cA), (bB, oB, cB), (bC, r0, c0) = build(c, route, opA, opB, C0)
    if route == "host":
        api.fast_dgemm(c.ta, c.tb, c.alpha, bA[:, oA:oA + cA], bB[:, oB:oB + cB], c.beta, bC[r0:r0 + c.M, c0:c0 + c.N])
        return bC, r0, c0
    import torch
    dA, dB, dC = (torch.from_numpy(b).cuda() for b in (bA, bB, bC))
    api.fast_dgemm(c.ta, c.tb, c.alpha, dA[:, oA:oA + cA], dB[:, oB:oB + cB], c.beta, dC[r0:r0 + c.M, c0:c0 + c.N])
    return dC.cpu().numpy(), r0, c0


def run_exact(api, c, route):
    opA, opB, C0, _ = exact_problem(c.M, c.N, c.K)
    bufC, r0, c0 = call(api, c, route, opA, opB, C0)
    return check(bufC, r0, c0, exact_reference(c), case_id(c) + "-" + route)


def run_exact_list(api, cases):
    """Every case on every route it lists; the mismatches of all of them."""
    errs = []
    for c in cases:
        for route in c.routes:
            errs += run_exact(api, c, route)
    return errs

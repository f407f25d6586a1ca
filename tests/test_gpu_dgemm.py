"""The fp64 MFMA GEMM (gemma_amd/csrc/dgemm_mfma.hip.h) on every branch of launch_dgemm_t, in the four transpose forms, against an
exact reference -- runs on the MI355X box.  Cases, references and guards: tests/gemmcases.py (checked on the CPU by
tests/test_gemmcases_cpu.py, which also holds every case against the plan it claims).

Inputs are small integers, so the right C is one bit pattern whatever the summation order, and the comparison is np.array_equal
over the whole of C; C sits inside a sentinel-filled buffer whose every guard element is compared after the call.

Which group reaches which plan (N,N / T,N / N,T / T,T unless noted; "route" = host arrays and device tensors unless noted):

    group      shapes (M, N, K)                                     plan
    pipeline   (128, 128, 16 32 48 64 80 144), beta 0 / 0.25        interior: 1, 2, 3, 4, 5, 9 K-tiles of the LDS-DMA pipeline
    raster     (768, 384, 32) (128, 1152, 32) (1152, 128, 32)       interior: 18 tiles in groups of 4 + 2 rows; 9 tiles both ways
    ragged     (130|131, 258|259) (255, 129) (129, 129), K = 48     beta 0: clamped where the shifted [k][m] operand stays aligned
                                                                    (N,T always; N,N: N even; T,T: M even; T,N: both even), else
                                                                    strips; beta 0.25: strips (right, bottom, corner)
    ktail      (128, 128) (131, 259) (256, 130) x K 65 79 81,       ktail + interior / clamped / strips: the tail launch adds with
               (131, 259, 1031), beta 0 / 0.25                      beta = 1, so a lost or doubled tail is an integer error
    checked    (127, 300, 64) (300, 127, 64) (128, 128, 63 | 15),   checked (no complete tile; K < 64 off the K-tile; K == 0 is
               (200, 200, 1), (128, 130, 0); (256, 256, 64) with    C = beta C; unaligned A or B -- an odd column offset only
               A / B at an odd offset or odd ld, C at an odd offset as a device tensor, the host entry stages to an aligned base)
    side       (4099, 2049, 48) beta 1; (4100, 2050, 48) beta 0     strips_side (32 x 16 complete tiles); clamped at 33 x 17 tiles
               device tensors on a non-default stream
    kinship    n 128 131 647 1300, blocks 48+80 / 100+156 / 40+24   SYRK (T,N, beta 1) interior or right strip / K tail / checked;
                                                                    n = 1300: 66 triangle tiles through the square-root map
    rounding   (131, 259, 79) (386, 259, 1031) (256, 256, 64)       ktail + strips or clamped / the same / interior, real operands

GemmArgs::mirror, ::square_a and launch_dgemm_ksliced have no public route: they stay with the eigensolver's tests
(test_gpu_eigh.py).

The five GEMMA_HIP_GEMM_* switches are read once per process, so test_switches runs the exact lists in a fresh child per setting.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import gemmcases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", sorted(gc.EXACT_GROUPS))
def test_exact(gpu_api, group):
    t0 = time.time()
    errs = gc.run_exact_list(gpu_api, gc.EXACT_GROUPS[group])
    n = sum(len(c.routes) for c in gc.EXACT_GROUPS[group])
    print("dgemm exact[%s]: %d calls in %.2f s, %d mismatches" % (group, n, time.time() - t0, len(errs)))
    assert not errs, "\n".join(errs[:12])


def _upload_behind_a_kernel(buf):
    """The buffer reaches its values through a kernel queued on the current stream right before the GEMM (half the values are
    uploaded, then doubled in place -- exact): work that does not wait for the caller's stream reads the halves."""
    import torch
    d = torch.from_numpy(buf * 0.5).cuda()
    d.mul_(2.0)
    return d


@pytest.mark.parametrize("shape", [(4099, 2049), (4100, 2050)])
def test_side_stream(gpu_api, shape):
    """>= 512 complete tiles on a stream that is not the default one: with beta = 1 the strips run on the library's second stream
    between its `ready` and `done` events.  Operands and C0 are produced by kernels on the caller's stream just before the call
    (tests `ready`), column sums of C follow on that stream with no synchronisation (tests `done`)."""
    import torch
    cases = [c for c in gc.SIDE if (c.M, c.N) == shape]
    assert len(cases) == 4
    stream = torch.cuda.Stream()
    errs = []
    for c in cases:
        opA, opB, C0, _ = gc.exact_problem(c.M, c.N, c.K)
        ref = gc.exact_reference(c)
        (bA, oA, cA), (bB, oB, cB), (bC, r0, c0) = gc.build(c, "device", opA, opB, C0)
        with torch.cuda.stream(stream):
            dA, dB, dC = (_upload_behind_a_kernel(b) for b in (bA, bB, bC))
            Cv = dC[r0:r0 + c.M, c0:c0 + c.N]
            gpu_api.fast_dgemm(c.ta, c.tb, c.alpha, dA[:, oA:oA + cA], dB[:, oB:oB + cB], c.beta, Cv)
            colsum = Cv.sum(dim=0)
            got_sum = colsum.cpu().numpy()
            got = dC.cpu().numpy()
        tag = gc.case_id(c)
        errs += gc.check(got, r0, c0, ref, tag)
        want_sum = ref.sum(axis=0)  # integers below 2^26: exact in any order
        if not np.array_equal(got_sum, want_sum):
            errs.append("%s: column sums taken on the caller's stream differ in %d of %d columns, first %d" % (
                tag, int((got_sum != want_sum).sum()), c.N, int(np.flatnonzero(got_sum != want_sum)[0])))
        del dA, dB, dC, Cv, colsum
    assert not errs, "\n".join(errs[:12])


@pytest.mark.parametrize("blocks", sorted(gc.KIN_BLOCKS))
@pytest.mark.parametrize("n", gc.KIN_N)
def test_kinship_syrk_exact(gpu_api, n, blocks):
    """K = G G^T / ns through kin_begin / kin_add / kin_end: integer genotypes, ns a power of two -> K == S / ns bit for bit."""
    from gemma_amd import _lib as L
    total = sum(blocks)
    G, S = gc.kin_problem(n, total)
    Gf = G.astype(np.float64)
    gpu_api.kin_begin(n, 1)
    at = 0
    for l in blocks:
        gpu_api.kin_add(np.ascontiguousarray(Gf[:, at:at + l]), L.GENO_F64_IDV_MAJOR)
        at += l
    K = np.full((n, n), gc.SENTINEL)
    ns = gpu_api.kin_end(K)
    assert ns == total
    ref = S.astype(np.float64) / total
    bad = np.argwhere(K != ref)
    assert len(bad) == 0, "n=%d blocks=%s: %d entries differ, rows %d..%d cols %d..%d, first %s: %r vs %r" % (
        n, blocks, len(bad), bad[:, 0].min(), bad[:, 0].max(), bad[:, 1].min(), bad[:, 1].max(), bad[0], K[tuple(bad[0])],
        ref[tuple(bad[0])])
    assert np.array_equal(K, K.T)


@pytest.mark.parametrize("shape", gc.ROUNDING_SHAPES)
def test_rounding(gpu_api, shape):
    """Real-valued operands against a long-double product; entrywise bar (K + 4) 2^-53 (|alpha| |op A| |op B| + |beta| |C0|), the
    any-order dot-product bound plus the epilogue's three roundings (gemmcases.rounding_ratio).  Guards as everywhere."""
    M, N, K = shape
    opA, opB, C0, _, _ = gc.rounding_problem(M, N, K)
    worst, errs = 0.0, []
    for ta, tb in gc.FORMS:
        for alpha, beta in gc.AB_PAIRS:
            for route in gc.BOTH:
                c = gc.Case("rounding", ta, tb, M, N, K, alpha, beta, None, "plain", gc.BOTH)
                buf, r0, c0 = gc.call(gpu_api, c, route, opA, opB, C0)
                errs += gc.check_guards(buf, r0, c0, M, N, gc.case_id(c) + "-" + route)
                r = gc.rounding_ratio(np.ascontiguousarray(buf[r0:r0 + M, c0:c0 + N]), M, N, K, alpha, beta)
                if not r <= 1.0:
                    errs.append("%s-%s: |err| / bar = %.3g" % (gc.case_id(c), route, r))
                worst = max(worst, r)
    print("dgemm rounding %s: worst |err| / bar = %.4f" % (shape, worst))
    assert not errs, "\n".join(errs[:12])


# --------------------------------------------------------------------------------------------------------------- the switches
SWITCHES = [
    {"GEMMA_HIP_GEMM_PIPE": "1"},
    {"GEMMA_HIP_GEMM_PIPE": "0"},
    {"GEMMA_HIP_GEMM_PIPE": "0", "GEMMA_HIP_GEMM_WAVES": "8"},
    {"GEMMA_HIP_GEMM_CLAMP": "0"},
    {"GEMMA_HIP_GEMM_SIDE_STREAM": "0", "GEMMA_HIP_GEMM_GM": "3"},
]
# Per child.  Measured on an MI355X: the five exact lists (560 calls) took 0.35 s in the parent under the default switches (0.34 to
# 0.43 s in the children), a child needs 1.8 s from its first line to an initialised library (torch import included);
# 10 x lists + start-up = 5.3 s is below the floor of 60 s, so the floor holds.
MEASURED_LISTS_S = 0.35
MEASURED_STARTUP_S = 1.8
CHILD_TIMEOUT_S = max(60.0, 10 * MEASURED_LISTS_S + MEASURED_STARTUP_S)

_CHILD = """
import json
import sys
import time
t0 = time.time()
sys.path.insert(0, %r)
sys.path.insert(0, %r)
import gemmcases as gc
from gemma_amd import api
api.init(0, 0)
t1 = time.time()
errs, calls = {}, 0
for name in sorted(gc.EXACT_GROUPS):
    e = gc.run_exact_list(api, gc.EXACT_GROUPS[name])
    calls += sum(len(c.routes) for c in gc.EXACT_GROUPS[name])
    if e:
        errs[name] = [len(e)] + e[:8]
print("GEMMCASES " + json.dumps({"errors": errs, "calls": calls, "startup_s": t1 - t0, "lists_s": time.time() - t1}))
"""


def test_switches(gpu_api, tmp_path):
    """PIPE=1, PIPE=0, PIPE=0 + WAVES=8, CLAMP=0, SIDE_STREAM=0 + GM=3: a fresh process each (the switches are cached in statics), one
    after another; each runs the exact lists (no side-stream, no kinship group) and reports its mismatches as JSON.  A child that
    runs out of time, dies on a signal or exits 134 / 139 ends the test there: nothing more is started on the device."""
    script = tmp_path / "gemm_child.py"
    script.write_text(_CHILD % (ROOT, os.path.join(ROOT, "tests")))
    base = {k: v for k, v in os.environ.items() if not k.startswith("GEMMA_HIP_GEMM_")}
    n_calls = sum(len(c.routes) for g in gc.EXACT_GROUPS.values() for c in g)
    bad = []
    for sw in SWITCHES:
        tag = " ".join("%s=%s" % (k[len("GEMMA_HIP_GEMM_"):], v) for k, v in sorted(sw.items()))
        try:
            r = subprocess.run([sys.executable, str(script)], env=dict(base, **sw), capture_output=True, text=True,
                               timeout=CHILD_TIMEOUT_S)
        except subprocess.TimeoutExpired as e:
            out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
            err = e.stderr if isinstance(e.stderr, str) else (e.stderr or b"").decode(errors="replace")
            pytest.fail("[%s] no answer within %.0f s; no further child started\n%s\n%s" % (tag, CHILD_TIMEOUT_S, out[-2000:], err[-2000:]))
        if r.returncode < 0 or r.returncode in (134, 139):
            pytest.fail("[%s] child ended with status %d; no further child started\n%s\n%s" % (
                tag, r.returncode, r.stdout[-2000:], r.stderr[-2000:]))
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("GEMMCASES ")]
        if r.returncode != 0 or len(line) != 1:
            bad.append("[%s] exit %d\n%s\n%s" % (tag, r.returncode, r.stdout[-1000:], r.stderr[-2000:]))
            continue
        res = json.loads(line[0][len("GEMMCASES "):])
        print("dgemm switches [%s]: %d calls, start-up %.2f s, lists %.2f s, mismatching groups %s" % (
            tag, res["calls"], res["startup_s"], res["lists_s"], sorted(res["errors"])))
        if res["calls"] != n_calls:
            bad.append("[%s] ran %d calls, not %d" % (tag, res["calls"], n_calls))
        for name, e in res["errors"].items():
            bad.append("[%s] %s: %d mismatches\n  %s" % (tag, name, e[0], "\n  ".join(e[1:])))
    assert not bad, "\n".join(bad)

"""The plane read-back of the records kernel's plane-0 epilogue four steps ahead, the mask accumulators parked in LDS
(gemma_amd/csrc/i8gemm_sparse2_r16.hip.h, COMBINE: ep_fixed; GEMMA_HIP_I8_EPI_DEPTH, default 4) against the schedule with one step
in flight (GEMMA_HIP_I8_EPI_DEPTH=1): the Horner steps and their order are the same, only when the loads are issued differs, so
every U^T x entry and every SUMSTAT field must be the SAME BITS.  No tolerance anywhere in this file.

Cases and child process are those of tests/test_gpu_fused_epilogue.py (fresh child per switch value: the switch is read once per
setup); that file's own test holds the default to the separate combine."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_fused_epilogue as FE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# three planes (the deep body for nplanes 3), four planes (nplanes 4), plane 0 without mask accumulators, the complete-block pair,
# seven unfused planes (the generic body on both sides), short lists and a fix-up row behind the epilogue
NAMES = ("d7 fused", "d6 forced", "7g6m", "complete", "unfused", "miss5")
WANT = {"d7 fused": (7, 1), "d6 forced": (6, 1), "7g6m": (7, 1), "complete": (7, 1), "unfused": (7, 0), "miss5": (7, 1)}


def _child(out_path):
    from gemma_amd import api
    from gemma_amd import _lib as L
    api.init(0, verbose=0)
    res = {}
    switches = ("GEMMA_HIP_I8_DIGITS", "GEMMA_HIP_I8_FORM", "GEMMA_HIP_I8_FUSE", "GEMMA_HIP_I8_COMPLETE", "GEMMA_HIP_OVERLAP")
    for name in NAMES:
        ind, codes, U, ev, UtW, Uty, env = FE._case_data(name)
        raw = FE._pack(codes)
        for k in switches:
            os.environ.pop(k, None)
        os.environ.update(env)
        lmm = api.LMM(a_mode=1)
        lmm.setup(U, ev, UtW, Uty, plink=True)
        try:
            lmm.set_indicator(ind)
            res[name + "/utx"] = lmm.dbg_utx(raw, L.GENO_PLINK_2BIT, 1)
            assert api.last_utx_path() == 1
            res[name + "/stats"] = np.array(lmm.batch(raw, L.GENO_PLINK_2BIT)).view(np.float64)
            k = api.last_utx_kernel()
            res[name + "/info"] = np.array([k["variant"], k["digits"], k["fuse"], api.last_block_missing(), *FE._i8_post(L)], dtype=np.int64)
        finally:
            lmm.finish()
        for k in env:
            os.environ.pop(k, None)
    np.savez(out_path, **res)


@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = tmp_path_factory.mktemp("epidepth")
    out = {}
    for knob in ("1", "default"):
        env = dict(os.environ)
        env.pop("GEMMA_HIP_I8_EPI_DEPTH", None)
        if knob != "default":
            env["GEMMA_HIP_I8_EPI_DEPTH"] = knob
        env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
        path = str(d / ("depth_%s.npz" % knob))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, "child with GEMMA_HIP_I8_EPI_DEPTH=%s failed:\n%s\n%s" % (knob, r.stdout[-3000:], r.stderr[-3000:])
        with np.load(path) as z:
            out[knob] = {k: z[k] for k in z.files}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_deep_read_back_equals_one_step_ahead_bit_for_bit(sides, name):
    one, deep = sides["1"], sides["default"]
    variant, digits, fuse, anymiss, short_rows, long_rows, epi = (int(v) for v in deep[name + "/info"])
    from gemma_amd import _lib as L
    assert variant == L.UTX_KERNEL_RECORDS_R16 and epi == 1 and (digits, fuse) == WANT[name]
    assert list(one[name + "/info"]) == list(deep[name + "/info"])
    if name == "complete":
        assert anymiss == 0 and short_rows == 0 and long_rows == 0
    else:
        assert anymiss == 1
    if name == "miss5":  # a case that meets no dropped call proves nothing
        ind, codes, *_ = FE._case_data(name)
        d = FE.dropped_calls(codes, ind)
        assert short_rows == int(((d >= 1) & (d <= FE.SUR_MAX)).sum()) >= 20
        assert long_rows == int((d > FE.SUR_MAX).sum()) >= 1
    u0, u1 = one[name + "/utx"], deep[name + "/utx"]
    assert u0.shape == u1.shape and np.isfinite(u0).all() and np.abs(u0).max() > 0
    assert u0.tobytes() == u1.tobytes(), "U^T x differs in %d entries" % int((u0.view(np.uint64) != u1.view(np.uint64)).sum())
    s0, s1 = one[name + "/stats"], deep[name + "/stats"]
    assert np.isfinite(s0.reshape(-1, 8)[:, 0]).mean() > 0.9
    assert s0.tobytes() == s1.tobytes()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: %s --child OUT.npz" % sys.argv[0])

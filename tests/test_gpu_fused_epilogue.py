"""The digit combine as the epilogue of the records kernel's plane-0 launch (gemma_amd/csrc/i8gemm_sparse2_r16.hip.h, COMBINE;
GEMMA_HIP_I8_EPILOGUE, default 1) against the separate combine (GEMMA_HIP_I8_EPILOGUE=0): the operations and their order are the
same, so every U^T x entry and every SUMSTAT field must be the SAME BITS.  No tolerance anywhere in this file.

The switch is read once per setup, so each side runs in a fresh child process (this file run as a script); the children build the
same cases from the same seeds and the parent compares what they saved."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUR_MAX = 16  # gemma_amd/csrc/i8gemm.hip.h


def _pack(codes):
    p, ni = codes.shape
    pad = np.zeros((p, (ni + 3) // 4 * 4), dtype=np.uint8)
    pad[:, :ni] = codes
    return (pad[:, 0::4] | (pad[:, 1::4] << 2) | (pad[:, 2::4] << 4) | (pad[:, 3::4] << 6)).astype(np.uint8)


def _codes(rng, ni_total, p, miss):
    """PLINK 2-bit codes (01 = missing call), p SNPs x ni_total individuals"""
    return rng.choice([0, 1, 2, 3], size=(p, ni_total), p=[0.25, miss, 0.45 - miss, 0.3]).astype(np.uint8)


def dropped_calls(codes, ind):
    """Calls the 2:4 sparse mask operand drops, per SNP row: the analysed individuals in order, in groups of four; a group with more
    than two missing calls keeps its first two (tests/test_sparse_mask_words.py: encode)."""
    m = (codes[:, ind == 1] == 1).astype(np.int64)
    p, n = m.shape
    mp = np.zeros((p, (n + 3) // 4 * 4), dtype=np.int64)
    mp[:, :n] = m
    return np.maximum(mp.reshape(p, -1, 4).sum(axis=2) - 2, 0).sum(axis=1)


# name -> (seed, ni_total, p, drop, miss, environment).  Tiles are 256 SNP rows x 128 individuals.
CASES = {
    # 7 digits fused: 4 planes, plane 0 one digit wide; n % 4 != 0, l % 256 != 0
    "d7 fused": (11, 613, 257, 0.2, 0.01, {}),
    # 6 digits fused forced at a small n: 3 planes of two digits; l < 256
    "d6 forced": (12, 530, 200, 0.1, 0.01, {"GEMMA_HIP_I8_DIGITS": "6"}),
    # the strict form: plane 0 is the genotype product alone
    "7g6m": (13, 700, 300, 0.15, 0.01, {"GEMMA_HIP_I8_FORM": "7g6m"}),
    # one int32 plane per digit: seven planes, six of them read back
    "unfused": (14, 400, 130, 0.0, 0.02, {"GEMMA_HIP_I8_FUSE": "0"}),
    # no missing call among the analysed individuals: the complete-block pair, both digit forms
    "complete": (15, 520, 270, 0.1, 0.0, {}),
    "complete 7g6m": (16, 390, 100, 0.0, 0.0, {"GEMMA_HIP_I8_FORM": "7g6m"}),
    # the complete-block form off: both products whatever the block holds
    "complete off": (17, 520, 270, 0.1, 0.0, {"GEMMA_HIP_I8_COMPLETE": "0"}),
    # 5 % missing: about one row in five has a short list of dropped calls; row 5 is missing for most individuals (the fp64 fix-up)
    "miss5": (18, 2000, 300, 0.1, 0.05, {}),
    # row chunks on two streams: 2500 rows in chunks of 768, 768, 768, 196
    "chunked": (19, 640, 2500, 0.1, 0.03, {"GEMMA_HIP_OVERLAP": "1"}),
}
SEED_BIG = 20  # n = 16 403 >= 16 384: six digits by the library's own rule; n % 128 != 0, n % 4 != 0
N_BIG, P_BIG = 16403, 600


def _case_data(name):
    seed, ni_total, p, drop, miss, env = CASES[name]
    rng = np.random.default_rng(seed)
    ind = (rng.random(ni_total) > drop).astype(np.int32)
    codes = _codes(rng, ni_total, p, miss)
    if name == "miss5":
        codes[5, rng.random(ni_total) < 0.7] = 1
    n = int(ind.sum())
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    ev = np.sort(rng.random(n) * 2.0 + 0.05)
    y = rng.standard_normal(n)
    return ind, codes, U, ev, U.T @ np.ones((n, 1)), U.T @ y, env


def test_cases_meet_dropped_calls_of_both_kinds():
    """CPU: the seeds above give what the GPU test needs -- rows with 1 .. SUR_MAX dropped calls and a row with more in `miss5`,
    none at all in the complete blocks -- by the numpy restatement of the mask words."""
    from test_sparse_mask_words import encode
    ind, codes, *_ = _case_data("miss5")
    d = dropped_calls(codes, ind)
    assert ((d >= 1) & (d <= SUR_MAX)).sum() >= 20 and (d > SUR_MAX).sum() >= 1 and (d == 0).sum() >= 1
    m = (codes[:, ind == 1] == 1).astype(int)
    for s in (0, 5, 17):  # the vectorised count is encode()'s, 32 individuals at a time
        row = np.zeros((m.shape[1] + 31) // 32 * 32, dtype=int)
        row[:m.shape[1]] = m[s]
        assert sum(len(encode(row[o:o + 32])[2]) for o in range(0, len(row), 32)) == d[s]
    for name in ("complete", "complete 7g6m", "complete off"):
        ind, codes, *_ = _case_data(name)
        assert not (codes[:, ind == 1] == 1).any()
    ind, codes, *_ = _case_data("d7 fused")
    assert int(ind.sum()) % 4 != 0 and int(ind.sum()) % 128 != 0


# ------------------------------------------------------------------------------------------------ the child process
def _i8_post(L):
    a, b, e = C.c_long(), C.c_long(), C.c_int()
    L.check(L.lib().gemma_hip_dbg_last_i8_post(C.byref(a), C.byref(b), C.byref(e)), "dbg_last_i8_post")
    return a.value, b.value, e.value


def _child(out_path):
    import torch
    from gemma_amd import api
    from gemma_amd import _lib as L
    api.init(0, verbose=0)
    res = {}
    switches = ("GEMMA_HIP_I8_DIGITS", "GEMMA_HIP_I8_FORM", "GEMMA_HIP_I8_FUSE", "GEMMA_HIP_I8_COMPLETE", "GEMMA_HIP_OVERLAP")

    def run(name, ind, raw, U, ev, UtW, Uty, env, a_mode=1):
        for k in switches:
            os.environ.pop(k, None)
        os.environ.update(env)
        lmm = api.LMM(a_mode=a_mode)
        lmm.setup(U, ev, UtW, Uty, plink=True)
        try:
            if ind is not None:
                lmm.set_indicator(ind)
            res[name + "/utx"] = lmm.dbg_utx(raw, L.GENO_PLINK_2BIT, 1)
            assert api.last_utx_path() == 1
            res[name + "/stats"] = np.array(lmm.batch(raw, L.GENO_PLINK_2BIT)).view(np.float64)
            k = api.last_utx_kernel()
            res[name + "/info"] = np.array([k["variant"], k["digits"], k["fuse"], api.last_block_missing(), *_i8_post(L)], dtype=np.int64)
            if name == "d7 fused":  # the two-block pipe on the same state: three blocks, the middle one another block
                dev = torch.device("cuda", 0)
                blocks = [raw, raw[::-1].copy(), raw]
                plain = [np.array(lmm.batch(b, L.GENO_PLINK_2BIT)).view(np.float64) for b in blocks]
                tb = [torch.from_numpy(b).to(dev) for b in blocks]
                outs = [torch.zeros((b.shape[0], 8), dtype=torch.float64, device=dev) for b in blocks]
                for b, o in zip(tb, outs):
                    lmm.batch_pipe(b, L.GENO_PLINK_2BIT, o)
                lmm.pipe_flush()
                torch.cuda.synchronize()
                res["pipe/epilogue"] = np.array([_i8_post(L)[2]], dtype=np.int64)
                for i, (pl, o) in enumerate(zip(plain, outs)):
                    res["pipe/plain%d" % i] = pl
                    res["pipe/piped%d" % i] = o.cpu().numpy().reshape(-1)
        finally:
            lmm.finish()
        for k in env:
            os.environ.pop(k, None)

    for name in CASES:
        ind, codes, U, ev, UtW, Uty, env = _case_data(name)
        run(name, ind, _pack(codes), U, ev, UtW, Uty, env, a_mode=4 if name == "chunked" else 1)
    rng = np.random.default_rng(SEED_BIG)
    U = rng.standard_normal((N_BIG, N_BIG)) / np.sqrt(N_BIG)
    ev = np.sort(rng.random(N_BIG) * 2.0 + 0.05)
    y = rng.standard_normal(N_BIG)
    run("big", None, _pack(_codes(rng, N_BIG, P_BIG, 0.01)), U, ev, U.T @ np.ones((N_BIG, 1)), U.T @ y, {})
    np.savez(out_path, **res)


# ------------------------------------------------------------------------------------------------ the comparison
@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = tmp_path_factory.mktemp("epilogue")
    out = {}
    for knob in ("0", "1"):
        env = dict(os.environ)
        env["GEMMA_HIP_I8_EPILOGUE"] = knob
        env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
        path = str(d / ("knob%s.npz" % knob))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=1500)
        assert r.returncode == 0, "child with GEMMA_HIP_I8_EPILOGUE=%s failed:\n%s\n%s" % (knob, r.stdout[-3000:], r.stderr[-3000:])
        with np.load(path) as z:
            out[knob] = {k: z[k] for k in z.files}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES) + ["big"])
def test_epilogue_equals_the_separate_combine_bit_for_bit(sides, name):
    off, on = sides["0"], sides["1"]
    variant, digits, fuse, anymiss, short_rows, long_rows, epi = (int(v) for v in on[name + "/info"])
    from gemma_amd import _lib as L
    assert variant == L.UTX_KERNEL_RECORDS_R16
    # the two sides really are the two forms, on the same digit form
    assert epi == 1 and int(off[name + "/info"][6]) == 0
    assert list(off[name + "/info"][:6]) == list(on[name + "/info"][:6])
    want = {"d7 fused": (7, 1), "d6 forced": (6, 1), "7g6m": (7, 1), "unfused": (7, 0), "complete": (7, 1), "complete 7g6m": (7, 1),
            "complete off": (7, 1), "miss5": (7, 1), "chunked": (7, 1), "big": (6, 1)}[name]
    assert (digits, fuse) == want
    if name.startswith("complete"):
        assert anymiss == (-1 if name == "complete off" else 0) and short_rows == 0 and long_rows == 0
    elif name != "big":
        assert anymiss == 1
    if name == "miss5":  # a test that never meets a dropped call proves nothing: both kinds, and as many as numpy counts
        ind, codes, *_ = _case_data(name)
        d = dropped_calls(codes, ind)
        assert short_rows == int(((d >= 1) & (d <= SUR_MAX)).sum()) >= 20
        assert long_rows == int((d > SUR_MAX).sum()) >= 1
    u0, u1 = off[name + "/utx"], on[name + "/utx"]
    assert u0.shape == u1.shape and np.isfinite(u0).all() and np.abs(u0).max() > 0
    assert u0.tobytes() == u1.tobytes(), "U^T x differs in %d entries" % int((u0.view(np.uint64) != u1.view(np.uint64)).sum())
    s0, s1 = off[name + "/stats"], on[name + "/stats"]
    assert np.isfinite(s0.reshape(-1, 8)[:, 0]).mean() > 0.9 or name == "big"  # (big: U is not orthogonal, only equality matters)
    assert s0.tobytes() == s1.tobytes()


@pytest.mark.gpu
def test_pipe_keeps_the_separate_combine_and_equals_the_plain_batch(sides):
    """gemma_hip_lmm_batch_pipe_d has ONE U^T x buffer for two blocks in flight: its product must not write it, so it keeps the
    separate combine whatever the switch says -- and still gives the plain batch's records, which come from the epilogue."""
    for knob in ("0", "1"):
        r = sides[knob]
        assert int(r["pipe/epilogue"][0]) == 0
        for i in range(3):
            assert r["pipe/plain%d" % i].tobytes() == r["pipe/piped%d" % i].tobytes(), (knob, i)
    for i in range(3):
        assert sides["0"]["pipe/plain%d" % i].tobytes() == sides["1"]["pipe/plain%d" % i].tobytes()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: %s --child OUT.npz" % sys.argv[0])

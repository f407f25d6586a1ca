"""The left factor of a PLINK block straight from its 2-bit rows (gemma_amd/csrc/plink_records.hip.h: plink_records_kernel,
GEMMA_HIP_I8_DIRECT, default 1) against the byte matrix and the records built from it (GEMMA_HIP_I8_DIRECT=0: ingest_i8_kernel +
sparse2_meta_kernel): the records, the row means and the dropped-call counts are the same integers, so every U^T x entry and every
SUMSTAT field must be the SAME BITS.  No tolerance anywhere in this file.

The switch is read once per setup, so each side runs in a fresh child process (this file run as a script), as in
tests/test_gpu_fused_epilogue.py, whose case generators are used here."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_fused_epilogue import SUR_MAX, _codes, _i8_post, _pack, dropped_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> (seed, ni_total, p, drop, miss, environment).  drop = 0: no indicator is set, every individual is analysed -- the only
# form that takes the one-pass kernel.  Tiles are 256 SNP rows x 128 individuals, a .bed word is 16 calls, a row ni_total / 4 bytes.
CASES = {
    # n % 16 != 0, n % 128 != 0 (ragged last word, K padding); l % 256 = 1; 154 bytes a row: every other row off the 4-byte grid
    "n613 l257": (31, 613, 257, 0.0, 0.01, {}),
    # l < 256; 133 bytes a row: three rows in four take the byte-load branch; six digits forced
    "stride133 l200": (32, 530, 200, 0.0, 0.01, {"GEMMA_HIP_I8_DIGITS": "6"}),
    # no missing call at all: the any-missing flag must stay 0
    "nomiss": (33, 520, 270, 0.0, 0.0, {}),
    # 5 % missing, row 5 missing for most individuals: short lists and a fix-up row, read from the 2-bit rows
    "miss5": (34, 2000, 300, 0.0, 0.05, {}),
    # an indicator that drops individuals: the byte matrix is taken whatever the switch says
    "indicator": (35, 613, 257, 0.2, 0.01, {}),
    # row chunks on two streams: 2500 rows in chunks of 768, 768, 768, 196 -- the side stream's surplus kernels read the 2-bit rows
    "chunked": (36, 640, 2500, 0.0, 0.03, {"GEMMA_HIP_OVERLAP": "1"}),
    # the strict form: plane 0 is the genotype product alone
    "7g6m": (37, 700, 300, 0.0, 0.01, {"GEMMA_HIP_I8_FORM": "7g6m"}),
}
DIRECT = {name: c[3] == 0.0 for name, c in CASES.items()}


def _case_data(name):
    seed, ni_total, p, drop, miss, env = CASES[name]
    rng = np.random.default_rng(seed)
    ind = (rng.random(ni_total) > drop).astype(np.int32) if drop > 0 else None
    codes = _codes(rng, ni_total, p, miss)
    if name == "miss5":
        codes[5, rng.random(ni_total) < 0.7] = 1
    n = ni_total if ind is None else int(ind.sum())
    U = np.linalg.qr(rng.standard_normal((n, n)))[0]
    ev = np.sort(rng.random(n) * 2.0 + 0.05)
    y = rng.standard_normal(n)
    return ind, codes, U, ev, U.T @ np.ones((n, 1)), U.T @ y, env


def test_cases_are_the_shapes_the_kernel_can_go_wrong_at():
    """CPU: what the comments above promise, by numpy."""
    for name, (seed, ni, p, drop, miss, env) in CASES.items():
        ind, codes, *_ = _case_data(name)
        assert (ind is None) == DIRECT[name]
    assert 613 % 16 and 613 % 128 and 257 % 256 == 1 and 200 < 256
    assert ((530 + 3) // 4) % 4 != 0 and ((613 + 3) // 4) % 4 != 0  # row strides off the 4-byte grid
    _, codes, *_ = _case_data("nomiss")
    assert not (codes == 1).any()
    _, codes, *_ = _case_data("miss5")
    d = dropped_calls(codes, np.ones(codes.shape[1], dtype=np.int32))
    assert ((d >= 1) & (d <= SUR_MAX)).sum() >= 20 and (d > SUR_MAX).sum() >= 1 and (d == 0).sum() >= 1


# ------------------------------------------------------------------------------------------------ the child process
def _child(out_path):
    import torch
    from gemma_amd import api
    from gemma_amd import _lib as L
    api.init(0, verbose=0)
    api.profile_enable(True)
    res = {}
    switches = ("GEMMA_HIP_I8_DIGITS", "GEMMA_HIP_I8_FORM", "GEMMA_HIP_OVERLAP")
    for name in CASES:
        ind, codes, U, ev, UtW, Uty, env = _case_data(name)
        raw = _pack(codes)
        for k in switches:
            os.environ.pop(k, None)
        os.environ.update(env)
        lmm = api.LMM(a_mode=4 if name == "chunked" else 1)
        lmm.setup(U, ev, UtW, Uty, plink=True)
        try:
            if ind is not None:
                lmm.set_indicator(ind)
            res[name + "/utx"] = lmm.dbg_utx(raw, L.GENO_PLINK_2BIT, 1)
            assert api.last_utx_path() == 1
            api.profile_read(L.STAGE_INGEST, reset=True)
            res[name + "/stats"] = np.array(lmm.batch(raw, L.GENO_PLINK_2BIT)).view(np.float64)
            scopes = api.profile_read(L.STAGE_INGEST, reset=True)[1]  # timed scopes of the ingest stage: 1 = one pass, 2 = bytes + records
            k = api.last_utx_kernel()
            res[name + "/info"] = np.array([k["variant"], k["digits"], k["fuse"], api.last_block_missing(), *_i8_post(L), scopes],
                                           dtype=np.int64)
            if name == "n613 l257":  # the two-block pipe on the same state: three blocks, the middle one another block
                dev = torch.device("cuda", 0)
                blocks = [raw, raw[::-1].copy(), raw]
                plain = [np.array(lmm.batch(b, L.GENO_PLINK_2BIT)).view(np.float64) for b in blocks]
                tb = [torch.from_numpy(b).to(dev) for b in blocks]
                outs = [torch.zeros((b.shape[0], 8), dtype=torch.float64, device=dev) for b in blocks]
                for b, o in zip(tb, outs):
                    lmm.batch_pipe(b, L.GENO_PLINK_2BIT, o)
                lmm.pipe_flush()
                torch.cuda.synchronize()
                for i, (pl, o) in enumerate(zip(plain, outs)):
                    res["pipe/plain%d" % i] = pl
                    res["pipe/piped%d" % i] = o.cpu().numpy().reshape(-1)
        finally:
            lmm.finish()
        for k in env:
            os.environ.pop(k, None)
    np.savez(out_path, **res)


# ------------------------------------------------------------------------------------------------ the comparison
@pytest.fixture(scope="module")
def sides(tmp_path_factory):
    d = tmp_path_factory.mktemp("direct")
    out = {}
    for knob in ("0", "1"):
        env = dict(os.environ)
        env["GEMMA_HIP_I8_DIRECT"] = knob
        env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
        path = str(d / ("knob%s.npz" % knob))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, "child with GEMMA_HIP_I8_DIRECT=%s failed:\n%s\n%s" % (knob, r.stdout[-3000:], r.stderr[-3000:])
        with np.load(path) as z:
            out[knob] = {k: z[k] for k in z.files}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_one_pass_records_equal_the_byte_matrix_bit_for_bit(sides, name):
    off, on = sides["0"], sides["1"]
    variant, digits, fuse, anymiss, short_rows, long_rows, epi, scopes = (int(v) for v in on[name + "/info"])
    from gemma_amd import _lib as L
    assert variant == L.UTX_KERNEL_RECORDS_R16
    # the two sides really are the two forms: one timed ingest scope against two (bytes, then records) -- unless an indicator is set
    assert int(off[name + "/info"][7]) == 2 and scopes == (1 if DIRECT[name] else 2)
    # same kernel, digit form, any-missing flag, short and long rows, epilogue
    assert list(off[name + "/info"][:7]) == list(on[name + "/info"][:7])
    assert (digits, fuse, epi) == ((6, 1, 1) if name == "stride133 l200" else (7, 1, 1))
    assert anymiss == (0 if name == "nomiss" else 1)
    if name == "nomiss":
        assert short_rows == 0 and long_rows == 0
    if name == "miss5":  # a case that meets no dropped call proves nothing: both kinds, and as many as numpy counts
        _, codes, *_ = _case_data(name)
        d = dropped_calls(codes, np.ones(codes.shape[1], dtype=np.int32))
        assert short_rows == int(((d >= 1) & (d <= SUR_MAX)).sum()) >= 20
        assert long_rows == int((d > SUR_MAX).sum()) >= 1
    u0, u1 = off[name + "/utx"], on[name + "/utx"]
    assert u0.shape == u1.shape and np.isfinite(u0).all() and np.abs(u0).max() > 0
    assert u0.tobytes() == u1.tobytes(), "U^T x differs in %d entries" % int((u0.view(np.uint64) != u1.view(np.uint64)).sum())
    s0, s1 = off[name + "/stats"], on[name + "/stats"]
    assert np.isfinite(s0.reshape(-1, 8)[:, 0]).mean() > 0.9
    assert s0.tobytes() == s1.tobytes()


@pytest.mark.gpu
def test_pipe_equals_the_plain_batch_on_both_sides(sides):
    """gemma_hip_lmm_batch_pipe_d keeps the byte matrix (its caller may overwrite a block before the block's surplus kernels run) and
    gives the plain batch's records, which come from the one-pass kernel on side 1."""
    for knob in ("0", "1"):
        r = sides[knob]
        for i in range(3):
            assert r["pipe/plain%d" % i].tobytes() == r["pipe/piped%d" % i].tobytes(), (knob, i)
    for i in range(3):
        assert sides["0"]["pipe/plain%d" % i].tobytes() == sides["1"]["pipe/plain%d" % i].tobytes()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        sys.exit("usage: %s --child OUT.npz" % sys.argv[0])

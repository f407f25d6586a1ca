"""The refinement of the score panel's hits (gemma_hip_lmm_score_panel_refine_*, _hits_refine_batch; LMM.setup_score_refine /
assoc_score_refine / refine_last, batch_score_panel_hits(refine=True), AnalyzeScorePanelHits(refine=True)) on the MI355X.

1. Bits.  For every pair the eight fields of refine_assoc_d equal row `snp` of the single-phenotype path the project already pins
   (tests/test_gpu_lmm_definition.py, tests/test_gpu_parity.py): gemma_hip_lmm_setup_d with a_mode 4, the same grid, plink_nan_rule
   0, column t of UtY and the trait's null fit, then gemma_hip_lmm_assoc_d on the same UtX, with GEMMA_HIP_ASSOC_GRID=0 in the
   environment of that setup.  Shapes and lists: tests/scorerefinecases.py.
2. The ways in agree: refine_last_d after hits_batch_d with refine_assoc_d on dbg_utx of the block, the host form with refine_last_d
   of its own list, AnalyzeScorePanelHits(refine=True) over two blocks with the per-block calls.
3. The definition (tests/lmmdefcases.py), through test_gpu_lmm_definition._check: its BAR, P_BAR, lambda_criteria, RATIO_MIN and
   LEFT_OUT_MAX on a sample of pairs of (65, 3, 17) and (203, 6, 4).
4. State and argument errors.
Not here: a refine_setup whose T x n copy cannot fit (GEMMA_HIP_ENOMEM with the byte count) -- T is the score-panel setup's, and a
setup whose transposed panel exceeds the free memory cannot be reached without allocating towards exhaustion.

Observed on an MI355X: every list of every shape in bits; the sampled pairs against the definition beta 2.9e-14, se 4.8e-15, logl_H1
9.3e-15, p_wald 1.9e-13, p_lrt 3.8e-14, p_score 1.9e-13, interior lambda-hats at most 6.6e-6 from the maximiser, nothing left out."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import lmmdefcases as D
import scorehitcases as sh
import scorerefinecases as R
import test_gpu_lmm_definition as G

pytestmark = pytest.mark.gpu
_REF, _NULLS = {}, {}


def _dev(a):
    import torch
    return torch.tensor(np.array(a), dtype=torch.float64, device="cuda")


@contextlib.contextmanager
def _env(**kv):
    saved = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _forced(forced):
    return _env(GEMMA_HIP_FORCE_GENERIC="1") if forced else contextlib.nullcontext()


def _nulls(api, oracle, n, c, T):
    """(l_mle_null, logl_mle_H0) of the panel's T traits: the device's own null fits"""
    key = (n, c, T)
    if key not in _NULLS:
        p = R.panel(oracle, n, c, T)
        fit = api.CalcLambdaNullPanel(p["ev"], p["UtW"], p["UtY"])
        _NULLS[key] = (fit["l_mle_null"].copy(), fit["logl_mle_H0"].copy())
    return _NULLS[key]


def _reference(api, oracle, n, c, T, t, forced=False):
    """(L_ROWS, 8) records of the single-phenotype streaming path on trait t, computed once"""
    import torch
    key = (n, c, T, t, forced)
    if key not in _REF:
        p = R.panel(oracle, n, c, T)
        lam, logl = _nulls(api, oracle, n, c, T)
        with _env(GEMMA_HIP_ASSOC_GRID="0"), _forced(forced):
            lmm = api.LMM(a_mode=4, l_mle_null=float(lam[t]), logl_mle_H0=float(logl[t]))
            lmm.setup(_dev(p["U"]), _dev(p["ev"]), _dev(p["UtW"]), _dev(p["UtY"][:, t]))
            try:
                out = lmm.assoc(_dev(p["UtX"]))
                torch.cuda.synchronize()
                out = out.cpu().numpy()
            finally:
                lmm.finish()
        out.setflags(write=False)
        _REF[key] = out
    return _REF[key]


@contextlib.contextmanager
def _refine(api, oracle, n, c, T, forced=False):
    """a score-panel setup of the panel with its refinement, on device tensors -> (lmm, UtX on the device)"""
    p = R.panel(oracle, n, c, T)
    lam, logl = _nulls(api, oracle, n, c, T)
    with _forced(forced):
        lmm = api.LMM(a_mode=3)
        UtY_d = _dev(p["UtY"])
        lmm.setup_score_panel(_dev(p["U"]), _dev(p["ev"]), _dev(p["UtW"]), UtY_d, lam)
        try:
            lmm.setup_score_refine(UtY_d, logl)
            yield lmm, _dev(p["UtX"])
        finally:
            lmm.finish()


def _want(api, oracle, n, c, T, pairs, forced=False):
    return np.stack([_reference(api, oracle, n, c, T, int(t), forced)[int(s)] for s, t in pairs])


def _pairs_t(pairs):
    import torch
    return torch.tensor(np.asarray(pairs), dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. bits
@pytest.mark.parametrize("n,c,T,forced", [s + (False,) for s in R.SHAPES] + [R.FORCED + (True,)])
def test_refined_pairs_equal_the_single_phenotype_streaming_path(gpu_api, oracle, n, c, T, forced):
    """m = 1, m = 5 (ragged workgroup, monomorphic and all-missing rows), reversed order, a repeated pair, all T * l pairs at
    (31, 1, 5), U^T x with ld = n and with an odd ld > n; one out-of-range pair (snp = l, pheno = T, both 2^32 - 1) among valid
    ones: its record is NaN, its neighbours' are what they were"""
    import torch
    lists = R.pair_lists(n, c, T)
    for t in range(T):  # before the score-panel setup: a single-phenotype setup would take its place
        _reference(gpu_api, oracle, n, c, T, t, forced)
    with _refine(gpu_api, oracle, n, c, T, forced) as (lmm, UtX):
        wide = torch.full((R.L_ROWS, n + 5), float("nan"), dtype=torch.float64, device="cuda")
        wide[:, :n] = UtX
        seen_finite = 0
        for name, pairs in lists.items():
            want = _want(gpu_api, oracle, n, c, T, pairs, forced)
            for tag, X in (("ld = n", UtX), ("ld = n + 5", wide[:, :n])):
                got = lmm.assoc_score_refine(X, _pairs_t(pairs)).cpu().numpy()
                assert got.shape == (len(pairs), 8)
                assert sh.same_bits(got, want), (name, tag, np.flatnonzero((got.view(np.uint64) != want.view(np.uint64)).any(axis=1))[:8])
            ordinary = pairs[:, 0] < R.MONO
            assert np.isfinite(want[ordinary]).all(), name  # every ordinary pair has a whole record
            seen_finite += int(ordinary.sum())
        assert seen_finite >= 20
        # a ScoreHitsDev goes in as the (m, 2) tensor does
        pairs = lists["five"]
        h = gpu_api.ScoreHitsDev(_pairs_t(pairs[:, 0]), _pairs_t(pairs[:, 1]), torch.zeros((5, 3), dtype=torch.float64, device="cuda"))
        assert sh.same_bits(lmm.assoc_score_refine(UtX, h).cpu().numpy(), _want(gpu_api, oracle, n, c, T, pairs, forced))
        # out of range
        base = lists["repeated"]
        clean = _want(gpu_api, oracle, n, c, T, base, forced)
        for bad in ((R.L_ROWS, 0), (0, T), (2 ** 32 - 1, 2 ** 32 - 1)):
            for at in (0, 3, len(base)):
                pairs = np.insert(base, at, bad, axis=0)
                got = lmm.assoc_score_refine(UtX, _pairs_t(pairs)).cpu().numpy()
                assert np.isnan(got[at]).all(), (bad, at, got[at])
                assert sh.same_bits(np.delete(got, at, axis=0), clean), (bad, at)


def test_the_lists_reach_every_branch_of_the_record(gpu_api, oracle):
    """over the reference records the lists are compared with: lambda-hats inside the grid and at both ends, p-values from near 1 to
    below 1e-100, NaN on the all-missing row, and pairs of one SNP that differ between phenotypes"""
    lam, p = [], []
    for n, c, T in R.SHAPES:
        for t in range(T):
            ref = _reference(gpu_api, oracle, n, c, T, t)
            assert np.isnan(ref[R.MISSING]).any()
            lam.append(ref[:R.MONO, 2:4].ravel())
            p.append(ref[:R.MONO, 4:7].ravel())
        a, b = _reference(gpu_api, oracle, n, c, T, 0), _reference(gpu_api, oracle, n, c, T, T - 1)
        assert not sh.same_bits(a[:R.MONO], b[:R.MONO])
    lam, p = np.concatenate(lam), np.concatenate(p)
    inside = (lam > 1e-5) & (lam < 1e5)
    print("lambda-hat inside %d, at l_min %d, at l_max %d; p from %.3g to %.3g" % (inside.sum(), (lam == 1e-5).sum(), (lam == 1e5).sum(),
                                                                                   p.min(), p.max()))
    assert inside.sum() >= 100 and (lam == 1e-5).sum() >= 10 and (lam == 1e5).sum() >= 10
    assert 0 < p.min() < 1e-100 and p.max() > 0.5


# ------------------------------------------------------------------------------------------------ 2. the ways in agree
def _plink_block():
    """24 rows of scorehitcases.plink_panel(3, 17): 22 of its SNPs, a monomorphic row (every call 0) and an all-missing row"""
    raw, U, ev, UtW, UtY, ind = sh.plink_panel(3, 17)
    blk = np.ascontiguousarray(raw[:R.L_ROWS]).copy()
    blk[R.MONO] = 0xFF     # code 11 four times: genotype 0
    blk[R.MISSING] = 0x55  # code 01 four times: missing
    return blk, U, ev, UtW, UtY, ind


P_MAX = 0.2


@contextlib.contextmanager
def _plink_refine(api):
    blk, U, ev, UtW, UtY, ind = _plink_block()
    fit = api.CalcLambdaNullPanel(ev, UtW, UtY)
    lam, logl = fit["l_mle_null"].copy(), fit["logl_mle_H0"].copy()
    lmm = api.LMM(a_mode=3)
    lmm.setup_score_panel(U, ev, UtW, UtY, lam)
    try:
        lmm.set_indicator(ind)
        lmm.setup_score_refine(UtY, logl)
        yield lmm, blk, (U, ev, UtW, UtY, ind, lam, logl)
    finally:
        lmm.finish()


def test_refine_last_equals_refine_assoc_on_the_blocks_utx(gpu_api):
    import torch
    from gemma_amd import _lib as L
    with _plink_refine(gpu_api) as (lmm, blk, _):
        hits, _ = lmm.batch_score_panel_hits(torch.from_numpy(blk).cuda(), L.GENO_PLINK_2BIT, P_MAX)
        assert len(hits.snp) >= 30 and not bool(((hits.snp == R.MONO) | (hits.snp == R.MISSING)).any())
        last = lmm.refine_last(hits).cpu().numpy()
        # the records form leaves its U^T x behind as well
        lmm.batch_score_panel(torch.from_numpy(blk).cuda(), L.GENO_PLINK_2BIT)
        again = lmm.refine_last(hits).cpu().numpy()
        UtX = lmm.dbg_utx(blk, L.GENO_PLINK_2BIT, 1)
        assoc = lmm.assoc_score_refine(_dev(UtX), hits).cpu().numpy()
        assert np.isfinite(last).all()
        assert sh.same_bits(last, assoc) and sh.same_bits(again, assoc)
        # p_score, beta and se are those of the -lmm 4 body: the Wald ones, not copies of the hit's
        assert not np.array_equal(last[:, 0], hits.stats[:, 0].cpu().numpy())
        # the degenerate rows through the block's own U^T x: records, whatever they hold, and the neighbours untouched
        extra = lmm.assoc_score_refine(_dev(UtX), _pairs_t([[R.MONO, 3], [int(hits.snp[0]), int(hits.pheno[0])], [R.MISSING, 5]])).cpu().numpy()
        assert sh.same_bits(extra[1], assoc[0])


def test_host_form_equals_refine_last_of_its_own_list(gpu_api):
    from gemma_amd import _lib as L
    with _plink_refine(gpu_api) as (lmm, blk, _):
        hits, best, refined = lmm.batch_score_panel_hits(blk, L.GENO_PLINK_2BIT, P_MAX, refine=True)
        plain, best0 = lmm.batch_score_panel_hits(blk, L.GENO_PLINK_2BIT, P_MAX)
        assert sh.same_bits(hits, plain) and sh.same_bits(best, best0)
        assert refined.dtype == gpu_api.SUMSTAT_DTYPE and len(refined) == len(hits) >= 30
        pairs = np.column_stack([hits["snp"].astype(np.int64), hits["pheno"].astype(np.int64)])
        last = lmm.refine_last(_pairs_t(pairs)).cpu().numpy()
        assert sh.same_bits(refined.view(np.float64).reshape(-1, 8), last)
        # a list shorter than the hits: the mirror repeats the block, the records follow
        h2, _, r2 = lmm.batch_score_panel_hits(blk, L.GENO_PLINK_2BIT, P_MAX, cap=7, refine=True)
        assert sh.same_bits(h2, hits) and sh.same_bits(r2, refined)
        # no hit: nothing to refine
        h0, _, r0 = lmm.batch_score_panel_hits(blk, L.GENO_PLINK_2BIT, 0.0, refine=True)
        assert len(h0) == 0 and len(r0) == 0


def test_analyze_with_refine_over_two_blocks_equals_the_per_block_calls(gpu_api):
    import torch
    from gemma_amd import _lib as L
    with _plink_refine(gpu_api) as (lmm, blk, (U, ev, UtW, UtY, ind, lam, logl)):
        parts = []
        for s0 in (0, 16):
            h, _, r = lmm.batch_score_panel_hits(np.ascontiguousarray(blk[s0:s0 + 16]), L.GENO_PLINK_2BIT, P_MAX, refine=True)
            h = h.copy()
            h["snp"] += s0
            parts.append((h, r))
    hits = np.concatenate([h for h, _ in parts])
    refined = np.concatenate([r for _, r in parts])
    order = np.lexsort((hits["snp"], hits["pheno"]))
    hits, refined = hits[order], refined[order]
    assert len(hits) >= 30 and (hits["snp"] >= 16).any() and (hits["snp"] < 16).any()
    a = gpu_api.LMM(a_mode=3)
    got = a.AnalyzeScorePanelHits(U, ev, UtW, UtY, blk, L.GENO_PLINK_2BIT, P_MAX, indicator_idv=ind, l_mle_null=lam, batch=16, refine=True,
                                  logl_mle_H0=logl)
    assert len(got) == 3 and a.scoreRefined is got[2]
    assert sh.same_bits(got[0], hits) and sh.same_bits(got[2], refined)
    # missing nulls are fitted by CalcLambdaNullPanel: the same fits, the same bits
    fitted = gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(U, ev, UtW, UtY, blk, L.GENO_PLINK_2BIT, P_MAX, indicator_idv=ind, batch=16, refine=True)
    assert sh.same_bits(fitted[0], hits) and sh.same_bits(fitted[2], refined)
    # the default leaves today's return values
    plain = gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(U, ev, UtW, UtY, blk, L.GENO_PLINK_2BIT, P_MAX, indicator_idv=ind, l_mle_null=lam, batch=16)
    assert len(plain) == 2 and sh.same_bits(plain[0], hits)
    # device tensors in, device tensors out
    dev = torch.device("cuda")
    Ud, evd, UtWd, UtYd = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (U, ev, UtW, UtY))
    t = gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(Ud, evd, UtWd, UtYd, torch.from_numpy(blk).to(dev), L.GENO_PLINK_2BIT, P_MAX,
                                                    indicator_idv=ind, l_mle_null=lam, batch=16, refine=True, logl_mle_H0=logl)
    assert t[2].is_cuda and sh.same_bits(sh.hits_of_dev(t[0]), hits)
    assert sh.same_bits(t[2].cpu().numpy(), refined.view(np.float64).reshape(-1, 8))


# ------------------------------------------------------------------------------------------------ 3. the definition
@pytest.mark.parametrize("n,c,T", R.DEF_SHAPES)
def test_sampled_pairs_against_the_definition(gpu_api, oracle, n, c, T):
    """the pairs of scorerefinecases.def_sample on the case's three traits, held as tests/test_gpu_lmm_definition.py holds a mode 4
    block of the per-SNP stage (its _check: BAR, P_BAR, lambda_criteria, RATIO_MIN, LEFT_OUT_MAX of tests/lmmdefcases.py)"""
    sample = R.def_sample(n, c, T)
    p = R.panel(oracle, n, c, T)
    lam, logl = _nulls(gpu_api, oracle, n, c, T)
    pairs = np.concatenate([np.column_stack([rows, np.full(len(rows), t)]) for t, rows in sample.items()])
    with _refine(gpu_api, oracle, n, c, T) as (lmm, UtX):
        got = lmm.assoc_score_refine(UtX, _pairs_t(pairs)).cpu().numpy()
    at = 0
    for t, rows in sample.items():
        null = G._null(gpu_api, oracle, n, c, t, "default")  # what _check reads; the panel's fit of the trait is the single fit's
        assert null["l_mle_null"] == lam[t] and null["logl_mle_H0"] == logl[t]
        idx = p["rows"][rows]  # rows of the case behind the panel's
        score = G._run(gpu_api, oracle, n, c, t, 3)[idx]
        G._check(oracle, n, c, t, 4, got[at:at + len(rows)], tag="refined pairs", idx=idx, score_out=score)
        at += len(rows)


# ------------------------------------------------------------------------------------------------ 4. state and argument errors
def _p(t):
    return C.c_void_p(t.data_ptr())


def test_state_and_argument_errors(gpu_api, oracle):
    import torch
    from gemma_amd import _lib as L
    lib = L.lib()
    n, c, T = R.FORCED
    p = R.panel(oracle, n, c, T)
    lam, logl = _nulls(gpu_api, oracle, n, c, T)
    dev = torch.device("cuda")
    UtX, UtY = _dev(p["UtX"]), _dev(p["UtY"])
    pairs = gpu_api.LMM._pairs_dev(_pairs_t([[1, 0], [2, 1], [3, 2]]), dev)
    out = torch.full((3, 8), 7.0, dtype=torch.float64, device=dev)
    blk = np.ascontiguousarray(np.random.default_rng(5).integers(0, 3, size=(R.L_ROWS, n)).astype(np.float64))
    hits_h, refined_h = np.zeros(64, dtype=sh.HIT_DTYPE), np.zeros(64, dtype=gpu_api.SUMSTAT_DTYPE)
    cnt = C.c_ulonglong(0)
    UtY_h, logl_h = np.ascontiguousarray(p["UtY"]), np.ascontiguousarray(logl)

    def every_call():
        return {"refine_setup": lib.gemma_hip_lmm_score_panel_refine_setup(UtY_h.ctypes.data, logl_h.ctypes.data),
                "refine_setup_d": lib.gemma_hip_lmm_score_panel_refine_setup_d(_p(UtY), logl_h.ctypes.data, None),
                "refine_assoc_d": lib.gemma_hip_lmm_score_panel_refine_assoc_d(_p(UtX), R.L_ROWS, n, _p(pairs), 3, _p(out), None),
                "refine_last_d": lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, _p(out), None),
                "hits_refine_batch": lib.gemma_hip_lmm_score_panel_hits_refine_batch(
                    L.GENO_F64_SNP_MAJOR, blk.ctypes.data, R.L_ROWS, n, 0.5, hits_h.ctypes.data, 64, C.addressof(cnt), None,
                    refined_h.ctypes.data)}

    def untouched():
        torch.cuda.synchronize()
        return bool((out == 7.0).all())

    # no setup at all, and a single-phenotype setup: every refine entry point is a state error
    assert set(every_call().values()) == {L.ESTATE}
    single = gpu_api.LMM(a_mode=4)
    single.setup(_dev(p["U"]), _dev(p["ev"]), _dev(p["UtW"]), _dev(p["UtY"][:, 0]))
    try:
        assert set(every_call().values()) == {L.ESTATE}
    finally:
        single.finish()
    lmm = gpu_api.LMM(a_mode=3)
    lmm.setup_score_panel(_dev(p["U"]), _dev(p["ev"]), _dev(p["UtW"]), UtY, lam)
    try:
        # a score panel without refine_setup
        assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(_p(UtX), R.L_ROWS, n, _p(pairs), 3, _p(out), None) == L.ESTATE
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, _p(out), None) == L.ESTATE
        assert lib.gemma_hip_lmm_score_panel_hits_refine_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, R.L_ROWS, n, 0.5, hits_h.ctypes.data, 64,
                                                               C.addressof(cnt), None, refined_h.ctypes.data) == L.ESTATE
        # refine_setup: null pointers
        assert lib.gemma_hip_lmm_score_panel_refine_setup(None, logl_h.ctypes.data) == L.EINVAL
        assert lib.gemma_hip_lmm_score_panel_refine_setup(UtY_h.ctypes.data, None) == L.EINVAL
        assert lib.gemma_hip_lmm_score_panel_refine_setup_d(None, logl_h.ctypes.data, None) == L.EINVAL
        assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(_p(UtX), R.L_ROWS, n, _p(pairs), 3, _p(out), None) == L.ESTATE  # a failed setup is none
        assert untouched()
        assert lib.gemma_hip_lmm_score_panel_refine_setup(UtY_h.ctypes.data, logl_h.ctypes.data) == L.OK
        # no score-panel block since the setup
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, _p(out), None) == L.ESTATE
        assert "no score-panel block" in lib.gemma_hip_last_error().decode()
        # m == 0 returns OK and touches nothing, null pointers included
        assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(None, 0, 0, None, 0, None, None) == L.OK
        assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(_p(UtX), R.L_ROWS, n, _p(pairs), 0, _p(out), None) == L.OK
        assert untouched()
        # null pointers with m > 0, ld_utx < n
        for args in ((None, R.L_ROWS, n, _p(pairs), 3, _p(out)), (_p(UtX), R.L_ROWS, n, None, 3, _p(out)), (_p(UtX), R.L_ROWS, n, _p(pairs), 3, None),
                     (_p(UtX), R.L_ROWS, n - 1, _p(pairs), 3, _p(out))):
            assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(*args, None) == L.EINVAL
        assert untouched()
        # a block: refine_last_d works, m == 0 and null pointers as above
        lmm.batch_score_panel_hits(torch.from_numpy(blk).to(dev), L.GENO_F64_SNP_MAJOR, 0.5)
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(None, 0, None, None) == L.OK
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(None, 3, _p(out), None) == L.EINVAL
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, None, None) == L.EINVAL
        assert untouched()
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, _p(out), None) == L.OK
        assert not untouched()
        # dbg_utx overwrites the U^T x buffer: the remembered block is gone until the next batch
        lmm.dbg_utx(blk, L.GENO_F64_SNP_MAJOR, 1)
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, _p(out), None) == L.ESTATE
        lmm.batch_score_panel(torch.from_numpy(blk).to(dev), L.GENO_F64_SNP_MAJOR)
        assert lib.gemma_hip_lmm_score_panel_refine_last_d(_p(pairs), 3, _p(out), None) == L.OK
        # the host form: refined is needed with a list
        assert lib.gemma_hip_lmm_score_panel_hits_refine_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, R.L_ROWS, n, 0.5, hits_h.ctypes.data, 64,
                                                               C.addressof(cnt), None, None) == L.EINVAL
        assert lib.gemma_hip_lmm_score_panel_hits_refine_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, R.L_ROWS, n, 0.5, hits_h.ctypes.data, 64,
                                                               C.addressof(cnt), None, refined_h.ctypes.data) == L.OK
        assert 0 < cnt.value <= 64
        # count only: no list, no records
        assert lib.gemma_hip_lmm_score_panel_hits_refine_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, R.L_ROWS, n, 0.5, None, 0,
                                                               C.addressof(cnt), None, None) == L.OK
        # a new score-panel setup takes the refinement state down with the old one
        lmm.setup_score_panel(_dev(p["U"]), _dev(p["ev"]), _dev(p["UtW"]), UtY, lam)
        assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(_p(UtX), R.L_ROWS, n, _p(pairs), 3, _p(out), None) == L.ESTATE
        assert lib.gemma_hip_lmm_score_panel_refine_setup_d(_p(UtY), logl_h.ctypes.data, None) == L.OK
        assert lib.gemma_hip_lmm_score_panel_refine_assoc_d(_p(UtX), R.L_ROWS, n, _p(pairs), 3, _p(out), None) == L.OK
        torch.cuda.synchronize()
    finally:
        lmm.finish()
    # gemma_hip_lmm_finish has taken everything down
    assert set(every_call().values()) == {L.ESTATE}
    # the mirrors say what is wrong with a list
    with pytest.raises(ValueError):
        gpu_api.LMM._pairs_dev(torch.zeros((3, 3), dtype=torch.int64), dev)
    with pytest.raises(ValueError):
        gpu_api.LMM._pairs_dev(torch.tensor([[-1, 0]]), dev)

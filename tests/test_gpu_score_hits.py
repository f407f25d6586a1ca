"""The hits form of the score panel (gemma_hip_lmm_score_panel_hits_*, LMM.batch_score_panel_hits / assoc_score_panel_hits /
AnalyzeScorePanelHits, tests/cpp/score_panel_file_driver.cpp) on the MI355X.

The reference of every case but the last two is the records form of the same process on the same blocks after the same setup,
filtered by the restatement tests/scorehitcases.select: the hit list equals it as a set of (pheno, snp) and bit for bit in beta, se
and p_score, and `best` equals its argmin bit for bit, snp included.  Shapes: n = 203 (K no multiple of 4), the blocks of
scorecases.BLOCKS (1, 130 and 300 SNPs, each twice), (c, T) of scorehitcases.SHAPES; p_max of scorehitcases.P_MAXES and the
p_score of one pair of the block (that pair is a hit: its F sits on the critical value, behind the pre-filter's margin of 1e-9).
The null lambdas are a fixed spread over 1e-3 ... 1e2: what is compared is two forms of one product, not a fit."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import filecases as fc
import multicases as mc
import scorecases as sc
import scorehitcases as sh

pytestmark = pytest.mark.gpu
KINDS = ("hard", "plink", "dosage")


def _lams(T):
    return np.logspace(-3, 2, T) if T > 1 else np.array([0.5])


@functools.lru_cache(maxsize=None)
def _inputs(kind, c, T):
    """blocks, geno_kind, U, eval, UtW, UtY, indicator"""
    from gemma_amd import _lib as L
    if kind == "plink":
        raw, U, ev, UtW, UtY, ind = sh.plink_panel(c, T)
        return sc.cut(raw), L.GENO_PLINK_2BIT, U, ev, UtW, UtY, ind
    X, U, ev, UtW, UtY = sc.panel(203, c, T, dosage=(kind == "dosage"))
    return sc.cut(X), L.GENO_F64_SNP_MAJOR, U, ev, UtW, UtY, None


def _setup(api, kind, c, T):
    blocks, gk, U, ev, UtW, UtY, ind = _inputs(kind, c, T)
    lmm = api.LMM(a_mode=3)
    lmm.setup_score_panel(U, ev, UtW, UtY, _lams(T))
    if ind is not None:
        lmm.set_indicator(ind)
    return lmm, blocks, gk


def _hold(got, want, tag):
    (gh, gb), (wh, wb) = got, want
    assert len(gh) == len(wh), (tag, "hits", len(gh), len(wh))
    assert np.array_equal(gh["pheno"], wh["pheno"]) and np.array_equal(gh["snp"], wh["snp"]), (tag, "the index sets differ")
    assert sh.same_bits(gh, wh), (tag, "a hit differs from its record")
    assert np.array_equal(gb["snp"], wb["snp"]), (tag, "best snp", gb["snp"], wb["snp"])
    assert sh.same_bits(gb, wb), (tag, "a best differs from its record")


@pytest.mark.parametrize("c,T", sh.SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_hits_equal_the_filtered_records(gpu_api, kind, c, T):
    lmm, blocks, gk = _setup(gpu_api, kind, c, T)
    try:
        seen = 0
        for b, blk in enumerate(blocks):
            rec = lmm.batch_score_panel(blk, gk)
            assert gpu_api.last_utx_path() == (0 if kind == "dosage" else 1)
            assert not np.isnan(rec["p_score"]).any()  # no degenerate row in these panels
            pick = float(rec["p_score"][T // 2, rec.shape[1] // 2])
            for p_max in sh.P_MAXES + (pick,):
                got = lmm.batch_score_panel_hits(blk, gk, p_max)
                want = sh.select(rec, p_max)
                _hold(got, want, "%s c=%d T=%d block %d p_max=%g" % (kind, c, T, b, p_max))
                if p_max == 1.0:
                    assert len(got[0]) == rec.size  # every pair with a p_score
                if p_max == 0.0:
                    assert len(got[0]) == int((rec["p_score"] == 0.0).sum())
                if p_max == pick:
                    assert ((got[0]["pheno"] == T // 2) & (got[0]["snp"] == rec.shape[1] // 2)).any()  # p == p_max is a hit
                seen += len(got[0])
        assert seen > 0
    finally:
        lmm.finish()


def test_planted_degenerate_rows_are_neither_hits_nor_best(gpu_api):
    """monomorphic and all-missing rows (scorecases.PLANTED): their P_xx is rounding noise or NaN.  The hits form leaves such pairs
    out whatever their noise p_score is, so the reference is the records with the planted rows set to NaN."""
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = sc.panel(203, 3, 17, planted=True)
    lmm = gpu_api.LMM(a_mode=3)
    lmm.setup_score_panel(U, ev, UtW, UtY, _lams(17))
    try:
        s0 = 0
        for blk in sc.cut(X):
            rec = lmm.batch_score_panel(blk, L.GENO_F64_SNP_MAJOR)
            inside = [s - s0 for s in sc.PLANTED if s0 <= s < s0 + len(blk)]
            for k in sc.FIELDS:
                rec[k][:, inside] = np.nan
            for p_max in (0.05, 1e-3, 1.0):
                hits, best = lmm.batch_score_panel_hits(blk, L.GENO_F64_SNP_MAJOR, p_max)
                assert not np.isin(hits["snp"], inside).any() and not np.isin(best["snp"], inside).any()
                _hold((hits, best), sh.select(rec, p_max), "planted block at %d p_max=%g" % (s0, p_max))
            s0 += len(blk)
        only = np.ascontiguousarray(X[list(sc.PLANTED)])  # a block of nothing but such rows
        for p_max in (0.05, 1.0):
            hits, best = lmm.batch_score_panel_hits(only, L.GENO_F64_SNP_MAJOR, p_max)
            assert len(hits) == 0
            assert (best["snp"] == -1).all() and all(np.isnan(best[k]).all() for k in sh.STATS)
        hits, best = lmm.batch_score_panel_hits(np.zeros((0, 203)), L.GENO_F64_SNP_MAJOR, 0.05)  # l == 0
        assert len(hits) == 0 and (best["snp"] == -1).all() and np.isnan(best["p_score"]).all()
    finally:
        lmm.finish()


def test_overflow_counts_everything_and_writes_nothing_past_the_list(gpu_api):
    import torch
    from gemma_amd import _lib as L
    lib = L.lib()
    lmm, blocks, gk = _setup(gpu_api, "hard", 3, 100)
    try:
        blk = blocks[4]
        l, ld = blk.shape
        rec = lmm.batch_score_panel(blk, gk)
        want, _ = sh.select(rec, 0.05)
        assert len(want) >= 200
        truth = {(int(h["pheno"]), int(h["snp"])): h.tobytes() for h in want}
        cap, guard = 10, 64
        # the host form
        buf = np.zeros(cap + guard, dtype=sh.HIT_DTYPE)
        buf.view(np.uint8)[:] = 0xAB
        cnt = C.c_ulonglong(0)
        rc = lib.gemma_hip_lmm_score_panel_hits_batch(gk, blk.ctypes.data, l, ld, 0.05, buf.ctypes.data, cap, C.addressof(cnt), None)
        assert rc == L.OK and cnt.value == len(want)
        assert (buf[cap:].view(np.uint8) == 0xAB).all()
        for h in buf[:cap]:
            assert truth.get((int(h["pheno"]), int(h["snp"]))) == h.tobytes()
        # the device form: the kernel's own guard
        dev = torch.device("cuda")
        raw = torch.full((cap + guard, 4), -6148914691236517206, dtype=torch.int64, device=dev)  # 0xAAAA...
        cnt_d = torch.zeros(1, dtype=torch.int64, device=dev)
        blk_d = torch.from_numpy(blk).to(dev)
        rc = lib.gemma_hip_lmm_score_panel_hits_batch_d(gk, blk_d.data_ptr(), l, ld, 0.05, raw.data_ptr(), cap, cnt_d.data_ptr(), None,
                                                        None)
        torch.cuda.synchronize()
        assert rc == L.OK and int(cnt_d.item()) == len(want)
        got = raw.cpu().numpy()
        assert (got[cap:] == -6148914691236517206).all()
        stored = got[:cap].copy().view(sh.HIT_DTYPE).ravel()
        assert len({(int(h["pheno"]), int(h["snp"])) for h in stored}) == cap
        for h in stored:
            assert truth.get((int(h["pheno"]), int(h["snp"]))) == h.tobytes()
        # count only
        cnt = C.c_ulonglong(0)
        assert lib.gemma_hip_lmm_score_panel_hits_batch(gk, blk.ctypes.data, l, ld, 0.05, None, 0, C.addressof(cnt), None) == L.OK
        assert cnt.value == len(want)
        # the mirror repeats with a sufficient list
        hits, _ = lmm.batch_score_panel_hits(blk, gk, 0.05, cap=cap)
        assert sh.same_bits(hits, want)
    finally:
        lmm.finish()


def test_two_runs_and_the_other_block_order_agree_bit_for_bit(gpu_api):
    import torch
    lmm, blocks, gk = _setup(gpu_api, "hard", 3, 100)
    try:
        dev = torch.device("cuda")
        use = [torch.from_numpy(blocks[k]).to(dev) for k in (2, 4)]

        def run(order):
            out = {}
            for k in order:
                h, b = lmm.batch_score_panel_hits(use[k], gk, 0.05)
                out[k] = (sh.hits_of_dev(h), sh.best_of_dev(b))
            return out
        first, again, other = run((0, 1)), run((0, 1)), run((1, 0))
        for k in (0, 1):
            assert len(first[k][0]) > 100
            for o in (again, other):
                assert sh.same_bits(first[k][0], o[k][0]) and sh.same_bits(first[k][1], o[k][1])
    finally:
        lmm.finish()


def test_hits_assoc_on_a_caller_made_utx(gpu_api):
    """hits_assoc_d on a torch U^T x with ld > n (odd: the unaligned row loads) gives the hits of the batch form"""
    import torch
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = sc.panel(203, 3, 17)
    blk = np.ascontiguousarray(X[:130])
    dev = torch.device("cuda")
    lmm = gpu_api.LMM(a_mode=3)
    Ud, evd, UtWd, UtYd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (U, ev, UtW, UtY))
    lmm.setup_score_panel(Ud, evd, UtWd, UtYd, _lams(17))
    try:
        hb, bb = lmm.batch_score_panel_hits(torch.from_numpy(blk).to(dev), L.GENO_F64_SNP_MAJOR, 0.05)
        assert hb.snp.is_cuda and hb.stats.is_cuda and bb.stats.is_cuda and tuple(bb.stats.shape) == (17, 3)
        want = sh.select(sh.as_records(lmm.batch_score_panel(torch.from_numpy(blk).to(dev), L.GENO_F64_SNP_MAJOR)), 0.05)
        _hold((sh.hits_of_dev(hb), sh.best_of_dev(bb)), want, "batch_d")
        UtX = lmm.dbg_utx(blk, L.GENO_F64_SNP_MAJOR, 1)
        for ld in (203 + 5, 203 + 6):
            buf = torch.full((130, ld), float("nan"), dtype=torch.float64, device=dev)
            buf[:, :203] = torch.from_numpy(UtX).to(dev)
            ha, ba = lmm.assoc_score_panel_hits(buf[:, :203], 0.05)
            assert len(ha.snp) > 20
            assert sh.same_bits(sh.hits_of_dev(ha), sh.hits_of_dev(hb)) and sh.same_bits(sh.best_of_dev(ba), sh.best_of_dev(bb)), ld
    finally:
        lmm.finish()


def test_analyze_score_panel_hits_over_three_blocks(gpu_api):
    import torch
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = sc.panel(203, 3, 17)
    X = np.ascontiguousarray(X[:730])  # 300 + 300 + 130
    lams = _lams(17)
    rec = gpu_api.LMM(a_mode=3).AnalyzeScorePanel(U, ev, UtW, UtY, X, L.GENO_F64_SNP_MAJOR, l_mle_null=lams, batch=300)
    want = sh.select(rec, 1e-2)
    assert len(want[0]) > 50 and want[0]["snp"].max() >= 600
    lmm = gpu_api.LMM(a_mode=3)
    got = lmm.AnalyzeScorePanelHits(U, ev, UtW, UtY, X, L.GENO_F64_SNP_MAJOR, 1e-2, l_mle_null=lams, batch=300)
    assert got[0].dtype == gpu_api.SCORE_HIT_DTYPE and lmm.scoreHits is got[0] and lmm.scoreBest is got[1]
    _hold(got, want, "numpy")
    dev = torch.device("cuda")
    Ud, evd, UtWd, UtYd, Xd = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (U, ev, UtW, UtY, X))
    h, b = gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(Ud, evd, UtWd, UtYd, Xd, L.GENO_F64_SNP_MAJOR, 1e-2, l_mle_null=lams, batch=300)
    assert h.snp.is_cuda and b.snp.is_cuda
    _hold((sh.hits_of_dev(h), sh.best_of_dev(b)), want, "torch")
    # nulls that are not given are fitted as AnalyzeScorePanel fits them
    rec = gpu_api.LMM(a_mode=3).AnalyzeScorePanel(U, ev, UtW, UtY, X[:130], L.GENO_F64_SNP_MAJOR)
    _hold(gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(U, ev, UtW, UtY, X[:130], L.GENO_F64_SNP_MAJOR, 0.05), sh.select(rec, 0.05), "fitted")


def test_hits_argument_and_state_errors(gpu_api):
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = sc.panel(203, 3, 17)
    blk = np.ascontiguousarray(X[:4])
    lib = L.lib()
    cnt = C.c_ulonglong(0)

    def count_only(p_max):
        return lib.gemma_hip_lmm_score_panel_hits_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, 4, 203, p_max, None, 0, C.addressof(cnt), None)
    lib.gemma_hip_lmm_finish(None, None)  # whatever an earlier test left behind (OK or ESTATE)
    assert count_only(0.5) == L.ESTATE  # before a setup
    lmm = gpu_api.LMM(a_mode=3)
    lmm.setup_score_panel(U, ev, UtW, UtY, _lams(17))
    want = sh.select(lmm.batch_score_panel(blk, L.GENO_F64_SNP_MAJOR), 0.5)
    for bad in (-1.0, 1.5, float("nan")):
        assert count_only(bad) == L.EINVAL
        with pytest.raises(L.GemmaHipError) as e:
            lmm.batch_score_panel_hits(blk, L.GENO_F64_SNP_MAJOR, bad)
        assert e.value.code == L.EINVAL
        _hold(lmm.batch_score_panel_hits(blk, L.GENO_F64_SNP_MAJOR, 0.5), want, "after p_max=%r" % bad)  # the state is still usable
    buf = np.zeros(4, dtype=sh.HIT_DTYPE)
    assert lib.gemma_hip_lmm_score_panel_hits_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, 4, 203, 0.5, None, 4, C.addressof(cnt),
                                                    None) == L.EINVAL  # a null list with room
    assert lib.gemma_hip_lmm_score_panel_hits_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, 4, 203, 0.5, buf.ctypes.data, 4, None,
                                                    None) == L.EINVAL  # nowhere to count
    assert count_only(0.5) == L.OK and cnt.value == len(want[0])
    lmm.finish()
    assert count_only(0.5) == L.ESTATE  # after finish()
    one = gpu_api.LMM(a_mode=3, l_mle_null=0.5)
    one.setup(U, ev, UtW, np.ascontiguousarray(UtY[:, 0]))
    assert count_only(0.5) == L.ESTATE  # after a single-phenotype setup
    one.finish()


@functools.lru_cache(maxsize=None)
def _reference_chain():
    """multicases.plink_set through SnpQC -> kinship (10-digit text round trip) -> eigendecomposition, as
    test_score_panel_pins_the_reference_p_score runs it; p_max and the printed tables from the golden alone"""
    from gemma_amd import api, _lib as L
    ref = np.load(mc.REF_NPZ)
    codes, pheno = mc.plink_set()
    assert np.array_equal(ref["codes"], codes) and np.array_equal(ref["pheno"], pheno)
    ns, ni = codes.shape
    raw = mc.pack_bed(codes)
    W = np.ones((ni, 1))
    keep = api.SnpQC(raw, L.GENO_PLINK_2BIT, np.ones(ni, dtype=np.int32), W)[0].astype(bool)
    rows = np.ascontiguousarray(raw[keep])
    K10 = api.WriteMatrix10(api.CalcKin(rows, L.GENO_PLINK_2BIT, ni, 1))
    K = K10.copy()
    api.CenterMatrix(K)
    U, ev = np.zeros((ni, ni)), np.zeros(ni)
    api.EigenDecomp_Zeroed(K, U, ev)
    names = ["rs%d" % (s + 1) for s in np.flatnonzero(keep)]
    return codes, pheno, rows, K10, U, ev, W, names, sh.golden_threshold(ref)


def _golden_gap(thr):
    p_max, below, total, ratio, tables = thr
    assert ratio >= 1 + 1e-3 and 5 <= below <= total // 2, (ratio, below, total)
    assert all(not (abs(p / p_max - 1) < 4e-4).any() for _, p in tables)  # 200 x STAT_TOL on either side
    return p_max, tables


def test_hits_against_the_reference_print(gpu_api):
    """tests/golden/ref_multi.npz: the hit set is the reference's rows with a printed p_score <= p_max, phenotype by phenotype,
    where p_max sits in a gap of the printed values that p_score's agreement with the print (filecases.STAT_TOL) cannot cross"""
    from gemma_amd import _lib as L
    codes, pheno, rows, K10, U, ev, W, names, thr = _reference_chain()
    p_max, tables = _golden_gap(thr)  # before anything else
    hits, best = gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(U, ev, U.T @ W, U.T @ pheno, rows, L.GENO_PLINK_2BIT, p_max)
    for t, (rs, printed) in enumerate(tables):
        assert rs == names, "the analysed SNPs differ from the reference's"
        mine = hits[hits["pheno"] == t]
        assert list(mine["snp"]) == list(np.flatnonzero(printed <= p_max)), t
        rel = np.abs(mine["p_score"] - printed[mine["snp"]]) / printed[mine["snp"]]
        assert (rel <= fc.STAT_TOL).all(), (t, float(rel.max()))
        lowest = np.flatnonzero(printed == printed.min())
        if len(lowest) == 1:
            assert best["snp"][t] == lowest[0], t
        assert abs(best["p_score"][t] - printed.min()) <= fc.STAT_TOL * printed.min(), t
    print("golden: p_max = %.6g with %d of %d rows below, %d hits" % (p_max, thr[1], thr[2], len(hits)))


def test_file_driver_writes_the_hits_of_the_reference(gpu_api, tmp_path):
    """score_panel_file_driver on the same PLINK set from files: run.hits.txt holds the reference's rows below p_max with the SNP
    columns of the reference's print and beta, se, p_score of LMM.AnalyzeScorePanelHits in WriteFiles' format; run.best.txt
    agrees with `best`; run.log.txt carries the nulls and the count"""
    from gemma_amd import build, _lib as L
    build.build()
    libdir = os.path.join(fc.ROOT, "gemma_amd")
    exe = str(tmp_path / "sfd")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(fc.ROOT, "include"),
                           os.path.join(fc.ROOT, "tests", "cpp", "score_panel_file_driver.cpp"), "-L" + libdir, "-lgemma_hip",
                           "-Wl,-rpath," + libdir, "-lz", "-pthread", "-o", exe])
    codes, pheno, rows, K10, U, ev, W, names, thr = _reference_chain()
    p_max, tables = _golden_gap(thr)
    pre = str(tmp_path / "M")
    mc.write_plink(pre, codes, pheno)
    np.savetxt(tmp_path / "pheno.txt", pheno, fmt="%.6f", delimiter="\t")
    np.savetxt(tmp_path / "K.cXX.txt", K10, fmt="%.10g", delimiter="\t")
    kv = fc.drive(exe, "-bfile", pre, "-p", tmp_path / "pheno.txt", "-k", tmp_path / "K.cXX.txt", "-lmm", 3, "-pmax", repr(p_max),
                  "-o", "run", "-outdir", tmp_path)
    assert int(kv["n_ph"]) == 3 and int(kv["ni_test"]) == 150 and int(kv["snps"]) == len(names)
    hits, best = gpu_api.LMM(a_mode=3).AnalyzeScorePanelHits(U, ev, U.T @ W, U.T @ pheno, rows, L.GENO_PLINK_2BIT, p_max)
    assert int(kv["hits"]) == len(hits) > 0
    ref = np.load(mc.REF_NPZ)
    snp_cols = {}
    for t in range(3):
        text = ref["assoc%d" % (t + 1)].tobytes().decode().strip().split("\n")
        for ln in text[1:]:
            w = ln.split("\t")
            snp_cols[w[1]] = w[:7]
    lines = open(tmp_path / "run.hits.txt").read().strip().split("\n")
    assert lines[0].split("\t") == "chr rs ps n_miss allele1 allele0 af phenotype beta se p_score".split()
    body = [ln.split("\t") for ln in lines[1:]]
    assert len(body) == len(hits)
    for w, h in zip(body, hits):  # sorted by phenotype, then by the SNP order of the file
        rs = names[h["snp"]]
        assert w[:7] == snp_cols[rs] and int(w[7]) == h["pheno"] + 1
        assert float(tables[h["pheno"]][1][h["snp"]]) <= p_max
        # the driver fits its nulls through the C++ mirror of CalcLambdaNull: the statistics agree to the print, not to the bit
        for txt, k in zip(w[8:], sh.STATS):
            assert abs(float(txt) - h[k]) <= 2e-6 * abs(h[k]), (rs, k, txt, h[k])
            assert len(txt.split("e")[0].lstrip("-")) == 8  # "%.6e"
    for t, (rs, printed) in enumerate(tables):
        assert [w[1] for w in body if int(w[7]) == t + 1] == [rs[s] for s in np.flatnonzero(printed <= p_max)]
    lines = open(tmp_path / "run.best.txt").read().strip().split("\n")
    assert lines[0].split("\t") == "phenotype rs ps beta se p_score".split() and len(lines) == 4
    for t, ln in enumerate(lines[1:]):
        w = ln.split("\t")
        assert int(w[0]) == t + 1 and w[1] == names[best["snp"][t]] and w[2] == snp_cols[w[1]][2]
        assert abs(float(w[5]) - best["p_score"][t]) <= 2e-6 * best["p_score"][t]
    log = open(tmp_path / "run.log.txt").read()
    assert all("l_mle_null.%d = " % t in log for t in (1, 2, 3)) and "number of hits = %d" % len(hits) in log

"""The host plumbing of the LMM entry points, pinned byte for byte: what a host block entry point reads of a row, the three sources
of a setup (host arrays, device arrays, the kept U), and what a setup does to the state of the one before it.

Everything here goes through the C ABI directly (ctypes), with tiny shapes; outputs are compared as raw bytes since the records hold
NaN."""
import ctypes as C

import numpy as np
import pytest

from gemma_amd import _lib as L

pytestmark = pytest.mark.gpu

SNP, BED, IDV = L.GENO_F64_SNP_MAJOR, L.GENO_PLINK_2BIT, L.GENO_F64_IDV_MAJOR
PAD = 3  # items of padding behind every row of the wide layout
T_PANEL = 3


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _cfg(a_mode, n, c):
    cfg = L.LmmCfg()
    cfg.a_mode, cfg.n, cfg.n_cvt = a_mode, n, c
    cfg.l_min, cfg.l_max, cfg.n_region = 1e-5, 1e5, 10
    cfg.l_mle_null, cfg.logl_mle_H0 = 0.3, -10.0
    cfg.plink_nan_rule = 0  # the PLINK carry chain would make a block's records depend on the block before it
    return cfg


def _problem(n, c, T, seed):
    """U, eval of a random centred kinship, W (intercept first), Y (n x T), and their rotations"""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(n, 40)).astype(np.float64)
    G -= G.mean(axis=0)
    K = G @ G.T / 40.0
    ev, U = np.linalg.eigh(K)
    ev = np.where(ev < 1e-10, 0.0, ev)
    W = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
    Y = rng.standard_normal((n, T))
    U = np.ascontiguousarray(U)
    return dict(n=n, c=c, T=T, K=K, U=U, ev=np.ascontiguousarray(ev), W=W, Y=Y, UtW=np.ascontiguousarray(U.T @ W),
                UtY=np.ascontiguousarray(U.T @ Y))


def _block(kind, n, l, per_row, rng):
    """(contiguous, wide) layouts of one block and its (rows, need): the wide one holds the same data with PAD items behind every row,
    NaN for fp64 input and 0xFF for 2-bit rows.  fp64 blocks of l = 1 are hard calls (the int8-digit product), longer ones real-valued
    dosages (the fp64 GEMM, with the even-ld copy of U at odd n)."""
    if kind == BED:
        rows, need = l, (per_row + 3) // 4
        data = rng.integers(0, 256, size=(rows, need)).astype(np.uint8)
        wide = np.full((rows, need + PAD), 0xFF, dtype=np.uint8)
    else:
        vals = rng.integers(0, 3, size=(l, n)).astype(np.float64) if l == 1 else np.round(rng.uniform(0.0, 2.0, size=(l, n)), 5)
        if kind == SNP:
            vals[0, n // 2] = np.nan
            rows, need, data = l, n, vals
        else:  # the reference's Xlarge: individuals x SNPs, already imputed
            rows, need, data = n, l, np.ascontiguousarray(vals.T)
        wide = np.full((rows, need + PAD), np.nan)
    data = np.ascontiguousarray(data)
    wide[:, :need] = data
    return data, wide, need


def _twice(call, kind, n, l, per_row, out_bytes, seed):
    """call(geno, ld, out) on the contiguous and on the wide layout of one block -> the two outputs as bytes"""
    data, wide, need = _block(kind, n, l, per_row, np.random.default_rng(seed))
    outs = []
    for geno, ld in ((data, need), (wide, need + PAD)):
        out = np.full(out_bytes, 0xAB, dtype=np.uint8)
        call(geno, ld, out)
        outs.append(out.tobytes())
    return outs


def _setup_single(pb, a_mode=1, col=0):
    lib = L.lib()
    uty = np.ascontiguousarray(pb["UtY"][:, col])
    L.check(lib.gemma_hip_lmm_setup(C.byref(_cfg(a_mode, pb["n"], pb["c"])), _p(pb["U"]), _p(pb["ev"]), _p(pb["UtW"]), _p(uty)), "lmm_setup")


def _finish():
    L.check(L.lib().gemma_hip_lmm_finish(None, None), "lmm_finish")


def _indicator(pb, ni_total):
    ind = np.ones(ni_total, dtype=np.int32)
    ind[[1, ni_total - 2][:ni_total - pb["n"]]] = 0
    assert ind.sum() == pb["n"]
    L.check(L.lib().gemma_hip_lmm_set_indicator(_p(ind), ni_total), "lmm_set_indicator")


# ---- entry point -> (kinds, runner).  A runner sets the state up, calls _twice and finishes.
def _run_lmm(api, pb, kind, l, ni_total=0):
    lib = L.lib()
    _setup_single(pb)
    try:
        if ni_total:
            _indicator(pb, ni_total)
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_lmm_batch(kind, _p(g), l, ld, _p(o)), "lmm_batch"), kind, pb["n"], l,
                      ni_total or pb["n"], l * 64, 11)
    finally:
        _finish()


def _run_lm(api, pb, kind, l):
    lib = L.lib()
    y = np.ascontiguousarray(pb["Y"][:, 0])
    L.check(lib.gemma_hip_lm_setup(51, pb["n"], pb["c"], _p(pb["W"]), _p(y)), "lm_setup")
    try:
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_lm_batch(kind, _p(g), l, ld, _p(o)), "lm_batch"), kind, pb["n"], l, pb["n"],
                      l * 64, 12)
    finally:
        L.check(lib.gemma_hip_lm_finish(), "lm_finish")


def _run_multi(api, pb, kind, l):
    lib = L.lib()
    T = pb["T"]
    L.check(lib.gemma_hip_lmm_multi_setup(C.byref(_cfg(1, pb["n"], pb["c"])), T, None, None, _p(pb["U"]), _p(pb["ev"]), _p(pb["UtW"]),
                                          _p(pb["UtY"])), "lmm_multi_setup")
    try:
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_lmm_multi_batch(kind, _p(g), l, ld, _p(o)), "lmm_multi_batch"), kind, pb["n"],
                      l, pb["n"], T * l * 64, 13)
    finally:
        _finish()


def _score_setup(pb):
    lam = np.linspace(0.2, 1.5, pb["T"])
    L.check(L.lib().gemma_hip_lmm_score_panel_setup(C.byref(_cfg(3, pb["n"], pb["c"])), pb["T"], _p(lam), _p(pb["U"]), _p(pb["ev"]),
                                                    _p(pb["UtW"]), _p(pb["UtY"])), "lmm_score_panel_setup")


def _run_score(api, pb, kind, l):
    lib = L.lib()
    _score_setup(pb)
    try:
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_lmm_score_panel_batch(kind, _p(g), l, ld, _p(o)), "lmm_score_panel_batch"),
                      kind, pb["n"], l, pb["n"], pb["T"] * l * 24, 14)
    finally:
        _finish()


def _run_hits(api, pb, kind, l):
    lib = L.lib()
    T = pb["T"]
    cap = T * l
    _score_setup(pb)

    def call(g, ld, o):  # o: the sorted list, the count, the best of every phenotype
        L.check(lib.gemma_hip_lmm_score_panel_hits_batch(kind, _p(g), l, ld, 1.0, _p(o), cap, _p(o[cap * 32:]), _p(o[cap * 32 + 8:])),
                "lmm_score_panel_hits_batch")
    try:
        return _twice(call, kind, pb["n"], l, pb["n"], cap * 32 + 8 + T * 32, 15)
    finally:
        _finish()


def _run_mvlmm(api, pb, kind, l):
    lib = L.lib()
    d = 2
    UtY = np.ascontiguousarray(pb["UtY"][:, :d])
    mv = api.MVLMM(a_mode=1)
    mv.fit_null(pb["ev"], pb["UtW"], UtY)
    _setup_single(pb)
    try:
        opt = mv._opt()
        L.check(lib.gemma_hip_mvlmm_set(d, _p(UtY), C.byref(mv._null_struct), C.byref(opt)), "mvlmm_set")
        stride = d + 3 * (d * (d + 1) // 2) + 3
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_mvlmm_batch(kind, _p(g), l, ld, _p(o)), "mvlmm_batch"), kind, pb["n"], l,
                      pb["n"], l * stride * 8, 16)
    finally:
        _finish()


def _run_gxe(api, pb, kind, l):
    lib = L.lib()
    env = np.random.default_rng(5).standard_normal(pb["n"])
    _setup_single(pb)
    try:
        L.check(lib.gemma_hip_lmm_set_env(_p(env)), "lmm_set_env")
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_lmm_gxe_batch(kind, _p(g), l, ld, _p(o)), "lmm_gxe_batch"), kind, pb["n"], l,
                      pb["n"], l * 64, 17)
    finally:
        _finish()


def _run_gene(api, pb, kind, l):
    lib = L.lib()
    n = pb["n"]
    _setup_single(pb)  # the tested variable sits in the Uty slot
    try:
        rng = np.random.default_rng(18)
        data = np.ascontiguousarray(rng.standard_normal((l, n)))
        wide = np.full((l, n + PAD), np.nan)
        wide[:, :n] = data
        outs = []
        for Y, ld in ((data, n), (wide, n + PAD)):
            out = np.full(l * 64, 0xAB, dtype=np.uint8)
            L.check(lib.gemma_hip_lmm_gene_batch(_p(Y), l, ld, _p(out)), "lmm_gene_batch")
            outs.append(out.tobytes())
        return outs
    finally:
        _finish()


def _run_dbg_utx(api, pb, kind, l):
    lib = L.lib()
    _setup_single(pb)
    try:
        return _twice(lambda g, ld, o: L.check(lib.gemma_hip_dbg_utx(kind, _p(g), l, ld, 1, _p(o)), "dbg_utx"), kind, pb["n"], l, pb["n"],
                      l * pb["n"] * 8, 19)
    finally:
        _finish()


ENTRIES = {"lmm_batch": ((SNP, BED, IDV), _run_lmm), "lm_batch": ((SNP, BED, IDV), _run_lm), "lmm_multi_batch": ((SNP, BED, IDV), _run_multi),
           "lmm_score_panel_batch": ((SNP, BED, IDV), _run_score), "lmm_score_panel_hits_batch": ((SNP, BED, IDV), _run_hits),
           "mvlmm_batch": ((SNP, BED, IDV), _run_mvlmm), "lmm_gxe_batch": ((SNP, BED), _run_gxe),  # GXE: SNP-major input only
           "lmm_gene_batch": ((None,), _run_gene),  # no geno_kind: rows of n doubles
           "dbg_utx": ((SNP, BED, IDV), _run_dbg_utx)}
CASES = [(name, kind) for name, (kinds, _) in ENTRIES.items() for kind in kinds]


@pytest.fixture(scope="module")
def problems():
    return {n: _problem(n, 1, T_PANEL, 100 + n) for n in (7, 8)}


@pytest.mark.parametrize("l", [1, 5])
@pytest.mark.parametrize("n", [7, 8])
@pytest.mark.parametrize("name,kind", CASES, ids=["%s-%s" % (a, {SNP: "snp", BED: "bed", IDV: "idv", None: "rows"}[k]) for a, k in CASES])
def test_host_staging_reads_only_what_a_row_holds(gpu_api, problems, name, kind, n, l):
    """A host block entry point gives the same bytes for a contiguous block (ld = need) and for the same rows inside a wider array
    (ld = need + 3) whose padding holds NaN / 0xFF: it reads the `need` leading items of every row and nothing else."""
    a, b = ENTRIES[name][1](gpu_api, problems[n], kind, l)
    assert len(a) and a == b


def test_host_staging_plink_rows_of_all_individuals(gpu_api, problems):
    """with an indicator (7 of 9 individuals analysed) a PLINK row holds ceil(9 / 4) bytes, not ceil(7 / 4)"""
    a, b = _run_lmm(gpu_api, problems[7], BED, 5, ni_total=9)
    assert a == b


# ---- the three sources of a setup --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kept(gpu_api):
    """a problem whose (U, eval) are the library's own: gemma_hip_eigh_keep of a centred K, read back with gemma_hip_kept_U_get"""
    lib = L.lib()
    n, c = 12, 2
    pb = _problem(n, c, T_PANEL, 7)
    K = pb["K"] - pb["K"].mean(axis=0)[None, :] - pb["K"].mean(axis=1)[:, None] + pb["K"].mean()
    K = np.ascontiguousarray((K + K.T) / 2.0)
    ev, tr = np.zeros(n), C.c_double()
    L.check(lib.gemma_hip_eigh_keep(_p(K), n, _p(ev), C.byref(tr)), "eigh_keep")
    U = np.zeros((n, n))
    L.check(lib.gemma_hip_kept_U_get(_p(U), _p(ev)), "kept_U_get")
    pb.update(U=U, ev=ev, UtW=np.ascontiguousarray(U.T @ pb["W"]), UtY=np.ascontiguousarray(U.T @ pb["Y"]))
    fits = gpu_api.CalcLambdaNullPanel(ev, pb["UtW"], pb["UtY"])
    pb["lam"] = np.ascontiguousarray(fits["l_mle_null"], dtype=np.float64)
    pb["logl"] = np.ascontiguousarray(fits["logl_mle_H0"], dtype=np.float64)
    rng = np.random.default_rng(21)
    X = rng.integers(0, 3, size=(5, n)).astype(np.float64)
    X[2, 4] = np.nan
    pb["X"] = X
    yield pb
    L.check(lib.gemma_hip_kept_release(), "kept_release")


def _family(name, pb):
    """-> (setup(source, arrays), batch() -> bytes) of one family; arrays: (U, eval, UtW, UtY) as pointers of the source"""
    lib = L.lib()
    n, c, T, l = pb["n"], pb["c"], pb["T"], pb["X"].shape[0]
    lam, logl = _p(pb["lam"]), _p(pb["logl"])
    if name == "single":
        cfg = _cfg(1, n, c)
        host = lambda U, ev, W, Y: lib.gemma_hip_lmm_setup(C.byref(cfg), U, ev, W, Y)
        dev = lambda U, ev, W, Y, s: lib.gemma_hip_lmm_setup_d(C.byref(cfg), U, ev, W, Y, s)
        kept_ = lambda W, Y: lib.gemma_hip_lmm_setup_kept(C.byref(cfg), W, Y)
        batch, size, cols = lib.gemma_hip_lmm_batch, l * 64, 1
    elif name == "multi":
        cfg = _cfg(1, n, c)
        host = lambda U, ev, W, Y: lib.gemma_hip_lmm_multi_setup(C.byref(cfg), T, lam, logl, U, ev, W, Y)
        dev = lambda U, ev, W, Y, s: lib.gemma_hip_lmm_multi_setup_d(C.byref(cfg), T, lam, logl, U, ev, W, Y, s)
        kept_ = lambda W, Y: lib.gemma_hip_lmm_multi_setup_kept(C.byref(cfg), T, lam, logl, W, Y)
        batch, size, cols = lib.gemma_hip_lmm_multi_batch, T * l * 64, T
    else:
        cfg = _cfg(3, n, c)
        host = lambda U, ev, W, Y: lib.gemma_hip_lmm_score_panel_setup(C.byref(cfg), T, lam, U, ev, W, Y)
        dev = lambda U, ev, W, Y, s: lib.gemma_hip_lmm_score_panel_setup_d(C.byref(cfg), T, lam, U, ev, W, Y, s)
        kept_ = lambda W, Y: lib.gemma_hip_lmm_score_panel_setup_kept(C.byref(cfg), T, lam, W, Y)
        batch, size, cols = lib.gemma_hip_lmm_score_panel_batch, T * l * 24, T

    def run():
        out = np.full(size, 0xAB, dtype=np.uint8)
        L.check(batch(SNP, _p(pb["X"]), l, n, _p(out)), name + " batch")
        return out.tobytes()
    return host, dev, kept_, run, cols


@pytest.mark.parametrize("name", ["single", "multi", "score"])
def test_three_sources_of_a_setup_are_one_setup(gpu_api, kept, name):
    """The kept U, host arrays and device arrays of the same values give the same setup: one fp64 block, byte for byte."""
    import torch
    pb = kept
    host, dev, kept_, run, cols = _family(name, pb)
    UtY = np.ascontiguousarray(pb["UtY"][:, :cols]) if cols > 1 else np.ascontiguousarray(pb["UtY"][:, 0])
    outs = {}
    L.check(kept_(_p(pb["UtW"]), _p(UtY)), name + " setup_kept")
    try:
        outs["kept"] = run()
    finally:
        _finish()
    L.check(host(_p(pb["U"]), _p(pb["ev"]), _p(pb["UtW"]), _p(UtY)), name + " setup")
    try:
        outs["host"] = run()
    finally:
        _finish()
    t = [torch.from_numpy(a).cuda() for a in (pb["U"], pb["ev"], pb["UtW"], UtY)]  # borrowed by the library until finish
    torch.cuda.synchronize()
    L.check(dev(*[C.c_void_p(x.data_ptr()) for x in t], C.c_void_p(torch.cuda.current_stream().cuda_stream)), name + " setup_d")
    try:
        outs["dev"] = run()
    finally:
        _finish()
    assert outs["kept"] == outs["host"]
    assert outs["dev"] == outs["host"]


# ---- a setup takes the state of the one before it down ------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["multi", "score"])
def test_single_setup_over_an_unfinished_panel_setup(gpu_api, problems, first):
    """A multi (score-panel) setup, then a single setup without lmm_finish in between: the panel batches answer ESTATE and
    gemma_hip_lmm_batch gives the bytes of a fresh single setup."""
    lib = L.lib()
    pb = problems[8]
    n, T, l = pb["n"], pb["T"], 5
    X, _, _ = _block(SNP, n, l, n, np.random.default_rng(31))

    def single():
        out = np.full(l * 64, 0xAB, dtype=np.uint8)
        L.check(lib.gemma_hip_lmm_batch(SNP, _p(X), l, n, _p(out)), "lmm_batch")
        return out.tobytes()

    _setup_single(pb)
    try:
        fresh = single()
    finally:
        _finish()
    if first == "multi":
        L.check(lib.gemma_hip_lmm_multi_setup(C.byref(_cfg(1, n, pb["c"])), T, None, None, _p(pb["U"]), _p(pb["ev"]), _p(pb["UtW"]),
                                              _p(pb["UtY"])), "lmm_multi_setup")
    else:
        _score_setup(pb)
    try:
        _setup_single(pb)
        panel = np.zeros(T * l * 64, dtype=np.uint8)
        assert lib.gemma_hip_lmm_multi_batch(SNP, _p(X), l, n, _p(panel)) == L.ESTATE
        assert lib.gemma_hip_lmm_score_panel_batch(SNP, _p(X), l, n, _p(panel)) == L.ESTATE
        assert single() == fresh
    finally:
        _finish()

"""The first-pass kernels at their edges: snp_qc_kernel, the ingest kernels, transpose_kernel, the centring kernels, loco_kernel,
zero_small_eval_kernel, plink_carry_kernel and lm_assoc_kernel against the plain references of tests/firstpasscases.py (exact
where the quantity is an integer or one correctly rounded division of integers, long double with a derived bar elsewhere).
The shapes are tiny on purpose: n below, at and astride the 64 lanes of the wavefront that owns a SNP, l that leaves the last
workgroup of four SNPs partly empty, ni_total % 4 in every residue with individuals dropped at the byte boundaries."""
import ctypes as C

import numpy as np
import pytest

import firstpasscases as FC

pytestmark = pytest.mark.gpu
U = FC.U
LD = FC.LD


@pytest.fixture(scope="module")
def api(gpu_api):
    return gpu_api


@pytest.fixture(scope="module")
def L():
    from gemma_amd import _lib
    return _lib


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, ref):
    """bit for bit, except that a NaN is any NaN"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan.ravel()], _bits(ref)[~nan.ravel()])


def _geno(cs_G, plink, L, extra=0):
    """(geno, kind) of rows over ALL individuals; extra > 0: a row stride above the minimum, with poison behind every row"""
    if plink:
        nb = (cs_G.shape[1] + 3) // 4
        return FC.pack_bed(FC.geno_to_codes(cs_G), ld=nb + extra, fill=0x55 if extra else 0xFF), L.GENO_PLINK_2BIT
    G = np.ascontiguousarray(cs_G, dtype=np.float64)
    return (FC.widen(G, G.shape[1] + extra, 1e300) if extra else G), L.GENO_F64_SNP_MAJOR


def _orthogonal(rng, n):
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return np.ascontiguousarray(Q), np.sort(rng.uniform(0.05, 3.0, size=n))


# ------------------------------------------------------------------------------------------------------- 1. QC
def _qc(api, L, cs, l=None, extra=0, W=None, ind="case", **cfg):
    G = cs["G"][:l]
    geno, kind = _geno(G, cs["plink"], L, extra)
    kw = dict(cs.get("cfg", {}))
    kw.update(cfg)
    return api.SnpQC(geno, kind, cs["ind"] if isinstance(ind, str) else ind, cs["W"] if W is None else W, **kw)


def _check_qc(got, ref, l, tag):
    got_i, got_maf, got_nm = got
    assert np.array_equal(got_nm, ref["n_miss"][:l]), (tag, got_nm, ref["n_miss"][:l])
    assert _same_bits(got_maf, ref["maf"][:l]), (tag, got_maf, ref["maf"][:l])
    assert np.array_equal(got_i, ref["indicator"][:l]), (tag, got_i, ref["why"][:l])


@pytest.mark.parametrize("n,pattern,rem,plink,seed", FC.qc_sweep_list())
def test_qc_statistics_and_cascade_sweep(api, L, n, pattern, rem, plink, seed):
    """n_miss and indicator_snp equal, maf bit for bit (one correctly rounded division of exact integers; NaN where nothing is
    observed) for every l that leaves the last workgroup partly empty; l = 5 also with a row stride above the minimum."""
    cs = FC.qc_sweep_case(n, pattern, rem, plink, seed)
    ref = FC.qc_reference(cs["G"], cs["ind"], cs["W"], plink, **cs["cfg"])
    for l in FC.L_LIST:
        _check_qc(_qc(api, L, cs, l=l), ref, l, (n, pattern, rem, plink, l))
    _check_qc(_qc(api, L, cs, l=5, extra=3), ref, 5, (n, pattern, rem, plink, "wide rows"))


@pytest.mark.parametrize("plink", [True, False])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 127, 129, 257])
def test_qc_without_an_indicator(api, L, n, plink):
    """indicator_idv == NULL: everybody is analysed and the PLINK rows end inside a byte (no n here is a multiple of 4)"""
    cs = FC.qc_sweep_case(n, "first", (n + 1) % 4, plink, 50 + n)
    keep = cs["ind"] != 0
    cs["G"] = np.ascontiguousarray(cs["G"][:, keep])
    cs["ind"] = np.ones(n, dtype=np.int32)
    ref = FC.qc_reference(cs["G"], cs["ind"], cs["W"], plink, **cs["cfg"])
    for l in (4, 9):
        _check_qc(_qc(api, L, cs, l=l, ind=None), ref, l, (n, plink, l))


@pytest.mark.parametrize("plink", [True, False])
def test_qc_planted_rows(api, L, plink):
    """Every planted row on its own (tests/test_firstpass_cases_cpu.py shows that the reference does what the names say): thresholds
    met exactly are kept (the code compares with > and <), one call further is dropped; maf_level = -1 switches the maf and the
    HWE filter off but not the polymorphism rule; a row equal to a covariate goes with three covariates and stays with one."""
    cs, row = FC.qc_planted_case(plink)
    for tag, over, W in (("levels", {}, None), ("maf_level -1", dict(maf_level=-1, hwe_level=FC.QC_PLANT_HWE), None),
                         ("hwe on", dict(hwe_level=FC.QC_PLANT_HWE), None), ("one covariate", {}, np.ones((cs["n"], 1)))):
        cfg = dict(cs["cfg"])
        cfg.update(over)
        ref = FC.qc_reference(cs["G"], cs["ind"], cs["W"] if W is None else W, plink, **cfg)
        got_i, got_maf, got_nm = _qc(api, L, cs, W=W, **over)
        for name, i in row.items():
            assert got_nm[i] == ref["n_miss"][i], (tag, name)
            assert _same_bits(got_maf[i:i + 1], ref["maf"][i:i + 1]), (tag, name, got_maf[i], ref["maf"][i])
            assert got_i[i] == ref["indicator"][i], (tag, name, "reference: %s" % ref["why"][i])
        if tag == "levels":
            kept = {k for k, i in row.items() if got_i[i]}
            assert {"miss_at_level", "maf_at_level", "maf_at_one_minus_level", "no_class0", "no_class1", "no_class2", "regular",
                    "no_het"} <= kept
            assert not kept & {"miss_above_level", "maf_below_level", "maf_above_one_minus_level", "mono0", "mono1", "mono2",
                               "all_missing_analysed", "one_observed", "equals_covariate"}
            assert np.isnan(got_maf[row["all_missing_analysed"]])
        if tag == "one covariate":
            assert got_i[row["equals_covariate"]] == 1
        if tag == "hwe on" and not plink:
            assert got_i[row["dosage_boundaries"]] == 1  # 0.5 is a homozygote of class 0, 1.5 one of class 2


@pytest.mark.parametrize("plink", [True, False])
def test_qc_hwe_on_planted_counts(api, L, plink):
    """The host's exact test through SnpQC against the exact Wigginton sum: every triple at every level that sits a factor of
    ten or more away from its p-value, so that rounding cannot flip the decision."""
    cs, trip = FC.hwe_case(plink)
    pvals = [FC.hwe_exact(*t) for t in trip]
    seen = set()
    for lv in FC.hwe_levels(trip):
        got_i, _, _ = _qc(api, L, cs, maf_level=0.0, miss_level=1.0, hwe_level=lv)
        for i, p in enumerate(pvals):
            p = float(p)
            if lv >= 10 * p * (1 - 1e-12) or lv <= p / 10 * (1 + 1e-12):
                assert got_i[i] == (0 if p < lv else 1), (trip[i], p, lv)
                seen.add((i, p < lv))
    assert len(seen) == 2 * len(trip)  # every triple was kept at one level and dropped at another


# ------------------------------------------------------------------------------------------- 2. LMM ingest
class _IdentityLMM:
    """api.LMM with U = I, eval = 1 and an intercept: dbg_utx(path=0) is the fp64 product of the ingested block with the identity,
    which is exact -- the ingest kernel's output itself"""

    def __init__(self, api, n, plink, ind=None):
        self.api = api
        self.lmm = api.LMM(a_mode=1)
        self.lmm.setup(np.eye(n), np.ones(n), np.ones((n, 1)), np.arange(n, dtype=np.float64) % 7, plink=plink)
        if ind is not None:
            self.lmm.set_indicator(ind)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.lmm.finish()

    def ingest(self, geno, kind):
        out = self.lmm.dbg_utx(geno, kind, 0)
        assert self.api.last_utx_path() == 0  # the fp64 GEMM, not the int8 digits
        return out


# The read-back goes through lmm_setup, which refuses n <= c + 1: with the intercept alone that is n < 3, so n = 1 and 2 of
# FC.N_LIST cannot be reached this way and ingest_lmm_kernel is NOT pinned below n = 3 by these tests (snp_qc_kernel and
# ingest_kin_kernel, which share its decode and lane loop, are pinned at n = 1 and 2 above and below).
LMM_INGEST_N = [3, 63, 64, 65, 127, 129, 257]


@pytest.mark.parametrize("n", LMM_INGEST_N)
def test_lmm_ingest_plink_bit_for_bit(api, L, n):
    """PLINK rows with and without an indicator (every pattern, ni_total % 4 rotating), every l; row 1 of the blocks of l >= 3 is
    missing throughout: all NaN, its neighbours in the workgroup untouched."""
    rng = np.random.default_rng(n)
    for k, pattern in enumerate(("none",) + FC.PATTERNS):
        ind = FC.indicator(n, pattern, (n + k) % 4)
        with _IdentityLMM(api, n, True, None if pattern == "none" else ind) as m:
            for l in FC.L_LIST:
                G = FC.hard_calls(rng, l, ind.size, miss=0.15)
                if l >= 3:
                    G[1, ind != 0] = np.nan
                ref = FC.impute_reference(G[:, ind != 0])
                for extra in ((0, 2) if l == 5 else (0,)):
                    got = m.ingest(_geno(G, True, L, extra)[0], L.GENO_PLINK_2BIT)
                    assert np.array_equal(got, ref, equal_nan=True), (n, pattern, l, extra)
                if l >= 3:
                    assert np.all(np.isnan(got[1]))  # (its neighbours equal the reference, above)


@pytest.mark.parametrize("n", LMM_INGEST_N)
def test_lmm_ingest_f64_snp_major_bit_for_bit(api, L, n):
    rng = np.random.default_rng(100 + n)
    with _IdentityLMM(api, n, False) as m:
        for l in FC.L_LIST:
            G = FC.hard_calls(rng, l, n, miss=0.15)
            if l >= 3:
                G[l - 2] = np.nan
            ref = FC.impute_reference(G)
            for extra in ((0, 3) if l == 5 else (0,)):
                geno = np.ascontiguousarray(np.hstack([G, np.full((l, extra), 1e300)]))  # dbg_utx takes the width as the stride
                got = m.ingest(geno, L.GENO_F64_SNP_MAJOR)
                assert np.array_equal(got, ref, equal_nan=True), (n, l, extra)
            if l >= 3:
                assert np.all(np.isnan(got[l - 2]))  # (its neighbours equal the reference, above)


@pytest.mark.parametrize("rows", [31, 32, 33])
def test_lmm_ingest_individual_major_is_the_transpose(api, L, rows):
    """transpose_kernel at 32 x 32 tiles: individuals x SNPs around 31 / 32 / 33, also 1 and 65 SNPs"""
    rng = np.random.default_rng(rows)
    with _IdentityLMM(api, rows, False) as m:
        for cols in (1, 31, 32, 33, 65):
            X = rng.integers(0, 3, size=(rows, cols)).astype(np.float64) + rng.integers(0, 8, size=(rows, cols)) / 8.0
            assert np.array_equal(m.ingest(X, L.GENO_F64_IDV_MAJOR), X.T), (rows, cols)


# --------------------------------------------------------------------------------------------- 3. kinship ingest
@pytest.fixture
def fp64_kin(api, monkeypatch):
    monkeypatch.setenv("GEMMA_HIP_KIN_I8", "0")
    api.reload_env()
    yield
    monkeypatch.undo()
    api.reload_env()


@pytest.mark.parametrize("n", FC.N_LIST)
def test_kin_ingest_against_long_double(api, L, fp64_kin, n):
    """ingest_kin_kernel (fp64 route) + the SYRK for k_mode 1 and 2, both encodings, p = 37 with a monomorphic row (variance 0:
    not scaled, contributes zeros) and a row with one observed call.  The bar is FC.kin_reference's: the dot-product bound
    p u sum |a_i b_i| of the reference's own operands plus the rounding of the centred (and scaled) entries themselves; K is
    bit-symmetric.  A SNP that is missing throughout is out of scope: QC removes it before the kinship is formed."""
    G = FC.kin_case(n, 300 + n)
    for k_mode in (1, 2):
        K_ref, bound = FC.kin_reference(G, k_mode)
        for plink in (True, False):
            geno, kind = _geno(G, plink, L, extra=0 if k_mode == 1 else 3)
            K = api.CalcKin(geno, kind, n, k_mode)
            assert np.array_equal(K, K.T), (n, k_mode, plink)
            err = np.abs(K.astype(LD) - K_ref)
            w = np.unravel_index(np.argmax(err - bound), err.shape)
            print("kin n=%d k_mode=%d plink=%d: worst |err| %.3e at bound %.3e" % (n, k_mode, plink, float(err[w]), float(bound[w])))
            assert np.all(err <= bound), (n, k_mode, plink, float(err[w]), float(bound[w]))


# ------------------------------------------------------------------------------------------------ 4. GXE ingest
def _gxe_rows(rng, n, l_each):
    """hard-call rows whose mean is not 1 and is EXACT (no missing call, or a power of two of observed ones: then x and 2 - x
    are imputed with m and 2 - m exactly and ingest to the same vector), and rows whose observed mean is exactly 1"""
    pow2 = 1 << (int(n).bit_length() - 1)
    if pow2 == n:
        pow2 //= 2
    rows, mean1 = [], []
    while len(rows) < l_each:
        x = rng.binomial(2, 0.3, size=n).astype(np.float64)
        if len(rows) % 2:
            x[rng.permutation(n)[:n - pow2]] = np.nan
        if np.nanmean(x) != 1 and len(set(x[~np.isnan(x)].tolist())) > 1:
            rows.append(x)
    for k in range(3):
        x = np.full(n, np.nan)
        half = (pow2 if k else n) // 2 - k
        x[rng.permutation(n)[:2 * half + k]] = np.concatenate([np.zeros(half), np.full(half, 2.0), np.ones(k)])
        mean1.append(x)
    return np.array(rows), np.array(mean1)


GXE_RTOL = 1e-6  # beta, se, logl_H1, p, lambda-hat against the oracle: the bar of test_gpu_parity.py::test_analyze_gxe
GXE_FIELDS = {1: ("beta", "se", "lambda_remle", "logl_H1", "p_wald"), 3: ("beta", "se", "p_score")}


def _records_within(got, ref, fields, rtol, tag):
    """|got - ref| <= rtol |ref| field by field (rtol: a number, or one per record), with the same NaN pattern"""
    for k in fields:
        g, r = got[k], ref[k]
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, k, g, r)
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        lim = (np.broadcast_to(rtol[k] if isinstance(rtol, dict) else rtol, r.shape)[ok]) * np.abs(r[ok])
        w = int(np.argmax(err - lim)) if ok.any() else 0
        assert np.all(err <= lim), (tag, k, g[ok][w], r[ok][w], err[w], lim[w])


@pytest.mark.parametrize("c", [1, 2])
@pytest.mark.parametrize("n", [63, 64, 65, 129])
def test_gxe_ingest_by_symmetry(api, L, oracle, n, c):
    """ingest_gxe_kernel: a block of rows x and the block of their complements 2 - x (PLINK: codes 0 and 3 swapped) ingest to the
    same vectors -- whichever of the two has a mean above 1 is recoded -- so AnalyzeGXE returns bit-identical records except
    beta, which changes sign.  Both encodings, PLINK behind an indicator; the complement block has a row stride above the
    minimum, so the bit identity holds across the two strides as well.

    Rows with a mean of exactly 1 are recoded in neither block: the two problems differ by x -> 2 - x in the covariates and
    z -> 2 env - z in the tested vector, the same model but two different float64 computations (2 - v itself is exact for hard
    calls; what differs is every sum formed from it).  Mode 3 has no lambda search: there each field is held to 8 times what
    the oracle's own float64 evaluation of the same two problems differs by, or 8 n u where the oracle's two agree more closely
    than one rounding per term -- measured on the CPU per row and field, never from device output.  Mode 1 goes through the
    lambda search, whose stopping rule (1e-5 relative) decides the last digits: the parity bar GXE_RTOL, lambda-hat included.

    And every record agrees with the oracle at these n within GXE_RTOL."""
    rng = np.random.default_rng(10 * n + c)
    Uo, ev = _orthogonal(rng, n)
    W = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(c - 1)])
    env = rng.standard_normal(n)
    rows, mean1 = _gxe_rows(rng, n, 9)
    X = np.vstack([rows[:5], mean1, rows[5:]])  # 12 rows: the planted ones astride the workgroups
    planted = np.arange(5, 8)
    reg = np.setdiff1d(np.arange(len(X)), planted)
    y = rng.standard_normal(n) + 0.4 * np.nan_to_num(X[0]) * env
    UtW, Uty = Uo.T @ W, Uo.T @ y
    ind = FC.indicator(n, "every_byte", n % 4)
    l_mle, logl0 = oracle.calc_lambda_null("L", ev, UtW, Uty)
    for mode in (1, 3):
        ref = oracle.gxe_analyze(mode, Uo, ev, UtW, Uty, env, X, l_mle_null=l_mle)
        tight = None
        if mode == 3:  # the oracle's own x against 2 - x on the planted rows
            ref_c = oracle.gxe_analyze(mode, Uo, ev, UtW, Uty, env, 2.0 - X[planted], l_mle_null=l_mle)
            tight = {}
            for k in GXE_FIELDS[3]:
                a_, b_ = ref[k][planted], (-ref_c[k] if k == "beta" else ref_c[k])
                tight[k] = 8 * np.maximum(np.abs(a_ - b_) / np.abs(a_), n * U)
        for plink in (False, True):
            recs = []
            for wide, blk in ((False, X), (True, 2.0 - X)):
                if plink:
                    G = np.random.default_rng(1).integers(0, 3, size=(len(blk), ind.size)).astype(np.float64)
                    G[:, ind != 0] = blk
                    geno, kind, indicator = _geno(G, True, L, 2 if wide else 0)[0], L.GENO_PLINK_2BIT, ind
                else:  # (AnalyzeGXE takes the width of the block as its row stride)
                    geno = np.ascontiguousarray(np.hstack([blk, np.full((len(blk), 3 if wide else 0), 1e300)]))
                    kind, indicator = L.GENO_F64_SNP_MAJOR, None
                recs.append(api.LMM(a_mode=mode, l_mle_null=l_mle, logl_mle_H0=logl0).AnalyzeGXE(
                    Uo, ev, UtW, Uty, env, geno, geno_kind=kind, indicator_idv=indicator, batch=5))
            a, b = recs
            tag = (n, c, mode, "plink" if plink else "f64")
            assert np.isfinite(a["beta"][reg]).mean() > 0.8
            for k in a.dtype.names:
                want = -a[k][reg] if k == "beta" else a[k][reg]
                assert _same_bits(b[k][reg], want), (tag, k)
            b_neg = b.copy()
            b_neg["beta"] = -b["beta"]
            if mode == 3:
                for k in GXE_FIELDS[3]:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        print("gxe mean-1 %s %s: rel %s, bar %s" % (tag, k, np.abs(b_neg[k][planted] - a[k][planted]) / np.abs(a[k][planted]), tight[k]))
                _records_within(b_neg[planted], a[planted], GXE_FIELDS[3], tight, tag + ("mean-1 rows",))
            else:
                _records_within(b_neg[planted], a[planted], GXE_FIELDS[1], GXE_RTOL, tag + ("mean-1 rows",))
            _records_within(a, ref, GXE_FIELDS[mode], GXE_RTOL, tag + ("oracle",))


# --------------------------------------------------------------------- 5. centring, LOCO, eigenvalue zeroing
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1025])
def test_center_matrix_integer_inputs(api, n):
    """Integer symmetric G: row sums and total are exact.  n a power of two: every step is exact and the result equals the
    reference; otherwise alpha = -1 / n, the two products, beta = d / n^2 and the three additions round: FC.CENTER_ULPS u max |G|."""
    G = FC.int_symmetric(np.random.default_rng(n), n)
    ref = FC.center_reference(G)
    got = api.CenterMatrix(G.copy())
    assert np.array_equal(got, got.T)
    if n & (n - 1) == 0:
        assert np.array_equal(got, ref.astype(np.float64))
    else:
        err = float(np.abs(got.astype(LD) - ref).max())
        print("centre n=%d: max err %.3e, bar %.3e" % (n, err, FC.CENTER_ULPS * U * np.abs(G).max()))
        assert err <= FC.CENTER_ULPS * U * np.abs(G).max()


@pytest.mark.parametrize("n", [64, 257])
def test_center_matrix_mirrors_the_updated_upper_triangle(api, n):
    """A K that is not bit-symmetric: the row sums see the matrix as given, the update is made on the upper triangle, the lower
    triangle is its mirror (csrc/ingest.hip.h, center_update_kernel)"""
    rng = np.random.default_rng(n)
    G = FC.int_symmetric(rng, n)
    G[np.tril_indices(n, -1)] += rng.integers(1, 9, size=n * (n - 1) // 2)
    assert not np.array_equal(G, G.T)
    ref = FC.center_reference(G)
    got = api.CenterMatrix(G.copy())
    assert np.array_equal(got, got.T)
    if n == 64:
        assert np.array_equal(got, ref.astype(np.float64))
    else:
        assert float(np.abs(got.astype(LD) - ref).max()) <= FC.CENTER_ULPS * U * np.abs(G).max()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_loco_combination_is_exact_and_refuses(api, L, n):
    """gemma_hip_kin_loco_d on device buffers: integer inputs with ns_all - ns_chr a power of two are exact; ns_all <= ns_chr is
    refused with EINVAL and leaves the library working"""
    import torch
    rng = np.random.default_rng(n)
    Ka, Kc = rng.integers(-999, 1000, size=(n, n)).astype(np.float64), rng.integers(-999, 1000, size=(n, n)).astype(np.float64)
    fn = L.lib().gemma_hip_kin_loco_d

    def run(nsa, nsc):
        a, c = torch.tensor(Ka, device="cuda"), torch.tensor(Kc, device="cuda")
        L.check(fn(C.c_void_p(a.data_ptr()), nsa, C.c_void_p(c.data_ptr()), nsc, n, api._stream()), "kin_loco")
        torch.cuda.synchronize()
        return c.cpu().numpy(), a.cpu().numpy()

    for nsa, nsc in ((37, 5), (1000, 488), (3, 1)):
        got, a_after = run(nsa, nsc)
        ref = FC.loco_reference(Ka, nsa, Kc, nsc)
        assert np.array_equal(got, ref.astype(np.float64)) and np.array_equal(ref.astype(np.float64).astype(LD), ref)
        assert np.array_equal(a_after, Ka)
    for nsa, nsc in ((5, 5), (4, 9)):
        with pytest.raises(L.GemmaHipError) as e:
            run(nsa, nsc)
        assert e.value.code == L.EINVAL
    got, _ = run(37, 5)
    assert np.array_equal(got, FC.loco_reference(Ka, 37, Kc, 5).astype(np.float64))


@pytest.mark.parametrize("n,seed", [(1, 0), (1, 1), (1, 2), (1, 3), (63, 0), (64, 0), (65, 0), (1025, 0)])
def test_eigenvalue_zeroing_at_the_threshold(api, n, seed):
    """EigenDecomp_Zeroed on a diagonal matrix: 1e-10 itself is kept (the test is <), nextafter(1e-10, 0), a negative value and
    -0.0 come back as +0.  The returned trace is the mean of the values after zeroing: a sum of n terms in the device's order
    ((n - 1) u sum |v|) and one division."""
    D, want, trace = FC.eval_case(n, seed)
    Uo, ev = np.zeros((n, n)), np.zeros(n)
    tr = api.EigenDecomp_Zeroed(D.copy(), Uo, ev)
    edge = want <= 1e-10  # the zeroed values and the one at the threshold: exact, the sign of the zeros included
    assert np.array_equal(ev[edge], want[edge]) and not np.any(np.signbit(ev[edge])), (ev[:6], want[:6])
    if n <= 65:
        assert np.array_equal(ev, want)
    else:  # the large eigenvalues are the eigensolver's (its two-stage form from this size on), within its n u ||A||: not this test's
        print("eval n=%d: max |ev - want| %.3e" % (n, np.abs(ev - want).max()))
        assert np.abs(ev - want).max() <= n * U * want.max()
    assert abs(tr - trace) <= n * U * np.abs(want).sum() / n + U * abs(trace), (tr, trace)


# --------------------------------------------------------------------------------------------------------- 6. -lm
def _lm_check(got, cs, ref, pv, mode, tag):
    n, c = cs["n"], cs["c"]
    exact_zero = c == 1 and n == 64
    assert np.all(got["lambda_remle"] == 0) and np.all(got["lambda_mle"] == 0) and np.all(got["logl_H1"] == 0), tag
    se_ref = ref["se_score"] if mode == 53 else ref["se_wald"]
    for s, kind in enumerate(cs["kinds"]):
        if kind in ("monomorphic", "collinear"):
            # x'P_w x = 0: what the device forms is the rounding residue r of x'x - (W'x)'(W'W)^-1(W'x), |r| <=
            # 64 (n + c^2) u cond(W'W) x'x.  r = 0 makes beta = x'P_w y / 0 and both se non-finite and the LRT statistic NaN; r < 0
            # makes se NaN.  A finite record must be one of a residue under that bound: y'P_w y = (df se^2 + beta^2) r with
            # the Wald se (y'P_wx y = y'P_w y - beta^2 r) and = n se^2 r with the score se (mode 53), so r is recovered from it.
            # A record that was never stored (zeros) or holds ordinary values gives an r far above the bound.
            b, e = got["beta"][s], got["se"][s]
            yPwy = float(ref["se_score"][0] ** 2 * n * ref["xPwx"][0])  # (row 0 is a regular row)
            if exact_zero and kind == "monomorphic":
                # W = 1, n = 64, x = 1: W'x = 64, (W'W)^-1 = 1/64 and x'x = 64 are exact, so r is exactly 0
                print("lm exact-zero record %s: %s" % (tag, got[s]))
                for k in ("beta", "se", "p_wald", "p_score", "p_lrt"):
                    assert not np.isfinite(got[k][s]), (tag, s, k, got[s])
            elif np.isfinite(b) and np.isfinite(e):
                with np.errstate(divide="ignore"):
                    r = yPwy / (n * e * e) if mode == 53 else yPwy / ((n - c - 1) * e * e + b * b)
                bound = 64 * (n + c * c) * U * np.linalg.cond(cs["W"].T @ cs["W"]) * float(ref["xx"][s])
                assert abs(r) <= bound, (tag, s, kind, r, bound, got[s])
            continue
        for k, r in (("beta", ref["beta"][s]), ("se", se_ref[s])):
            rel = abs(float((LD(got[k][s]) - r) / r))
            assert rel <= FC.LM_BAR, (tag, s, kind, k, got[k][s], float(r), rel)
        for k in ("p_wald", "p_score", "p_lrt"):
            p, bar, log10p = pv[k]
            if p[s] < 1e-300:
                assert abs(np.log10(got[k][s]) - log10p[s]) <= 1e-6, (tag, s, k)
            else:
                rel = abs(got[k][s] - p[s]) / p[s]
                assert rel <= bar[s], (tag, s, kind, k, got[k][s], p[s], rel, bar[s])


@pytest.mark.parametrize("nkind,c,l,seed", FC.lm_case_list())
def test_lm_against_long_double_qr(api, L, nkind, c, l, seed):
    """api.LM in modes 51-54, PLINK rows behind an indicator with drops at the byte boundaries and fp64 rows, against OLS by
    long-double QR within FC.LM_BAR (measured on the CPU, see tests/firstpasscases.py).  A monomorphic or collinear row has
    x'P_w x = 0: its record is non-finite where the residue is exactly 0 (c = 1, n = 64) and otherwise non-finite or that of a
    residue under the derived bound, in every mode (_lm_check); its neighbours in the workgroup are regular rows held to the bar."""
    cs = FC.lm_case(nkind, c, l, seed)
    n = cs["n"]
    ref = FC.lm_reference(cs["W"], cs["y"], cs["X"])
    pv = FC.lm_pvalues(ref, n, c)
    raw = FC.pack_bed(FC.geno_to_codes(cs["G"]), ld=(cs["ind"].size + 3) // 4 + (2 if l == 5 else 0), fill=0x55)
    Xw = FC.widen(cs["X"], n + 3, 1e300) if l == 5 else np.ascontiguousarray(cs["X"])
    first = {}
    for mode in (51, 52, 53, 54):
        got_p = api.LM(mode).Analyze(cs["W"], cs["y"], raw, L.GENO_PLINK_2BIT, indicator_idv=cs["ind"], batch=4)
        lm = api.LM(mode)
        got_b = lm.Analyze(cs["W"], cs["y"], Xw, L.GENO_F64_SNP_MAJOR) if l != 5 else _lm_strided(api, L, mode, cs, Xw)
        for enc, got in (("plink", got_p), ("f64", got_b)):
            _lm_check(got, cs, ref, pv, mode, (nkind, c, l, mode, enc))
            for k in ("beta", "p_wald", "p_lrt", "p_score"):  # the mode selects the se and nothing else
                assert _same_bits(got[k], first.setdefault((enc, k), got[k])), (mode, enc, k)


def _lm_strided(api, L, mode, cs, Xw):
    """LM.Analyze makes its input contiguous; the wide row stride goes through the entry points directly"""
    y = np.ascontiguousarray(cs["y"])
    W = np.ascontiguousarray(cs["W"])
    lib = L.lib()
    L.check(lib.gemma_hip_lm_setup(mode, W.shape[0], W.shape[1], C.c_void_p(W.ctypes.data), C.c_void_p(y.ctypes.data)), "lm_setup")
    try:
        out = np.zeros(Xw.shape[0], dtype=api.SUMSTAT_DTYPE)
        L.check(lib.gemma_hip_lm_batch(L.GENO_F64_SNP_MAJOR, C.c_void_p(Xw.ctypes.data), Xw.shape[0], Xw.strides[0] // 8,
                                       C.c_void_p(out.ctypes.data)), "lm_batch")
    finally:
        L.check(lib.gemma_hip_lm_finish(), "lm_finish")
    return out


def test_lm_refusals_leave_the_next_call_working(api, L):
    cs = FC.lm_case(63, 2, 5, 4242)
    good = api.LM(51).Analyze(cs["W"], cs["y"], cs["X"])

    def still_works():
        again = api.LM(51).Analyze(cs["W"], cs["y"], cs["X"])
        for k in again.dtype.names:
            assert _same_bits(again[k], good[k]), k

    rng = np.random.default_rng(1)
    n = 63
    bad = [("c = 17", 51, np.column_stack([rng.standard_normal((n, 16)), np.ones(n)]), cs["y"], cs["X"]),
           ("n = c + 1", 51, np.column_stack([rng.standard_normal(3), np.ones(3)]), cs["y"][:3], cs["X"][:, :3]),
           ("singular W", 51, np.column_stack([np.ones(n), np.ones(n)]), cs["y"], cs["X"]),
           ("a_mode 50", 50, cs["W"], cs["y"], cs["X"]), ("a_mode 55", 55, cs["W"], cs["y"], cs["X"])]
    for tag, mode, W, y, X in bad:
        with pytest.raises(L.GemmaHipError) as e:
            api.LM(mode).Analyze(W, y, np.ascontiguousarray(X))
        assert e.value.code == L.EINVAL, tag
        still_works()
    X = np.ascontiguousarray(cs["X"])
    out = np.zeros(len(X), dtype=api.SUMSTAT_DTYPE)
    rc = L.lib().gemma_hip_lm_batch(L.GENO_F64_SNP_MAJOR, C.c_void_p(X.ctypes.data), X.shape[0], X.shape[1], C.c_void_p(out.ctypes.data))
    assert rc == L.ESTATE  # lm_batch before lm_setup
    still_works()


# ----------------------------------------------------------------------------------------------- 7. carry chain
def _carry_run(api, L, G, ind, Uo, ev, UtW, Uty, batch, extra=0):
    Gall = np.random.default_rng(2).integers(0, 3, size=(len(G), ind.size)).astype(np.float64)
    Gall[:, ind != 0] = G
    raw = _geno(Gall, True, L, extra)[0]
    lmm = api.LMM(a_mode=1)
    lmm.Analyze(Uo, ev, UtW, Uty, raw, L.GENO_PLINK_2BIT, plink=True, indicator_idv=ind, batch=batch)
    return lmm.sumStat


@pytest.mark.parametrize("first_batch_failed", [False, True])
def test_plink_carry_chain_across_batches(api, L, first_batch_failed):
    """AnalyzePlink, mode 1, batches of 4: a failed SNP (all calls missing: logl_H1 is NaN) reports beta-hat and se of the nearest
    preceding successful SNP, across batch boundaries, bit for bit.  When nothing precedes it -- position 0 of the first batch,
    or a first batch that failed throughout -- it reports (0, 0): lmm_setup zeroes the carry buffer the first batch reads
    (csrc/abi_lmm_stage.inc.h).  One batch of all SNPs and batches of 4 give identical records."""
    G, failed = FC.carry_case()
    if first_batch_failed:
        G[:5] = np.nan
        failed = tuple(sorted(set(failed) | set(range(5))))
    n = G.shape[1]
    rng = np.random.default_rng(3)
    Uo, ev = _orthogonal(rng, n)
    y = rng.standard_normal(n) + 0.5 * np.nan_to_num(G[5])
    UtW, Uty = Uo.T @ np.ones((n, 1)), Uo.T @ y
    ind = FC.indicator(n, "every_byte", 3)
    one = _carry_run(api, L, G, ind, Uo, ev, UtW, Uty, batch=len(G))
    four = _carry_run(api, L, G, ind, Uo, ev, UtW, Uty, batch=4, extra=2)  # (and a row stride above the minimum)
    for k in one.dtype.names:
        assert _same_bits(four[k], one[k]), k
    assert tuple(np.flatnonzero(np.isnan(four["logl_H1"]))) == failed
    ok = [s for s in range(len(G)) if s not in failed]
    assert np.all(np.isfinite(four["beta"][ok])) and np.all(four["se"][ok] > 0)
    for s in failed:
        prev = [t for t in ok if t < s]
        want = (four["beta"][prev[-1]], four["se"][prev[-1]]) if prev else (0.0, 0.0)
        assert _same_bits([four["beta"][s], four["se"][s]], want), (s, four["beta"][s], four["se"][s], want)
        assert np.isnan(four["p_wald"][s])

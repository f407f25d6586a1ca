"""MQS summary statistics (-gs, -vc 1 -beta) on the device: the weighted, residualised, category-partitioned kinships
(gemma_hip_mqs_begin / _add / _end / _get), S and its jackknife variance (also gemma_hip_mqs_S alone), and the chain
AnalyzePlink -> Finish -> Calcq -> CalcVCss, against the numpy restatements of tests/mqscases.py, a long-double restatement of the
reference's loops and the reference binary's files (tests/golden/make_mqs_fixtures.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import mqscases as M

pytestmark = pytest.mark.gpu

KIN_BAR = 1e-13  # ||K - ref||_F / ||ref||_F, the bar of the standardised kinship in test_kinship_vs_oracle
LOG_KEYS = ("pve estimates", "se(pve)", "total pve", "se(total pve)", "sigma2 estimates", "se(sigma2)", "enrichment", "se(enrichment)")
API_KEYS = dict(zip(LOG_KEYS, ("pve", "se_pve", "pve_total", "se_pve_total", "sigma2", "se_sigma2", "enrich", "se_enrich")))


@pytest.fixture(scope="module")
def api():
    from gemma_amd import api as A
    A.init(0)
    return A


def frob(K, ref):
    return float(np.linalg.norm(K - ref) / np.linalg.norm(ref))


def device_run(api, c, batch=20000, weight=None, fp64=False, cat=None):
    """one slot 0 session on case dict c -> (MQS object, S, Svar, ns)"""
    m = api.MQS(c["indicator"], c["W"], c["n_vc"])
    cat = c["cat"] if cat is None else cat
    if c["kind"] == "plink" and not fp64:
        m.AnalyzePlink(c["geno"], cat, weight, batch=batch)
    else:
        G = M.decode_bed(c["geno"], c["ni_total"]) if c["kind"] == "plink" else c["geno"]
        m.AnalyzeBimbam(G, cat, weight, batch=batch)
    S, Svar, ns = m.Finish()
    return m, S, Svar, ns


def check_kinships(m, K_ref, ns_ref, tag):
    for i in range(K_ref.shape[0]):
        K = m.Get(0, i)
        if ns_ref[i] == 0:
            assert not K.any(), (tag, i)
        else:
            e = frob(K, K_ref[i])
            print("%s: kinship %d, relative Frobenius distance %.3g" % (tag, i, e))
            assert e < KIN_BAR, (tag, i, e)


# ------------------------------------------------------------------------------------------------ kinship stage
@pytest.mark.parametrize("tag", ["G1", "G2", "G2c", "G3c", "Q3"])
def test_kinships_on_P(api, tag):
    """240 individuals of which 154 are analysed (153 with covariates: three columns of W)"""
    c = M.case(tag)
    K_ref, _, _, ns_ref = M.case_ref(tag)
    m, _, _, ns = device_run(api, c)
    assert np.array_equal(ns, ns_ref)
    check_kinships(m, K_ref, ns_ref, tag)


def synth_case(n_cvt):
    """ni_total = 335 with 301 analysed (not a multiple of 4), 604 SNPs fed as 257 + 257 + 90; 2 % missing; n_vc = 4 with
    category 2 absent from the middle block and category 3 empty throughout; SNPs with cat = -1; SNP 5 monomorphic and SNP 300
    called in one analysed individual only (both dropped, not counted); non-unit weights."""
    rng = np.random.default_rng(335 + n_cvt)
    ni, n, p = 335, 301, 604
    ind = np.ones(ni, dtype=np.int32)
    ind[rng.choice(ni, ni - n, replace=False)] = 0
    G = M.synth_geno(rng, p, ni)
    G[5] = 2.0
    G[300] = np.nan
    G[300, np.flatnonzero(ind)[17]] = 1.0
    G[300, np.flatnonzero(ind == 0)] = rng.integers(0, 3, ni - n)  # called outside the analysed set: must not matter
    cat = rng.choice([0, 1, 2, -1], size=p, p=[0.4, 0.3, 0.2, 0.1]).astype(np.int32)
    mid = np.arange(257, 514)
    cat[mid[cat[mid] == 2]] = 1
    cat[5], cat[300] = 0, 1
    W = np.column_stack([np.ones(n)] + [rng.standard_normal(n) for _ in range(n_cvt - 1)])
    weight = rng.uniform(0.25, 4.0, size=p)
    return dict(kind="plink", geno=M.encode_bed(G), ni_total=ni, indicator=ind, W=np.ascontiguousarray(W), cat=cat, n_vc=4,
                G_test=G[:, ind != 0]), weight


@pytest.mark.parametrize("n_cvt", [1, 3])
def test_kinships_synthetic_blocks_edges(api, n_cvt):
    import torch
    c, weight = synth_case(n_cvt)
    K_ref, ns_ref = M.kin_ref(c["G_test"], c["W"], c["cat"], weight, 4)
    kept = (c["cat"] >= 0).sum()
    assert ns_ref.sum() == kept - 2 and ns_ref[3] == 0 and ns_ref[2] > 0  # the two degenerate SNPs are dropped and not counted
    K_ref = M.center_scale(K_ref)
    m, S, Svar, ns = device_run(api, c, batch=257, weight=weight)
    assert np.array_equal(ns, ns_ref)
    check_kinships(m, K_ref, ns_ref, "synthetic c=%d" % n_cvt)
    assert not S[3].any() and not S[:, 3].any() and not Svar[3].any() and not Svar[:, 3].any()  # the empty category
    Ks = [m.Get(0, i) for i in range(4)]
    # the fp64 SNP-major input with NaN: the same matrices
    m2, S2, Svar2, ns2 = device_run(api, c, batch=257, weight=weight, fp64=True)
    assert np.array_equal(ns2, ns)
    for i in range(3):
        e = frob(m2.Get(0, i), Ks[i])
        print("fp64 rows against 2-bit rows, kinship %d: %.3g" % (i, e))
        assert e < KIN_BAR
    np.testing.assert_allclose(S2, S, rtol=1e-9, atol=0)
    # the device-pointer entry: the same bits as the host-pointer entry
    m3 = api.MQS(c["indicator"], c["W"], 4)
    m3.AnalyzePlink(torch.as_tensor(c["geno"]).cuda(), torch.as_tensor(c["cat"]).cuda(), torch.as_tensor(weight).cuda(), batch=257)
    S3, Svar3, ns3 = m3.Finish()
    assert np.array_equal(ns3, ns) and np.array_equal(S3, S) and np.array_equal(Svar3, Svar)
    for i in range(4):
        assert np.array_equal(m3.Get(0, i), Ks[i]), i


# ------------------------------------------------------------------------------------------------ S and Svar
@pytest.mark.parametrize("tag", M.ALL_TAGS)
def test_S_matches_the_reference_files(api, tag):
    c = M.case(tag)
    _, S, Svar, ns = device_run(api, c)
    fS, fSvar, fns, _ = M.fixture_S(tag)
    np.testing.assert_allclose(S, fS, rtol=1e-9, atol=0)
    np.testing.assert_allclose(Svar, fSvar, rtol=1e-9, atol=0)
    assert np.array_equal(ns, fns)


@pytest.mark.parametrize("n,c", [(61, 1), (128, 3)])
def test_mqs_S_against_the_long_double_loops(api, n, c):
    """gemma_hip_mqs_S on A != K (three categories, the middle one empty).  Bar per block: 16 x max(the float64 numpy error on the
    same inputs, 64 n eps); the margin covers a different summation order."""
    A, K = M.synth_AK(n, c)
    S_ld, V_ld, eS, eV = M.synth_errors(n, c)
    S, Svar = api.MQS.S(A, K, c)
    dS, dV = M.block_err(S, S_ld), M.block_err(Svar, V_ld)
    floor = 64.0 * n * M.EPS
    print("n = %d, c = %d: device error S %.3g, Svar %.3g; numpy %.3g, %.3g; device / max(numpy, 64 n eps) = %.3g, %.3g"
          % (n, c, dS, dV, eS, eV, dS / max(eS, floor), dV / max(eV, floor)))
    assert dS <= M.bar16(eS, n) and dV <= M.bar16(eV, n)


@pytest.mark.parametrize("n_vc", [1, 8])
def test_mqs_S_one_and_eight_categories(api, n_vc):
    n, p = 61, 400
    rng = np.random.default_rng(n_vc)
    G = M.synth_geno(rng, p, n)
    W = np.ones((n, 1))
    K, ns = M.kin_ref(G, W, rng.integers(0, n_vc, p), None, n_vc)
    assert ns.all()
    K = M.center_scale(K)
    S_ld, V_ld = M.brute_force(K, K, 1)
    S_np, V_np = M.closed_form(K, K, 1)
    S, Svar = api.MQS.S(K, K, 1)
    assert M.block_err(S, S_ld) <= M.bar16(M.block_err(S_np, S_ld), n)
    assert M.block_err(Svar, V_ld) <= M.bar16(M.block_err(V_np, V_ld), n)
    assert np.array_equal(S, S.T) and np.array_equal(Svar, Svar.T)


@pytest.mark.parametrize("tag", ["Q2", "Q2c", "Q3", "Q3c"])
def test_whole_chain_against_the_reference_log(api, tag):
    """AnalyzePlink -> Finish -> Calcq -> CalcVCss against the estimate lines of the reference's -vc 1 -beta log (six digits)"""
    c = M.case(tag)
    _, S, Svar, ns = device_run(api, c)
    vec, n_block = M.q_inputs(tag)
    Vq, q, _ = api.Calcq(n_block, vec["vec_cat"], vec["vec_ni"], vec["vec_weight"], vec["vec_z2"], c["n_vc"])
    est = api.CalcVCss(Vq, S, Svar, q, ns, vec["ni_total"])
    log = M.fixture_log(tag)
    for key in LOG_KEYS:
        np.testing.assert_allclose(np.atleast_1d(est[API_KEYS[key]]), [float(x) for x in log[key]], rtol=5e-6, atol=0, err_msg=key)


def test_slot_1_fills_A_beside_the_kept_K(api):
    """The device side of the second CalcS of src/gemma.cpp:2198 on synthetic weights: K from unit weights, then A from other
    weights; S of the pair against the numpy closed form on the numpy matrices."""
    c, weight = synth_case(1)
    c = dict(c, n_vc=3, cat=np.where(c["cat"] == 2, 1, c["cat"]).astype(np.int32))
    K_ref = M.center_scale(M.kin_ref(c["G_test"], c["W"], c["cat"], None, 3)[0])
    A_ref = M.center_scale(M.kin_ref(c["G_test"], c["W"], c["cat"], weight, 3)[0])
    m = api.MQS(c["indicator"], c["W"], 3)
    m.AnalyzePlink(c["geno"], c["cat"], None, slot=0, batch=257)
    m.Finish()
    m.AnalyzePlink(c["geno"], c["cat"], weight, slot=1, batch=257)
    S, Svar, _ = m.Finish()
    for i in range(2):
        assert frob(m.Get(0, i), K_ref[i]) < KIN_BAR and frob(m.Get(1, i), A_ref[i]) < KIN_BAR
    S_np, V_np = M.closed_form(A_ref, K_ref, 1)
    np.testing.assert_allclose(S[:2, :2], S_np[:2, :2], rtol=1e-9, atol=0)
    np.testing.assert_allclose(Svar[:2, :2], V_np[:2, :2], rtol=1e-9, atol=0)
    assert not S[2].any() and not S[:, 2].any()
    assert not np.allclose(S, S.T, rtol=1e-12, atol=0)  # A != K: S is not symmetric


def test_at_size_4099(api):
    """n = 4 099 analysed of 4 200, n_vc = 3, n_cvt = 2, blocks of 1500, 1500 and 701 SNPs: kinships at the Frobenius bar; S and Svar
    against the numpy closed form, whose own error comes from a long-double run of the closed form (the 16 x rule)."""
    rng = np.random.default_rng(4099)
    ni, n, p = 4200, 4099, 3701
    ind = np.ones(ni, dtype=np.int32)
    ind[rng.choice(ni, ni - n, replace=False)] = 0
    G = M.synth_geno(rng, p, ni, miss=0.01)
    cat = rng.integers(0, 3, p).astype(np.int32)
    W = np.ascontiguousarray(np.column_stack([np.ones(n), rng.standard_normal(n)]))
    c = dict(kind="plink", geno=M.encode_bed(G), ni_total=ni, indicator=ind, W=W, cat=cat, n_vc=3)
    K_ref, ns_ref = M.kin_ref(G[:, ind != 0], W, cat, None, 3)
    K_ref = M.center_scale(K_ref)
    m, S, Svar, ns = device_run(api, c, batch=1500)
    assert np.array_equal(ns, ns_ref)
    check_kinships(m, K_ref, ns_ref, "n = 4099")
    S_np, V_np = M.closed_form(K_ref, K_ref, 2)
    S_ld, V_ld = M.closed_form(K_ref, K_ref, 2, dtype=np.longdouble)
    eS, eV = M.block_err(S_np, S_ld), M.block_err(V_np, V_ld)
    dS, dV = M.block_err(S, S_ld), M.block_err(Svar, V_ld)
    floor = 64.0 * n * M.EPS
    print("n = 4099: device error S %.3g, Svar %.3g; numpy %.3g, %.3g; device / max(numpy, 64 n eps) = %.3g, %.3g"
          % (dS, dV, eS, eV, dS / max(eS, floor), dV / max(eV, floor)))
    assert dS <= M.bar16(eS, n) and dV <= M.bar16(eV, n)


def test_two_runs_are_bit_identical(api):
    c, weight = synth_case(3)
    m, S, Svar, ns = device_run(api, c, batch=257, weight=weight)
    Ks = [m.Get(0, i) for i in range(4)]
    m2, S2, Svar2, ns2 = device_run(api, c, batch=257, weight=weight)
    assert np.array_equal(S, S2) and np.array_equal(Svar, Svar2) and np.array_equal(ns, ns2)
    for i in range(4):
        assert np.array_equal(m2.Get(0, i), Ks[i])


# ------------------------------------------------------------------------------------------------ errors and lifetime
def test_rejections_leave_the_library_usable(api):
    import torch
    from gemma_amd import _lib as L
    lib = L.lib()
    c = M.case("G2")
    good = device_run(api, c)[1]

    def still_good():
        assert np.array_equal(device_run(api, c)[1], good)

    ind, W, geno, cat = c["indicator"], c["W"], c["geno"], c["cat"]
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    ld = geno.shape[1]

    def begin(n_vc=2, n_cvt=1, slot=0):
        return lib.gemma_hip_mqs_begin(ind.size, p(ind), n_vc, p(W), n_cvt, slot)

    api.MQS.Release()
    assert lib.gemma_hip_mqs_add(L.GENO_PLINK_2BIT, p(geno), geno.shape[0], ld, p(cat), None) == L.EINVAL  # add before begin
    assert begin(slot=1) == L.EINVAL  # slot 1 without a kept K
    still_good()
    for kw in (dict(n_vc=0), dict(n_vc=9), dict(n_cvt=0), dict(n_cvt=65)):
        assert begin(**kw) == L.EINVAL, kw
        still_good()
    bad = cat.copy()
    bad[7] = 2
    assert begin() == L.OK
    assert lib.gemma_hip_mqs_add(L.GENO_PLINK_2BIT, p(geno), geno.shape[0], ld, p(bad), None) == L.EINVAL  # cat >= n_vc, host
    g_d, bad_d = torch.as_tensor(geno).cuda(), torch.as_tensor(bad).cuda()
    assert lib.gemma_hip_mqs_add_d(L.GENO_PLINK_2BIT, C.c_void_p(g_d.data_ptr()), geno.shape[0], ld, C.c_void_p(bad_d.data_ptr()), None,
                                   None) == L.EINVAL  # cat >= n_vc, found on the device
    # nothing of the rejected blocks was accumulated: the session goes on with the good block
    assert lib.gemma_hip_mqs_add(L.GENO_PLINK_2BIT, p(geno), geno.shape[0], ld, p(cat), None) == L.OK
    S = np.zeros((4, 2))
    assert lib.gemma_hip_mqs_end(p(S), None) == L.OK
    assert np.array_equal(S[:2], good)
    assert begin(n_vc=3, slot=1) == L.EINVAL  # slot 1 with another n_vc than the kept K
    still_good()


def test_release_returns_the_memory_and_a_vc_fit_still_passes(api):
    import torch
    from vccases import HE_CASES, HE_KEYS, fixture
    n, n_vc = 2000, 8
    m = api.MQS(np.ones(n, dtype=np.int32), np.ones((n, 1)), n_vc)
    rng = np.random.default_rng(3)
    m.AnalyzeBimbam(rng.integers(0, 3, (64, n)).astype(np.float64), rng.integers(0, n_vc, 64))
    m.Finish()
    torch.cuda.synchronize()
    held = n_vc * n * n * 8
    before = torch.cuda.mem_get_info()[0]
    api.MQS.Release()
    after = torch.cuda.mem_get_info()[0]
    print("released: %.1f MB of %.1f MB held" % ((after - before) / 1e6, held / 1e6))
    assert after - before >= 0.9 * held
    tag, inputs = HE_CASES[0]
    Ks, W, y = inputs()
    got = api.VC().CalcVChe(Ks, W, y)
    fx = fixture(tag)
    for key, fk in HE_KEYS:
        g = np.atleast_1d(getattr(got, "v_" + key) if hasattr(got, "v_" + key) else getattr(got, key))
        if fk in fx:
            assert np.allclose(g, np.array(fx[fk], dtype=float), rtol=5e-6, atol=0), (key, g, fx[fk])

"""Buffer lifetime of the separately compiled feature units (vc_tu, prdt_tu, mqs_tu) on the device: what their states allocate is
released by gemma_hip_shutdown and comes back, block and staging buffers grow in mid-session, and a refused allocation leaves
the library usable.  Small synthetic cases from the helpers of the feature tests (vccases, prdtcases, mqscases): 70 - 90
individuals, at most 40 SNPs."""
import ctypes as C

import numpy as np
import pytest

import mqscases as M
import prdtcases as pc
import vccases as vc

pytestmark = pytest.mark.gpu

F64, BED = 0, 1  # GEMMA_GENO_F64_SNP_MAJOR, GEMMA_GENO_PLINK_2BIT


def _p(a):
    return C.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------------------------------------ the three small cases
def vc_case():
    """n = 80, two kinships of 20 SNPs each, y with a component of either and noise: (Ks, W, y)"""
    rng = np.random.default_rng(80)
    n = 80
    Ks, y = [], rng.standard_normal(n)
    for _ in range(2):
        X = rng.binomial(2, 0.3, size=(n, 20)).astype(np.float64)
        X -= X.mean(0)
        Ks.append(vc.center_matrix(X @ X.T / 20))
        y += X @ rng.standard_normal(20) * 0.4
    return Ks, np.ones((n, 1)), y


def vc_fit(api):
    Ks, W, y = vc_case()
    he = api.VC().CalcVChe(Ks, W, y)
    re = api.VC().CalcVCreml(Ks, W, y)
    return np.concatenate([he.v_sigma2, he.v_se_sigma2, he.v_pve, he.v_se_pve, [he.pve_total, he.se_pve_total],
                           re.v_sigma2, re.v_se_sigma2, re.v_pve, re.v_se_pve, [re.pve_total, re.se_pve_total, re.iterations, re.status],
                           re.iter_sigma2.ravel()])


def prdt_case():
    """ni = 90 of which 64 are training individuals, 40 SNPs with missing calls: (G, rows, ind)"""
    rng = np.random.default_rng(90)
    ni, l = 90, 40
    G = M.synth_geno(rng, l, ni)
    ind = np.ones(ni, dtype=np.int32)
    ind[rng.choice(ni, 26, replace=False)] = 0
    return G, pc.bed_pack(G), ind


def prdt_fit(api):
    """ridge (-bslmm 2) on the training individuals, then -predict 1 with its effects: alpha, bv, y_prdt"""
    G, rows, ind = prdt_case()
    rng = np.random.default_rng(91)
    Xc = pc.centred_rows(G, ind)
    U, ev, _ = pc.eigen_zeroed(Xc.T @ Xc / G.shape[0])
    y = rng.standard_normal(int(ind.sum()))
    alpha, bv = api.BSLMM().RidgeR(U, ev, U.T @ (y - y.mean()), 0.7, rows, BED, indicator_idv=ind, batch=16)
    rs = ["s%d" % i for i in range(G.shape[0])]
    p = api.PRDT(ind)
    p.AnalyzePlink(rows, rs, dict(zip(rs, alpha)), batch=16)
    return np.concatenate([alpha, bv, p.Finish(y.mean(), 41)])


def mqs_case():
    """ni = 90 with 70 analysed, 25 SNPs in two categories (and two SNPs in none), non-unit weights, two covariates"""
    rng = np.random.default_rng(70)
    ni, n, p = 90, 70, 25
    ind = np.ones(ni, dtype=np.int32)
    ind[rng.choice(ni, ni - n, replace=False)] = 0
    G = M.synth_geno(rng, p, ni)
    cat = rng.integers(0, 2, p).astype(np.int32)
    cat[[4, 19]] = -1
    W = np.ascontiguousarray(np.column_stack([np.ones(n), rng.standard_normal(n)]))
    return dict(geno=M.encode_bed(G), G_test=G[:, ind != 0], indicator=ind, W=W, cat=cat, weight=rng.uniform(0.25, 4.0, size=p), n_vc=2)


def mqs_session(lib, c, cuts):
    """one slot 0 session through the C ABI, the host blocks cut at `cuts`: (S on top of Svar, ns, the kinships)"""
    from gemma_amd import _lib as L
    geno, cat, w, ind, W = c["geno"], c["cat"], c["weight"], c["indicator"], c["W"]
    L.check(lib.gemma_hip_mqs_begin(ind.size, _p(ind), c["n_vc"], _p(W), W.shape[1], 0), "mqs_begin")
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        blk, cb, wb = np.ascontiguousarray(geno[lo:hi]), np.ascontiguousarray(cat[lo:hi]), np.ascontiguousarray(w[lo:hi])
        L.check(lib.gemma_hip_mqs_add(BED, _p(blk), hi - lo, blk.shape[1], _p(cb), _p(wb)), "mqs_add")
    S, ns = np.zeros((2 * c["n_vc"], c["n_vc"])), np.zeros(c["n_vc"])
    L.check(lib.gemma_hip_mqs_end(_p(S), _p(ns)), "mqs_end")
    n = int(ind.sum())
    Ks = np.zeros((c["n_vc"], n, n))
    for i in range(c["n_vc"]):
        L.check(lib.gemma_hip_mqs_get(0, i, _p(Ks[i])), "mqs_get")
    return S, ns, Ks


def mqs_fit(api):
    from gemma_amd import _lib as L
    S, ns, Ks = mqs_session(L.lib(), mqs_case(), [0, 25])
    return np.concatenate([S.ravel(), ns, Ks.ravel()])


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("fit", [vc_fit, prdt_fit, mqs_fit], ids=["vc", "ridge_prdt", "mqs"])
def test_results_across_a_shutdown(gpu_api, fit):
    """fit, gemma_hip_shutdown(), the same fit again in this process: every buffer of the unit was released and comes back, and the
    two results agree bit for bit"""
    from gemma_amd import _lib as L
    first = fit(gpu_api)
    assert np.all(np.isfinite(first))
    L.lib().gemma_hip_shutdown()
    gpu_api.init(0, verbose=0)
    again = fit(gpu_api)
    assert np.array_equal(first, again)


def test_mqs_block_buffers_grow_in_mid_session(gpu_api):
    """Host blocks of 3, then 17, then 5 SNPs in one session: the block and staging buffers are replaced between two adds.  S at
    rtol 1e-9 against the numpy closed form on the numpy kinships and the counts exactly (the bars of tests/test_gpu_mqs.py); the
    same session once more is bit-identical."""
    from gemma_amd import _lib as L
    lib = L.lib()
    c = mqs_case()
    gpu_api.MQS.Release()  # no buffer of an earlier session: the 17-row block has to grow what the 3-row block allocated
    S, ns, Ks = mqs_session(lib, c, [0, 3, 20, 25])
    K_ref, ns_ref = M.kin_ref(c["G_test"], c["W"], c["cat"], c["weight"], c["n_vc"])
    K_ref = M.center_scale(K_ref)
    S_ref, _ = M.closed_form(K_ref, K_ref, c["W"].shape[1])
    assert ns_ref.all() and np.array_equal(ns, ns_ref)
    print("S: max relative difference %.3g" % np.max(np.abs(S[:2] - S_ref) / np.abs(S_ref)))
    np.testing.assert_allclose(S[:2], S_ref, rtol=1e-9, atol=0)
    S2, ns2, Ks2 = mqs_session(lib, c, [0, 3, 20, 25])
    assert np.array_equal(S, S2) and np.array_equal(ns, ns2) and np.array_equal(Ks, Ks2)


@pytest.mark.parametrize("kind", (F64, BED))
def test_ridge_batch_buffers_grow_in_both_forms(gpu_api, kind):
    """ridge_batch with a block of 5 rows and then one of 30 in one fit, host pointers and device pointers: work, staging and
    output buffers grow between the calls.  Every alpha within the dot-product bound of tests/test_gpu_prdt.py."""
    import torch
    G, _, ind = prdt_case()
    G = G[:35]
    rng = np.random.default_rng(35)
    r = rng.standard_normal(int(ind.sum()))
    ref, bound = pc.xtr(G, r, ind)
    blk = pc.bed_pack(G) if kind == BED else np.ascontiguousarray(G)
    for device in (False, True):
        gpu_api.ridge_finish()  # nothing left of an earlier fit
        gpu_api.ridge_set_r(r, 1.0)
        try:
            gpu_api.ridge_set_indicator(ind)
            parts = [torch.from_numpy(b).cuda() if device else b for b in (np.ascontiguousarray(blk[:5]), np.ascontiguousarray(blk[5:]))]
            outs = [gpu_api.ridge_batch(b, kind) for b in parts]
            got = np.concatenate([o.cpu().numpy() if device else o for o in outs])
        finally:
            gpu_api.ridge_finish()
        err = np.abs(got - ref)
        print("kind %d, %s form: max err / bound %.3g" % (kind, "device" if device else "host", np.max(err / np.maximum(bound, 1e-300))))
        assert np.all(err <= bound), (kind, device, int(np.argmax(err - bound)))


def test_a_refused_allocation_leaves_the_library_usable(gpu_api):
    """gemma_hip_mqs_begin for 300 000 individuals and 8 categories asks for 8 n^2 doubles = 5.76 TB in its first allocation, more
    than any device holds: the request is refused at once (nothing is touched), the call returns ENOMEM with the unit's text, and
    a small session afterwards gives what it gave before."""
    from gemma_amd import _lib as L
    lib = L.lib()
    before = mqs_fit(gpu_api)
    n = 300000
    W = np.ones((n, 1))
    rc = lib.gemma_hip_mqs_begin(n, None, 8, _p(W), 1, 0)
    assert rc == L.ENOMEM
    assert lib.gemma_hip_last_error().decode() == "mqs: cannot allocate %d bytes of device memory" % (8 * n * n * 8)
    ind = np.ones(4, dtype=np.int32)
    blk = np.zeros((1, 1), dtype=np.uint8)
    assert lib.gemma_hip_mqs_add(BED, _p(blk), 1, 1, _p(ind), None) == L.EINVAL  # no session was left half open
    assert np.array_equal(mqs_fit(gpu_api), before)

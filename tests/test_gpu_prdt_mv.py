"""Kinship-only prediction for several phenotypes on the device (-m gpu): the assembly of H_oo entry by entry, the factor + solve
path around the 128 block, the Kronecker system against the numpy restatement, the whole block against the files the reference
printed, the delegation of one phenotype, the calls the ABI rejects, and the file driver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import prdtcases as pc
import prdtmvcases as mc

pytestmark = pytest.mark.gpu

EPS = pc.EPS
TAU = 2.7e-13  # see test_whole_block_matches_the_reference_files


def _p(a):
    return a.ctypes.data


def _lib():
    from gemma_amd import _lib as L
    lib = L.lib()
    lib.gemma_hip_dbg_prdt_mv_assemble.argtypes = [C.c_size_t, C.c_size_t] + [C.c_void_p] * 5 + [C.c_size_t]
    lib.gemma_hip_dbg_spd_solve.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_long)]
    return L, lib


def patterns(ni, d, rng):
    full = np.ones((ni, d), dtype=np.int32)
    one_gone = full.copy()
    one_gone[ni // 2] = 0
    scattered = (rng.random((ni, d)) >= 0.3).astype(np.int32)
    one_trait = np.zeros((ni, d), dtype=np.int32)
    one_trait[:, d - 1] = 1
    return (("all observed", full), ("one individual all missing", one_gone), ("scattered 30 % missing", scattered),
            ("one trait ever observed", one_trait))


@pytest.mark.parametrize("d", [2, 3, 8])
@pytest.mark.parametrize("ni", [1, 5, 64, 65, 300])
def test_assembly_entry_by_entry(ni, d, gpu_api):
    """|got - ref| <= 2 eps (|Gc_ij Vg_ab| + |Ve_ab|) on the upper triangle; a guard value everywhere else of an N x (N + 3) array"""
    L, lib = _lib()
    rng = np.random.default_rng(1000 * ni + d)
    X = rng.standard_normal((ni, ni + 3))
    Gc = np.ascontiguousarray(pc.center_matrix(X @ X.T / (ni + 3)))
    A, E = rng.standard_normal((d, d)), rng.standard_normal((d, d))
    Vg, Ve = np.ascontiguousarray(A @ A.T), np.ascontiguousarray(E @ E.T)
    GUARD = -7.25e300
    for what, ind in patterns(ni, d, rng):
        ref, oi, oa = mc.h_oo(Gc, ind, Vg, Ve)
        N = len(oi)
        lda = N + 3
        H = np.full((max(N, 1), lda), GUARD)
        rc = lib.gemma_hip_dbg_prdt_mv_assemble(ni, d, _p(Gc), _p(ind), _p(Vg), _p(Ve), _p(H), lda)
        assert rc == L.OK, (what, lib.gemma_hip_last_error())
        if N == 0:
            assert np.all(H == GUARD), what
            continue
        upper = np.triu(np.ones((N, N), dtype=bool))
        got = H[:N, :N]
        bound = 2 * EPS * (np.abs(Gc[np.ix_(oi, oi)] * Vg[np.ix_(oa, oa)]) + np.abs(Ve[np.ix_(oa, oa)]))
        err = np.abs(got - ref)
        assert np.all(err[upper] <= bound[upper]), (what, float((err - bound)[upper].max()))
        assert np.all(got[~upper] == GUARD) and np.all(H[:, N:] == GUARD), what


def spd_case(N, seed):
    """A = Q diag(lambda) Q' with lambda log-uniform in [1, 1e3], and a right-hand side"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((N, N)))
    lam = np.exp(rng.uniform(0.0, np.log(1e3), N))
    lam[0], lam[-1] = 1.0, 1e3 if N > 1 else 1.0
    A = (Q * lam) @ Q.T
    return np.ascontiguousarray((A + A.T) / 2), rng.standard_normal(N)


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 257, 795])
def test_factor_and_solve_straddle_the_block(N, gpu_api):
    """z against np.linalg.solve at rtol 1e-8, atol 1e-8 max |z|; the inverse of the same matrix applied to r at the same bound"""
    L, lib = _lib()
    A, r = spd_case(N, 77 + N)
    ref = np.linalg.solve(A, r)
    z = r.copy()
    bad = C.c_long(-1)
    Au = np.ascontiguousarray(np.triu(A))  # the upper triangle alone is read
    assert lib.gemma_hip_dbg_spd_solve(_p(Au), N, _p(z), C.byref(bad)) == L.OK, lib.gemma_hip_last_error()
    atol = 1e-8 * np.abs(ref).max()
    print("N = %d: factor + solve %.3g, of max |z| %.3g" % (N, np.abs(z - ref).max(), np.abs(ref).max()))
    assert np.allclose(z, ref, rtol=1e-8, atol=atol)
    Ai = gpu_api.spd_inverse(A.copy())
    assert np.allclose(Ai @ r, ref, rtol=1e-8, atol=atol)
    assert np.array_equal(Ai, Ai.T)
    z2 = r.copy()
    assert lib.gemma_hip_dbg_spd_solve(_p(A), N, _p(z2), C.byref(bad)) == L.OK
    assert np.array_equal(z, z2)  # fixed summation orders: the same bits again, whatever lies below the diagonal


def apply_cases(oracle):
    for tag in sorted(mc.RUNS):
        c, f = mc.inputs(tag), mc.oracle_fit(oracle, tag)
        yield tag, dict(c, Vg=f["Vg"], Ve=f["Ve"], B=f["B"])
    for d, c in ((2, 1), (3, 3), (8, 1), (8, 3)):
        yield "synthetic d = %d, c = %d" % (d, c), mc.synthetic(203, d, c, 40 + 10 * d + c)


def test_apply_matches_the_restatement(gpu_api, oracle):
    import torch
    L, lib = _lib()
    for what, c in apply_cases(oracle):
        ref = mc.mvnorm_prdt_multi(c["G_full"], c["ind"], c["W"], c["Y"], c["Vg"], c["Ve"], c["B"])
        miss = c["ind"] == 0
        Y = gpu_api.PRDT.MvnormApply(c["G_full"], c["ind"], c["W"], c["Y"], c["Vg"], c["Ve"], c["B"])
        print("%s: %d missing, largest difference %.3g of %.3g" % (what, int(miss.sum()), np.abs(Y - ref).max(), np.abs(ref).max()))
        assert np.array_equal(Y[~miss], np.asarray(c["Y"])[~miss]), what
        assert np.allclose(Y, ref, rtol=1e-8, atol=1e-8 * np.abs(ref[miss]).max()), what
        # the device form: a padded kinship on the device, not changed; the same bits
        ni = c["G_full"].shape[0]
        Gp = torch.zeros((ni, ni + 5), dtype=torch.float64, device="cuda")
        Gp[:, :ni] = torch.from_numpy(np.ascontiguousarray(c["G_full"]))
        Yd = gpu_api.PRDT.MvnormApply(Gp[:, :ni], c["ind"], c["W"], c["Y"], c["Vg"], c["Ve"], c["B"])
        assert np.array_equal(Yd, Y), what
        assert np.array_equal(Gp[:, :ni].cpu().numpy(), c["G_full"]), what
    # the order of y_miss through the C entry itself: the synthetic pattern has an individual with two missing traits
    c = mc.synthetic(203, 3, 1, 71)
    ni, d = c["ind"].shape
    assert c["ind"][ni // 2, 0] == 0 and c["ind"][ni // 2, 1] == 0
    ref = mc.mvnorm_prdt_multi(c["G_full"], c["ind"], c["W"], c["Y"], c["Vg"], c["Ve"], c["B"])
    mi, ma = np.nonzero(c["ind"] == 0)  # row-major: i * d + a order
    k = int(np.flatnonzero((mi == ni // 2) & (ma == 0))[0])
    assert mi[k + 1] == ni // 2 and ma[k + 1] == 1 and abs(ref[ni // 2, 0] - ref[ni // 2, 1]) > 1e-3
    y_miss = np.zeros(len(mi))
    G, Yc, ind = (np.ascontiguousarray(c[k_]) for k_ in ("G_full", "Y", "ind"))
    Vg, Ve, B = (np.ascontiguousarray(c[k_]) for k_ in ("Vg", "Ve", "B"))
    assert lib.gemma_hip_prdt_kin_mv_apply(ni, d, _p(G), _p(ind), _p(c["W"]), 1, _p(Yc), _p(Vg), _p(Ve), _p(B), _p(y_miss)) == L.OK
    assert np.allclose(y_miss, ref[mi, ma], rtol=1e-8, atol=1e-8 * np.abs(ref[mi, ma]).max())


def assert_printed_tau(got, ref, what):
    """per entry RTOL_PRINTED |ref| + TAU max |ref|"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    bound = pc.RTOL_PRINTED * np.abs(ref) + TAU * np.abs(ref).max()
    print("%s: %d numbers, largest error / bound %.3g" % (what, ref.size, (err / bound).max()))
    assert np.all(err <= bound), (what, float((err / bound).max()))


@pytest.mark.parametrize("tag", sorted(mc.RUNS))
def test_whole_block_matches_the_reference_files(tag, gpu_api, oracle, tmp_path):
    """gemma_hip_prdt_kin_mv -> WriteFilesFull against the reference's .prdt.txt, Vg / Ve against its log, and at full precision
    against the restatement fed with the RETURNED Vg, Ve, B (rtol 1e-8, atol 1e-8 max |ref|: no tau there).

    Against the printed numbers the per-entry bound is RTOL_PRINTED |ref| + tau max |ref|.  tau covers the device null fit differing
    from the C restatement's (their agreement is pinned to 1e-6 only): four times the largest |device - numpy restatement with the C
    restatement's fit| / max |ref| measured over the three fixtures, capped at RTOL_PRINTED.  Measured on an MI355X: 4.6e-16 (Sb_mv2),
    3.6e-15 (Sb_mv2c), 6.6e-14 (Sb_mv3): the device fit and the C restatement's agree to rounding on these data, so tau = 4 x 6.6e-14 =
    2.7e-13 and the bound is the six printed digits in effect."""
    c = mc.inputs(tag)
    Y, fit = gpu_api.PRDT.MvnormPrdtMulti(c["G_full"], c["ind"], c["W"], c["Y"])
    gpu_api.PRDT.WriteFilesFull(str(tmp_path / "mv.prdt.txt"), Y)
    got = np.array([[float(v) for v in l.split()] for l in open(tmp_path / "mv.prdt.txt") if l.strip()])
    ref, log = mc.fx_prdt(tag), mc.fx_log(tag)
    f0 = mc.oracle_fit(oracle, tag)
    cpu = mc.mvnorm_prdt_multi(c["G_full"], c["ind"], c["W"], c["Y"], f0["Vg"], f0["Ve"], f0["B"])
    print("%s: |device - restatement with the C restatement's fit| / max |ref| = %.3g" % (tag, np.abs(Y - cpu).max() / np.abs(ref).max()))
    assert_printed_tau(got, ref, tag + " Y_full")
    assert_printed_tau(mc.lower(fit["Vg"]), mc.log_lower(log["Vg"]), tag + " Vg")
    assert_printed_tau(mc.lower(fit["Ve"]), mc.log_lower(log["Ve"]), tag + " Ve")
    full = mc.mvnorm_prdt_multi(c["G_full"], c["ind"], c["W"], c["Y"], fit["Vg"], fit["Ve"], fit["B"])
    assert np.allclose(Y, full, rtol=1e-8, atol=1e-8 * np.abs(full).max())


@pytest.mark.parametrize("name,cvt", [("B", False), ("Sb", True)])
def test_one_phenotype_is_handed_to_prdt_kin(name, cvt, gpu_api):
    L, lib = _lib()
    d = pc.load_set(name)
    _, W = pc.m43_inputs(name, cvt)
    K, W = np.ascontiguousarray(pc.kinship_all(d)), np.ascontiguousarray(W)
    ind, y = np.ascontiguousarray(d["ind"], dtype=np.int32), np.ascontiguousarray(d["y_all"])
    ni, m = len(ind), int((ind == 0).sum())
    a, b, fit3, nf = np.zeros(m), np.zeros(m), np.zeros(3), L.MvNull()
    assert lib.gemma_hip_prdt_kin(ni, _p(K), _p(ind), _p(W), W.shape[1], _p(y), 1e-5, 1e5, 10, _p(a), _p(fit3)) == L.OK
    assert lib.gemma_hip_prdt_kin_mv(ni, 1, _p(K), _p(ind), _p(W), W.shape[1], _p(y), 1e-5, 1e5, 10, None, _p(b), C.byref(nf)) == L.OK
    assert m > 0 and np.array_equal(a, b)
    assert nf.Vg_remle[0] == fit3[0] and nf.Ve_remle[0] == fit3[1]


def test_refusals_and_the_call_after(gpu_api):
    L, lib = _lib()
    c = mc.synthetic(40, 2, 1, 5)
    ni = 40
    G, W, Y, ind = (np.ascontiguousarray(c[k]) for k in ("G_full", "W", "Y", "ind"))
    Vg, Ve, B = (np.ascontiguousarray(c[k]) for k in ("Vg", "Ve", "B"))
    out = np.zeros(ni * 9)

    def kin_mv(d, ind_, W_, c_, Y_, out_):
        return lib.gemma_hip_prdt_kin_mv(ni, d, _p(G), _p(ind_), _p(W_), c_, _p(Y_), 1e-5, 1e5, 10, None, out_, None)

    ind9, Y9, I9, B9 = np.ones((ni, 9), dtype=np.int32), np.zeros((ni, 9)), np.eye(9), np.zeros((9, 1))
    ind9[0, 0] = 0
    assert kin_mv(9, ind9, W, 1, Y9, _p(out)) == L.EINVAL
    assert lib.gemma_hip_prdt_kin_mv_apply(ni, 9, _p(G), _p(ind9), _p(W), 1, _p(Y9), _p(I9), _p(I9), _p(B9), _p(out)) == L.EINVAL
    few = np.zeros((ni, 2), dtype=np.int32)  # three complete individuals, three covariates
    few[:3] = 1
    few[3:, 0] = 1
    W3 = np.ascontiguousarray(np.column_stack([np.ones(ni), np.arange(ni) % 3.0, np.arange(ni) % 5.0]))
    assert kin_mv(2, few, W3, 3, Y, _p(out)) == L.EINVAL
    assert kin_mv(2, ind, W, 1, Y, None) == L.EINVAL  # something is missing and y_miss is NULL
    assert lib.gemma_hip_prdt_kin_mv_apply(ni, 2, _p(G), _p(ind), _p(W), 1, _p(Y), _p(Vg), _p(Ve), _p(B), None) == L.EINVAL
    assert lib.gemma_hip_prdt_kin_mv_apply(ni, 2, None, _p(ind), _p(W), 1, _p(Y), _p(Vg), _p(Ve), _p(B), _p(out)) == L.EINVAL
    # nothing missing: OK, and nothing is written
    full = np.ones((ni, 2), dtype=np.int32)
    out[:] = -1.0
    assert lib.gemma_hip_prdt_kin_mv_apply(ni, 2, _p(G), _p(full), _p(W), 1, _p(Y), _p(Vg), _p(Ve), _p(B), None) == L.OK
    # Ve = 0 and two identical individuals: H_oo = Gc (x) Vg is singular.  Every number of this system is a small integer and the
    # pivots are 4, 4, 0 exactly: G's rows sum to zero, so centring leaves it as it is
    G4 = np.array([[4.0, 4, -4, -4], [4, 4, -4, -4], [-4, -4, 8, 0], [-4, -4, 0, 8]])
    ind4 = np.ones((4, 2), dtype=np.int32)
    ind4[3, 1] = 0
    W4, Y4, I2, Z2, B4 = np.ones((4, 1)), np.arange(8.0).reshape(4, 2), np.eye(2), np.zeros((2, 2)), np.zeros((2, 1))
    rc = lib.gemma_hip_prdt_kin_mv_apply(4, 2, _p(G4), _p(ind4), _p(W4), 1, _p(Y4), _p(I2), _p(Z2), _p(B4), _p(out))
    msg = lib.gemma_hip_last_error().decode()
    assert rc == L.ENOTPD and "pivot 2 of 7" in msg, msg
    # the next valid call works
    ref = mc.mvnorm_prdt_multi(G, ind, W, Y, Vg, Ve, B)
    got = gpu_api.PRDT.MvnormApply(G, ind, W, Y, Vg, Ve, B)
    assert np.allclose(got, ref, rtol=1e-8, atol=1e-8 * np.abs(ref).max())


def test_file_driver_reproduces_the_reference_file(gpu_api, tmp_path):
    from gemma_amd import build
    so = build.build()
    exe = str(tmp_path / "prdt_mv_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(pc.ROOT, "include"),
                           os.path.join(pc.ROOT, "tests", "cpp", "prdt_mv_driver.cpp"), "-L" + os.path.dirname(so), "-lgemma_hip", "-lz",
                           "-pthread", "-Wl,-rpath," + os.path.dirname(so), "-o", exe])
    tag = "Sb_mv3"
    K = mc.inputs(tag)["G_full"]
    with open(tmp_path / "K.cXX.txt", "w") as f:  # PARAM::WriteMatrix: ten significant digits, tab separated
        for row in K:
            f.write("\t".join("%.10g" % v for v in row) + "\t\n")
    r = subprocess.run([exe, "-g", os.path.join(pc.FX, "Sb.geno.txt.gz"), "-p", os.path.join(mc.FX, "Sb.pheno3.txt"), "-n", "1", "2", "3",
                        "-k", str(tmp_path / "K.cXX.txt"), "-predict", "1", "-o", tag, "-outdir", str(tmp_path)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.array([[float(v) for v in l.split()] for l in open(tmp_path / (tag + ".prdt.txt")) if l.strip()])
    assert_printed_tau(got, mc.fx_prdt(tag), tag + " Y_full from files")

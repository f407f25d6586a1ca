"""Null fits of a whole phenotype panel (gemma_hip_lmm_null_panel / api.CalcLambdaNullPanel): every column's fit is the single
fit's, bit for bit, in every kernel family, both forms and ragged chunks; the fits against the oracle at the bars of
tests/test_gpu_parity.py::test_null_model; the covariate effects against the oracle's CalcLmmVgVeBeta; no effect on a live
score-panel setup; the argument errors; and tests/cpp/null_panel_file_driver.cpp against the call, against the nulls the score-panel
driver logs and against the reference's log."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import filecases as fc
import multicases as mc
import nullpanelcases as nc
import prdtcases as pc

pytestmark = pytest.mark.gpu
ROOT = nc.ROOT
RTOL, LAM_RTOL = 1e-6, 1e-3  # tests/test_gpu_parity.py
_LOOP, _PANEL = {}, {}


def _bytes_equal(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _loop(api, oracle, n, c, n_region=10):
    """(19, 8): CalcLambdaNull per column, the fit every caller ran before"""
    key = (n, c, n_region)
    if key not in _LOOP:
        _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
        out = np.empty((nc.T, 8))
        for t in range(nc.T):
            f = api.CalcLambdaNull(ev, UtW, np.ascontiguousarray(UtY[:, t]), n_region=n_region, trace_G=float(ev.mean()))
            out[t] = [f[k] for k in nc.FIELDS]
        out.setflags(write=False)
        _LOOP[key] = out
    return _LOOP[key]


def _panel_fit(api, oracle, n, c):
    """(fit (19,) NULL_DTYPE, beta, se_beta) of the host form, beta for c <= 16"""
    key = (n, c)
    if key not in _PANEL:
        _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
        if c <= 16:
            _PANEL[key] = api.CalcLambdaNullPanel(ev, UtW, UtY, trace_G=float(ev.mean()), want_beta=True)
        else:
            _PANEL[key] = (api.CalcLambdaNullPanel(ev, UtW, UtY, trace_G=float(ev.mean())), None, None)
    return _PANEL[key]


def _as8(fit):
    return np.ascontiguousarray(fit).view(np.float64).reshape(-1, 8)


def _dev(a):
    import torch
    return torch.tensor(np.array(a), dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("n,c,n_region", [(n, c, 10) for n, c in nc.BIT_SHAPES] + [(203, 1, 1), (203, 1, 64)])
def test_panel_equals_the_loop_of_single_fits_bit_for_bit(gpu_api, oracle, n, c, n_region):
    """host form and torch _d form, T = 19 (ragged for every workgroup width) and T = 1, all eight fields as bytes (NaN = NaN)"""
    import torch
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    tr = float(ev.mean())
    want = _loop(gpu_api, oracle, n, c, n_region)
    assert np.isnan(want[nc.SPAN]).all() == (c >= 2)  # the span column: NaN for c >= 2, a fit at l_min for c = 1
    assert np.isfinite(want[:len(nc.H2S)]).all()
    host = gpu_api.CalcLambdaNullPanel(ev, UtW, UtY, n_region=n_region, trace_G=tr)
    assert host.dtype == gpu_api.NULL_DTYPE and host.shape == (nc.T,)
    diff = _as8(host).view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), "host form differs from the loop in (column, field) %s" % np.argwhere(diff).tolist()
    dev = gpu_api.CalcLambdaNullPanel(_dev(ev), _dev(UtW), _dev(UtY), n_region=n_region, trace_G=tr)
    assert dev.is_cuda and tuple(dev.shape) == (nc.T, 8)
    torch.cuda.synchronize()
    diff = dev.cpu().numpy().view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), "_d form differs from the loop in (column, field) %s" % np.argwhere(diff).tolist()
    for t in (4, nc.SPAN):  # T = 1: an interior trait and the span column
        one = gpu_api.CalcLambdaNullPanel(ev, UtW, np.ascontiguousarray(UtY[:, t:t + 1]), n_region=n_region, trace_G=tr)
        assert _bytes_equal(_as8(one)[0], want[t]), t
        one_d = gpu_api.CalcLambdaNullPanel(_dev(ev), _dev(UtW), _dev(UtY[:, t:t + 1]), n_region=n_region, trace_G=tr)
        assert _bytes_equal(one_d.cpu().numpy()[0], want[t]), t


def _child(in_path, out_path):
    from gemma_amd import api
    import torch
    z = np.load(in_path)
    ev, UtW, UtY, tr = z["ev"], z["UtW"], z["UtY"], float(z["tr"])
    fit, beta, se = api.CalcLambdaNullPanel(ev, UtW, UtY, trace_G=tr, want_beta=True)
    fd, bd, sd = api.CalcLambdaNullPanel(*(torch.tensor(a, device="cuda") for a in (ev, UtW, UtY)), trace_G=tr, want_beta=True)
    torch.cuda.synchronize()
    np.savez(out_path, fit=_as8(fit), beta=beta, se=se, fit_d=fd.cpu().numpy(), beta_d=bd.cpu().numpy(), se_d=sd.cpu().numpy())


def test_ragged_chunks_give_the_same_bits(gpu_api, oracle, tmp_path):
    """GEMMA_HIP_NULL_PANEL_CHUNK=5 in a fresh process: 19 columns in chunks of 5, 5, 5, 4 -- both forms, fits and covariate effects"""
    n, c = 203, 3
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    np.savez(tmp_path / "in.npz", ev=ev, UtW=UtW, UtY=UtY, tr=float(ev.mean()))
    env = dict(os.environ, GEMMA_HIP_NULL_PANEL_CHUNK="5")
    env["PYTHONPATH"] = ROOT + os.pathsep + os.path.join(ROOT, "tests") + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "child failed:\n%s\n%s" % (r.stdout[-3000:], r.stderr[-3000:])
    got = np.load(tmp_path / "out.npz")
    want = _loop(gpu_api, oracle, n, c)
    fit, beta, se = _panel_fit(gpu_api, oracle, n, c)  # one chunk, this process
    assert _bytes_equal(_as8(fit), want)
    for k in ("fit", "fit_d"):
        assert _bytes_equal(got[k], want), k
    for k, ref in (("beta", beta), ("beta_d", beta), ("se", se), ("se_d", se)):
        assert got[k].shape == (nc.T, c) and _bytes_equal(got[k], ref), k


# ------------------------------------------------------------------------------------------------ 2. oracle
@pytest.mark.parametrize("n,c", nc.ORACLE_SHAPES)
def test_panel_fits_against_the_oracle(gpu_api, oracle, n, c):
    """lambda-hat 1e-3, log-likelihoods 1e-6, pve 1e-4, ve 1e-5, vg 1e-4 (relative): the bars of test_null_model.  se(pve) only
    where the oracle's REML lambda is strictly inside (l_min, l_max) -- on the edge the curvature is a difference of nearly equal
    sums (tests/test_gpu_prdt.py states the exclusion); planted columns by NaN pattern; no other column is left out.  Before the
    bars, the condition on the case: ML fits at l_min, at l_max and inside at n = 203; the (1031, 6) panel is interior but for one fit
    (tests/test_null_panel_cpu.py has the counts), so "each end" cannot be asked of it."""
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    tr = float(ev.mean())
    ref = nc.oracle_fits(oracle, n, c)
    lo, hi, mid = nc.ends(ref[:, 0])
    if (n, c) == (1031, 6):  # interior but for one
        assert lo + hi >= 1 and mid >= 15, (lo, hi, mid)
    else:
        assert lo >= 1 and hi >= 1 and mid >= 1, (lo, hi, mid)
    fit = _panel_fit(gpu_api, oracle, n, c)[0]
    worst = {}
    for t in range(nc.T):
        y = np.ascontiguousarray(UtY[:, t])
        l_mle, logl_mle, l_remle, logl_remle = ref[t]
        got = fit[t]
        if t >= len(nc.H2S):
            pve, pve_se = oracle.calc_pve(ev, UtW, y, l_remle, tr) if np.isfinite(l_remle) else (np.nan, np.nan)
            vg, ve = oracle.calc_vg_ve_beta(ev, UtW, y, l_remle)[:2] if np.isfinite(l_remle) else (np.nan, np.nan)
            want = [l_mle, logl_mle, l_remle, logl_remle, pve, vg, ve]
            mine = [got[k] for k in ("l_mle_null", "logl_mle_H0", "l_remle_null", "logl_remle_H0", "pve", "vg_remle", "ve_remle")]
            assert list(np.isnan(mine)) == list(np.isnan(want)), (t, mine, want)
            continue
        pve, pve_se = oracle.calc_pve(ev, UtW, y, l_remle, tr)
        vg, ve, _, _ = oracle.calc_vg_ve_beta(ev, UtW, y, l_remle)
        pairs = {"l_mle_null": (l_mle, LAM_RTOL), "logl_mle_H0": (logl_mle, RTOL), "l_remle_null": (l_remle, LAM_RTOL),
                 "logl_remle_H0": (logl_remle, RTOL), "pve": (pve, 1e-4), "ve_remle": (ve, 1e-5), "vg_remle": (vg, 1e-4)}
        if nc.L_MIN < l_remle < nc.L_MAX:
            pairs["pve_se"] = (pve_se, 1e-4)
        for k, (w, tol) in pairs.items():
            rel = abs(got[k] - w) / abs(w)
            worst[k] = max(worst.get(k, 0.0), rel)
            print("n=%d c=%d column %d %s: got %.12g oracle %.12g rel %.3g" % (n, c, t, k, got[k], w, rel))
        for k, (w, tol) in pairs.items():
            assert got[k] == pytest.approx(w, rel=tol), (t, k)
    print("n=%d c=%d worst relative differences: %s" % (n, c, worst))


# ------------------------------------------------------------------------------------------------ 3. covariate effects
@pytest.mark.parametrize("n,c", nc.BETA_SHAPES)
def test_covariate_effects_against_the_oracle(gpu_api, oracle, n, c):
    """beta, se(beta) against CalcLmmVgVeBeta at the DEVICE's l_remle_null: |dbeta| <= 1e-6 max(|beta|, se), |dse| <= 1e-6 se.
    The bound is scaled by se because the planted effects are near zero.  Before the bar: cond(UtW' H UtW) < 1e4."""
    import torch
    _, _, ev, UtW, UtY = nc.panel(oracle, n, c)
    fit, beta, se = _panel_fit(gpu_api, oracle, n, c)
    assert beta.shape == se.shape == (nc.T, c)
    worst_b = worst_s = 0.0
    for t in range(len(nc.H2S)):
        lam = float(fit["l_remle_null"][t])
        assert nc.gram_cond(ev, UtW, lam) < nc.COND_MAX, t
        _, _, b, s = oracle.calc_vg_ve_beta(ev, UtW, np.ascontiguousarray(UtY[:, t]), lam)
        eb = np.abs(beta[t] - b) / np.maximum(np.abs(b), s)
        es = np.abs(se[t] - s) / s
        worst_b, worst_s = max(worst_b, float(eb.max())), max(worst_s, float(es.max()))
        assert (eb <= 1e-6).all() and (es <= 1e-6).all(), (t, eb.max(), es.max())
    print("n=%d c=%d: worst |dbeta| / max(|beta|, se) = %.3g, worst |dse| / se = %.3g" % (n, c, worst_b, worst_s))
    if c >= 2:  # the phenotype in the span of the covariates: no lambda, NaN in its own row, the call succeeded
        assert np.isnan(beta[nc.SPAN]).all() and np.isnan(se[nc.SPAN]).all()
    else:
        assert np.isfinite(beta[nc.SPAN]).all() and beta[nc.SPAN, 0] == pytest.approx(1.0, rel=1e-9)
    assert not np.isnan(beta[:len(nc.H2S)]).any()
    fd, bd, sd = gpu_api.CalcLambdaNullPanel(_dev(ev), _dev(UtW), _dev(UtY), trace_G=float(ev.mean()), want_beta=True)
    torch.cuda.synchronize()
    assert _bytes_equal(bd.cpu().numpy(), beta) and _bytes_equal(sd.cpu().numpy(), se) and _bytes_equal(fd.cpu().numpy(), _as8(fit))


# ------------------------------------------------------------------------------------------------ 4. independence
def test_a_live_score_panel_setup_is_not_disturbed(gpu_api, oracle):
    """the null panel between setup_score_panel and batch_score_panel: the block's records are the bytes of a run without it"""
    from gemma_amd import _lib as L
    n, c = 203, 3
    X, U, ev, UtW, UtY = nc.panel(oracle, n, c)
    Y17 = np.ascontiguousarray(UtY[:, :len(nc.H2S)])
    lam = _loop(gpu_api, oracle, n, c)[:len(nc.H2S), 0]
    recs = []
    for between in (False, True):
        lmm = gpu_api.LMM(a_mode=3)
        lmm.setup_score_panel(U, ev, UtW, Y17, lam)
        try:
            if between:
                fit = gpu_api.CalcLambdaNullPanel(ev, UtW, UtY, trace_G=float(ev.mean()), want_beta=True)[0]
                assert _bytes_equal(_as8(fit), _loop(gpu_api, oracle, n, c))
            recs.append(np.array(lmm.batch_score_panel(np.array(X), L.GENO_F64_SNP_MAJOR)))
        finally:
            lmm.finish()
    assert recs[0].shape == (len(nc.H2S), X.shape[0]) and np.isfinite(recs[0]["p_score"]).all()
    assert recs[0].tobytes() == recs[1].tobytes()


# ------------------------------------------------------------------------------------------------ 5. errors
def test_argument_errors(gpu_api):
    from gemma_amd import _lib as L
    lib = L.lib()
    n, c, T = 40, 2, 3
    rng = np.random.default_rng(5)
    ev, UtW, UtY = np.abs(rng.standard_normal(n)), rng.standard_normal((n, 18)), rng.standard_normal((n, T))
    fit, beta, se = np.zeros((T, 8)), np.zeros((T, 18)), np.zeros((T, 18))
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731

    def call(n=n, c=c, T=T, ev=p(ev), W=p(UtW), Y=p(UtY), l_min=1e-5, l_max=1e5, n_region=10, fit=p(fit), beta=None, se=None, d=False):
        if d:
            return lib.gemma_hip_lmm_null_panel_d(n, c, T, ev, W, Y, l_min, l_max, n_region, 1.0, fit, beta, se, None)
        return lib.gemma_hip_lmm_null_panel(n, c, T, ev, W, Y, l_min, l_max, n_region, 1.0, fit, beta, se)

    bad = [dict(T=0), dict(ev=None), dict(W=None), dict(Y=None), dict(fit=None), dict(beta=p(beta)), dict(se=p(se)),
           dict(n=2), dict(n=c), dict(c=0), dict(c=66, n=100), dict(c=17, beta=p(beta), se=p(se)), dict(l_max=1e-5), dict(l_max=1e-6),
           dict(l_max=float("nan")), dict(n_region=0), dict(n_region=65)]
    for kw in bad:
        for d in (False, True):  # the argument checks come before any pointer is followed: host pointers do for the _d form here
            rc = call(d=d, **kw)
            msg = lib.gemma_hip_last_error().decode()
            assert rc == L.EINVAL and "lmm_null_panel" in msg, (kw, d, rc, msg)
    rc = call(n=65535 * 32 + 1)  # more individuals than the transposes' grid holds: refused before any pointer is followed
    assert rc == L.EINVAL and "lmm_null_panel" in lib.gemma_hip_last_error().decode()
    import torch
    e64, W64, Y64 = _dev(ev), _dev(UtW[:, :2]), _dev(UtY)
    with pytest.raises(TypeError):  # a float32 tensor would be read as float64
        gpu_api.CalcLambdaNullPanel(e64, W64, Y64.to(torch.float32))
    with pytest.raises(TypeError):
        gpu_api.CalcLambdaNullPanel(ev, W64, Y64)  # host eval beside device tensors
    with pytest.raises(ValueError):
        gpu_api.CalcLambdaNullPanel(e64[:-1], W64, Y64)
    with pytest.raises(ValueError):
        gpu_api.CalcLambdaNullPanel(ev, UtW[:-1, :2], UtY)
    # beta with 18 covariates is refused, the fit alone at 18 covariates works
    n, c = 203, 18
    ev, UtW, UtY = np.abs(rng.standard_normal(n)), np.ascontiguousarray(rng.standard_normal((n, c))), rng.standard_normal((n, T))
    with pytest.raises(L.GemmaHipError) as e:
        gpu_api.CalcLambdaNullPanel(ev, UtW, UtY, want_beta=True)
    assert e.value.code == L.EINVAL and "lmm_null_panel" in str(e.value)
    fit = gpu_api.CalcLambdaNullPanel(ev, UtW, UtY)
    assert np.isfinite(_as8(fit)[:, :4]).all()
    assert gpu_api.CalcLambdaNullPanel(ev, UtW[:, :16], UtY, want_beta=True)[1].shape == (T, 16)


# ------------------------------------------------------------------------------------------------ 6., 7. from files
@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """(null_panel_file_driver, score_panel_file_driver) built against the library, side by side"""
    from gemma_amd import build
    build.build()
    libdir = os.path.join(ROOT, "gemma_amd")
    d = tmp_path_factory.mktemp("nulldrv")
    exes, procs = [], []
    for name in ("null_panel_file_driver", "score_panel_file_driver"):
        exes.append(str(d / name))
        procs.append(subprocess.Popen(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"),
                                       os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-L" + libdir, "-lgemma_hip",
                                       "-Wl,-rpath," + libdir, "-lz", "-pthread", "-o", exes[-1]]))
    assert [p.wait() for p in procs] == [0, 0]
    return exes


def _read_null(path, c):
    lines = open(path).read().strip().split("\n")
    hdr = "pheno l_mle_null logl_mle_H0 l_remle_null logl_remle_H0 pve se_pve vg ve".split()
    for a in range(c):
        hdr += ["beta_%d" % (a + 1), "se_%d" % (a + 1)]
    assert lines[0].split("\t") == hdr
    rows = [ln.split("\t") for ln in lines[1:]]
    assert all(len(r) == len(hdr) for r in rows)
    for r in rows:
        for txt in r[1:]:
            assert len(txt.split("e")[0].replace("-", "").replace(".", "").lstrip("0")) <= 6, txt  # six significant digits
    return [int(r[0]) for r in rows], np.array([[float(v) for v in r[1:]] for r in rows]), [r[1] for r in rows]


def test_file_driver_equals_the_call_and_the_score_drivers_nulls(gpu_api, drivers, tmp_path):
    """null_panel_file_driver on the phenotype file of a PLINK set with three columns and -c: every line of run.null.txt is
    api.CalcLambdaNullPanel on the driver's own inputs to the print, and its l_mle_null column is, character for character, what
    score_panel_file_driver -- which fits its nulls with the loop of single fits -- logs for the same files"""
    from gemma_amd import _lib as L
    api = gpu_api
    null_drv, score_drv = drivers
    codes, pheno = mc.plink_set()
    ni = codes.shape[1]
    W = np.hstack([np.ones((ni, 1)), np.round(np.random.default_rng(31).standard_normal((ni, 1)), 6)])
    pre = str(tmp_path / "M")
    mc.write_plink(pre, codes, pheno)
    np.savetxt(tmp_path / "pheno.txt", pheno, fmt="%.6f", delimiter="\t")
    np.savetxt(tmp_path / "cvt.txt", W, fmt="%.6f", delimiter="\t")
    raw = mc.pack_bed(codes)
    keep = api.SnpQC(raw, L.GENO_PLINK_2BIT, np.ones(ni, dtype=np.int32), W)[0].astype(bool)
    K10 = api.WriteMatrix10(api.CalcKin(np.ascontiguousarray(raw[keep]), L.GENO_PLINK_2BIT, ni, 1))
    np.savetxt(tmp_path / "K.cXX.txt", K10, fmt="%.10g", delimiter="\t")
    files = ["-p", tmp_path / "pheno.txt", "-c", tmp_path / "cvt.txt", "-k", tmp_path / "K.cXX.txt", "-outdir", tmp_path]
    kv = fc.drive(null_drv, *files, "-o", "run")
    assert int(kv["n_ph"]) == 3 and int(kv["n_cvt"]) == 2 and int(kv["ni_test"]) == ni and int(kv["fits"]) == 3
    K = K10.copy()
    api.CenterMatrix(K)
    U, ev = np.zeros((ni, ni)), np.zeros(ni)
    api.EigenDecomp_Zeroed(K, U, ev)
    fit, beta, se = api.CalcLambdaNullPanel(ev, U.T @ W, U.T @ pheno, trace_G=float(kv["trace_G"]), want_beta=True)
    want = np.hstack([_as8(fit), np.stack([beta, se], axis=2).reshape(3, -1)])
    cols, got, l_mle_text = _read_null(tmp_path / "run.null.txt", 2)
    assert cols == [1, 2, 3]
    pc.assert_printed(got, want, "run.null.txt against CalcLambdaNullPanel")
    fc.drive(score_drv, "-bfile", pre, *files, "-lmm", 3, "-pmax", "0.01", "-o", "scan")
    log = open(tmp_path / "scan.log.txt").read()
    for t, txt in enumerate(l_mle_text):
        assert "## l_mle_null.%d = %s\n" % (t + 1, txt) in log, (t, txt)
    # without -p the phenotype is the .fam file's own column: the first trait again (U^T y is then a product of another shape)
    kv = fc.drive(null_drv, "-bfile", pre, "-c", tmp_path / "cvt.txt", "-k", tmp_path / "K.cXX.txt", "-outdir", tmp_path, "-o", "fam")
    assert int(kv["n_ph"]) == 1
    cols, fam, _ = _read_null(tmp_path / "fam.null.txt", 2)
    assert cols == [1]
    pc.assert_printed(fam, want[:1], "fam.null.txt against CalcLambdaNullPanel")


def test_file_driver_against_the_reference_log(gpu_api, oracle, drivers, tmp_path):
    """tests/golden/null_panel: the three `-lmm 4 -n t` runs of the reference on Sb with Sb.cvt.txt -- both log-likelihoods, pve,
    se(pve), vg, ve, beta, se(beta) of its log against the driver's run.null.txt at the print bound"""
    G = oracle.read_bimbam_geno(os.path.join(pc.FX, "Sb.geno.txt.gz"))[1]
    ni = G.shape[1]
    snp_k = oracle.qc_snps(G, np.ones(ni, dtype=np.int32), np.ones((ni, 1)))[0]  # the fixture's -gk 1 run had the intercept alone
    K10 = oracle.round10(oracle.calc_kin(G[snp_k == 1], 1))  # what the reference's -gk 1 wrote: ten significant digits
    np.savetxt(tmp_path / "K.cXX.txt", K10, fmt="%.10g", delimiter="\t")
    kv = fc.drive(drivers[0], "-p", os.path.join(nc.FX, "Sb3.pheno.txt"), "-c", os.path.join(pc.FX, "Sb.cvt.txt"), "-k", tmp_path / "K.cXX.txt",
                  "-o", "run", "-outdir", tmp_path)
    assert int(kv["n_ph"]) == 3 and int(kv["ni_test"]) == ni == 300 and int(kv["n_cvt"]) == 2
    cols, got, _ = _read_null(tmp_path / "run.null.txt", 2)
    assert cols == [1, 2, 3]
    for t in range(3):
        log = nc.fx_log(t + 1)
        want = [float(log[k]) for k in ("logl_mle_H0", "logl_remle_H0", "pve", "pve_se", "vg", "ve")]
        want += [float(log["beta"][0]), float(log["se_beta"][0]), float(log["beta"][1]), float(log["se_beta"][1])]
        mine = [got[t][1], got[t][3]] + list(got[t][4:])
        pc.assert_printed(mine, want, "column %d against the reference's log" % (t + 1))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        _child(sys.argv[2], sys.argv[3])
    else:
        sys.exit("usage: test_gpu_null_panel.py --child in.npz out.npz")

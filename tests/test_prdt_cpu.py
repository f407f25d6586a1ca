"""Genomic prediction without a GPU: the float64 restatement of the ridge / BLUP fit, the SNP prediction, AddBV and the
kinship-only prediction (tests/prdtcases.py) against the files the reference printed (tests/golden/prdt), the writers of
gemma_amd.api against the same files byte for byte, and the `.param.txt` reader's two column defaults.  Bound for printed
numbers: rtol 5e-6.  The restatement is numpy except for one number: lambda comes from the project's C restatement of the
reference's CalcLambda (oracle.calc_lambda_null), not from the numpy dense search, which is only held to agree with it within the
reference's own stopping rule, |delta lambda| < 1e-5 -- the fixture `fits` says why."""

import numpy as np
import pytest

import prdtcases as pc


@pytest.fixture(scope="module")
def fits(oracle):
    """The numpy ridge fit of every set, once, at the reference's lambda: CalcLambda (Brent in ten regions, then Newton until
    |delta lambda| < 1e-5, src/lmm.cpp:1920-2060) in the project's C restatement.  Measured: that lambda sits 1e-7 (relative)
    beside the exact REML optimum a dense bounded search finds (P 8.2e-8, S 1.2e-7).  With the optimum the restatement differs
    from the printed files by at most 4.2e-6 on P (alpha) but by 1.9e-5 on one SNP of S, whose effect is a cancellation
    residue 2600 times below the largest one and moves 150 times as fast as lambda; with the reference's own lambda the
    largest difference over all four sets is 4.9e-7 (alpha) / 4.6e-7 (bv), the print precision."""
    out = {}
    for name in pc.SETS:
        d = pc.load_set(name)
        keep = d["snp"] == 1
        Xc = pc.centred_rows(d["G"][keep], d["ind"])
        y = d["y_all"][d["ind"] == 1]
        opt = pc.ridge(Xc, y)
        lam = oracle.calc_lambda_null("R", opt["ev"], opt["U"].T @ np.ones((len(y), 1)), opt["Uty"])[0]
        print("%s: lambda of the reference's search %.12g, of the dense search %.12g" % (name, lam, opt["lam"]))
        assert abs(lam - opt["lam"]) <= 1e-5  # the reference ends its Newton steps at |delta lambda| < 1e-5
        out[name] = pc.ridge(Xc, y, lam=lam)
    return out


@pytest.mark.parametrize("name", pc.SETS)
def test_ridge_restatement_matches_the_reference_files(name, fits, oracle):
    d, fit = pc.load_set(name), fits[name]
    rs, alpha = pc.parse_param(pc.fx_text(name + "_R", ".param.txt"))
    assert rs == [d["rs"][i] for i in np.flatnonzero(d["snp"] == 1)]
    log = pc.fx_log(name + "_R")
    assert int(log["number of analyzed SNPs/var"]) == len(rs) and int(log["number of analyzed individuals"]) == int(d["ind"].sum())
    pc.assert_printed(fit["alpha"], alpha, name + " alpha")
    bv, na = pc.parse_column(pc.fx_text(name + "_R", ".bv.txt"))
    assert np.array_equal(na, d["ind"] == 0)
    pc.assert_printed(fit["bv"], bv, name + " bv")
    pc.assert_printed([fit["pheno_mean"]], [float(log["estimated mean"])], name + " estimated mean")


@pytest.mark.parametrize("mode", ("p1", "p2", "p1k", "p2k"))
@pytest.mark.parametrize("name", pc.SETS)
def test_predict_restatement_matches_the_reference_files(name, mode, oracle):
    """from the reference's own printed .param.txt / .bv.txt / estimated mean, as its -predict run read them"""
    d = pc.load_set(name)
    tag = "%s_%s" % (name, mode)
    ebv = mode.endswith("k")
    rs, alpha = pc.parse_param(pc.fx_text(name + "_R", ".param.txt"))
    est = dict(zip(rs, np.zeros(len(rs)) if ebv else alpha))  # with -ebv the alpha column is not read (src/param.cpp:679-682)
    mean = float(pc.fx_log(name + "_R")["estimated mean"])
    kw = {}
    if ebv:
        kw = dict(G_kin=pc.kinship_all(d), u_hat=pc.parse_column(pc.fx_text(name + "_R", ".bv.txt"))[0])
    y, ignored = pc.predict(d["G"], d["rs"], d["ind"], est, mean, probit=mode.startswith("p2"), **kw)
    ref, na = pc.parse_column(pc.fx_text(tag, ".prdt.txt"))
    assert np.array_equal(na, d["ind"] == 1)
    assert ignored == pc.fx_log(tag)["ignored"]
    assert len(est) - len(ignored) == int(pc.fx_log(tag)["number of analyzed SNPs/var"])
    pc.assert_printed(y, ref, tag + " y_prdt")


def test_the_synthetic_set_has_what_the_other_sets_lack():
    d = pc.load_set("S")
    assert pc.fx_log("S_p1")["ignored"] == ["snp7", "snp311"]
    ref, _ = pc.parse_column(pc.fx_text("S_p1", ".prdt.txt"))
    assert len(np.unique(ref)) > 90 and float(pc.fx_log("S_R")["pve estimate in the null model"]) > 0.2
    assert np.array_equal(pc.bed_pack(d["G"]), d["rows"]) and np.array_equal(np.isnan(pc.load_set("Sb")["G"]), np.isnan(d["G"]))


@pytest.mark.parametrize("name", pc.SETS)
def test_writers_reproduce_the_reference_files_byte_for_byte(name, tmp_path, oracle):
    from gemma_amd import api
    d = pc.load_set(name)
    b = api.BSLMM()
    text = pc.fx_text(name + "_R", ".param.txt")
    _, alpha = pc.parse_param(text)
    b.WriteParam(str(tmp_path / "param.txt"), pc.snp_info(d), alpha)
    assert open(tmp_path / "param.txt").read() == text
    text = pc.fx_text(name + "_R", ".bv.txt")
    b.WriteBV(str(tmp_path / "bv.txt"), d["ind"], pc.parse_column(text)[0])
    assert open(tmp_path / "bv.txt").read() == text
    for mode in ("p1", "p2"):
        text = pc.fx_text("%s_%s" % (name, mode), ".prdt.txt")
        p = api.PRDT.__new__(api.PRDT)  # the writer alone: no device state
        p.indicator_idv = d["ind"]
        p.WriteFiles(str(tmp_path / "prdt.txt"), pc.parse_column(text)[0])
        assert open(tmp_path / "prdt.txt").read() == text


def test_log_writer_round_trips_the_estimated_mean(tmp_path):
    from gemma_amd import api
    b = api.BSLMM()
    b.pheno_mean, b.pve_null, b.pve_se_null = 7.7475649, 0.554837, 0.157612
    b.WriteLog(str(tmp_path / "log.txt"))
    assert api.ReadFile_log(str(tmp_path / "log.txt")) == 7.74756
    assert "## pve estimate in the null model = 0.554837\n" in open(tmp_path / "log.txt").read()


def test_param_reader_reproduces_both_column_defaults(tmp_path):
    from gemma_amd import api
    path = str(tmp_path / "x.param.txt")
    open(path, "w").write("chr\trs\tps\tn_miss\talpha\tbeta\tgamma\n"
                          "1\tsA\t10\t0\t1.500000e-01\t0.000000e+00\t0.000000e+00\n"
                          "1\tsB\t20\t3\t-2.000000e-02\t5.000000e-01\t2.500000e-01\n")
    assert api.ReadFile_est(path) == {"sA": 0.15, "sB": -0.02 + 0.5 * 0.25}  # columns 2 5 6 7
    assert api.ReadFile_est(path, have_ebv=True) == {"sA": 0.0, "sB": 0.5 * 0.25}  # 2 0 6 7: alpha is not read
    assert api.ReadFile_est(path, est_column=(2, 5, 0, 0)) == {"sA": 0.15, "sB": -0.02}  # beta 0, gamma 1 when not read
    open(path, "a").write("1\tsA\t10\t0\t1.0\t0.0\t0.0\n")
    with pytest.raises(ValueError):
        api.ReadFile_est(path)
    rs, alpha = pc.parse_param(pc.fx_text("P_R", ".param.txt"))
    real = str(tmp_path / "P.param.txt")
    open(real, "w").write(pc.fx_text("P_R", ".param.txt"))
    est = api.ReadFile_est(real)
    assert list(est) == rs and np.array_equal(np.array(list(est.values())), alpha)
    assert set(api.ReadFile_est(real, have_ebv=True).values()) == {0.0}


@pytest.mark.parametrize("name,cvt", pc.M43_CASES)
def test_kinship_only_prediction_restatement_matches_the_reference_files(name, cvt, oracle):
    """a_mode 43 for one phenotype on the BIMBAM sets (the reference refuses it on PLINK input with -p), with the intercept alone
    and with the synthetic set's covariate file (two covariates), at the reference's lambda as in the ridge fit above"""
    d = pc.load_set(name)
    K = pc.kinship_all(d)
    tag, W = pc.m43_inputs(name, cvt)
    opt = pc.mvnorm_prdt(K, d["ind"], W, d["y_all"])
    lam = oracle.calc_lambda_null("R", opt["ev"], opt["UtW"], opt["Uty"])[0]
    assert abs(lam - opt["lam"]) <= 1e-5  # the reference ends its Newton steps at |delta lambda| < 1e-5
    fit = pc.mvnorm_prdt(K, d["ind"], W, d["y_all"], lam=lam)
    ref = pc.parse_full(pc.fx_text(tag, ".prdt.txt"))
    log = pc.fx_log(tag)
    assert int(log["number of covariates"]) == W.shape[1]
    pc.assert_printed(fit["Y_full"], ref, tag + " Y_full")
    pc.assert_printed([fit["vg"], fit["ve"]], [float(log["vg"]), float(log["ve"])], tag + " vg, ve")


def test_full_writer_reproduces_the_reference_file_byte_for_byte(tmp_path):
    from gemma_amd import api
    text = pc.fx_text("Sb_m43", ".prdt.txt")
    api.PRDT.WriteFilesFull(str(tmp_path / "prdt.txt"), pc.parse_full(text))
    assert open(tmp_path / "prdt.txt").read() == text


@pytest.mark.parametrize("name", ("P", "B"))
def test_cpp_mirror_writers_reproduce_the_reference_files_byte_for_byte(name, tmp_path, oracle):
    """BSLMM::WriteParam / WriteBV and PRDT::WriteFiles of include/gemma_host.hpp, handed the reference's numbers"""
    import subprocess
    d = pc.load_set(name)
    exe = pc.mirror_driver(tmp_path)
    _, alpha = pc.parse_param(pc.fx_text(name + "_R", ".param.txt"))
    with open(tmp_path / "snps.txt", "w") as f:
        for si, a in zip(pc.snp_info(d), alpha):
            f.write("%s %s %s %d %.17g\n" % (si["chr"], si["rs"], si["ps"], si["n_miss"], a))
    bv = iter(pc.parse_column(pc.fx_text(name + "_R", ".bv.txt"))[0])
    open(tmp_path / "bv.txt", "w").write("".join("1 %.17g\n" % next(bv) if k else "0\n" for k in d["ind"]))
    y = iter(pc.parse_column(pc.fx_text(name + "_p1", ".prdt.txt"))[0])
    open(tmp_path / "prdt.txt", "w").write("".join("1\n" if k else "0 %.17g\n" % next(y) for k in d["ind"]))
    subprocess.check_call([exe, "writers", str(tmp_path)])
    assert open(tmp_path / "out.param.txt").read() == pc.fx_text(name + "_R", ".param.txt")
    assert open(tmp_path / "out.bv.txt").read() == pc.fx_text(name + "_R", ".bv.txt")
    assert open(tmp_path / "out.prdt.txt").read() == pc.fx_text(name + "_p1", ".prdt.txt")

"""The two genotype passes of the MQS confidence intervals (-ci 1 / -ci 2) on the device: gemma_hip_ci_begin / _xwz / _xwz_end /
_xtxwz, against the long-double restatement of tests/cicases.py under its error model -- every entry of Xz and XWz within
(L + 8) 2^-53 T, every entry of XtXWz within (n + 8) 2^-53 T, L the number of terms of the entry and T the sum of their absolute
values."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cicases as CI

pytestmark = pytest.mark.gpu

BLOCK = 200  # 523 SNPs go in as 200 + 200 + 123


@pytest.fixture(scope="module")
def api():
    from gemma_amd import api as A
    A.init(0)
    return A


def run(api, c, weighted, batch=BLOCK, fp64=False, dev=False):
    ci = api.CI(c["indicator"], c["n_vc"])
    w = c["w"] if weighted else None
    geno = c["G"] if fp64 else c["bed"]
    if dev:
        import torch
        geno = torch.as_tensor(np.ascontiguousarray(geno)).cuda()
    return (ci.AnalyzeBimbam if fp64 else ci.AnalyzePlink)(geno, c["cat"], c["z"], w, batch=batch)


def check(c, ref, out, tag):
    Xz, XWz, XtXWz, n_skipped = out
    if hasattr(XtXWz, "cpu"):
        XtXWz = XtXWz.cpu().numpy()
    assert n_skipped == int(ref["skipped"].sum())
    r1 = CI.check_pass1(Xz, XWz, ref)
    r2 = CI.check_pass2(XtXWz, c["G_test"], XWz, ref["skipped"])
    print("%s: worst error / bar: pass 1 %.3g, pass 2 %.3g" % (tag, r1, r2))
    return Xz, XWz, XtXWz


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n_vc", [1, 3, 8])
def test_passes_on_the_synthetic_set(api, n_vc, weighted):
    """ni_total = 1030 with 71 individuals dropped (n = 959: no multiple of 4, 16 or 64), 523 SNPs as 200 + 200 + 123, 2 % missing;
    n_vc = 3 has category 1 empty.  One SNP has no called genotype among the analysed individuals, one is monomorphic, one has a
    single called genotype.  The rule of the entry point -- var == 0 is skipped -- takes all three: a single called genotype is
    its own mean, so n_skipped == 3 and all three rows of XtXWz are exactly 0.  The singleton SNP (one heterozygote) is kept."""
    c = CI.synth(n_vc)
    ref = CI.synth_ref(n_vc, weighted)
    sp = c["special"]
    assert ref["skipped"].sum() == 3 and all(ref["skipped"][sp[k]] for k in ("all_missing", "monomorphic", "single_call"))
    Xz, XWz, XtXWz = check(c, ref, run(api, c, weighted), "n_vc=%d w=%s" % (n_vc, weighted))
    assert XtXWz[sp["singleton"]].any()
    if not weighted:
        assert np.array_equal(Xz, XWz)  # -ci 1: XWz = Xz
    if n_vc == 3:
        assert not Xz[:, 1].any() and not XWz[:, 1].any() and not XtXWz[:, 1].any()


@pytest.mark.parametrize("form", ["fp64", "device", "device_fp64"])
def test_equivalent_forms(api, form):
    """the fp64 route on the same data and the _d entry points, under the same bars"""
    c = CI.synth(8)
    check(c, CI.synth_ref(8, True), run(api, c, True, fp64="fp64" in form, dev="device" in form), form)


def test_determinism_and_blocking(api):
    """two runs agree bit for bit; one block of 523 and the three blocks both hold the bars (the sums are real-valued: they need
    not agree bit for bit)"""
    c = CI.synth(8)
    ref = CI.synth_ref(8, True)
    a = run(api, c, True)
    b = run(api, c, True)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    check(c, ref, run(api, c, True, batch=523), "one block")
    check(c, ref, a, "three blocks")


def test_above_one_tile_in_every_dimension(api):
    """n = 4099 of 4200, 3000 SNPs as 2048 + 952, n_vc = 8: more than one workgroup along the individuals (512 per workgroup), more
    than one SNP partition, more than one K group per wavefront in pass 2"""
    c = CI.synth(8, ni_total=4200, n_drop=101, p=3000, miss=0.01)
    ref = CI.pass1(c["G_test"], c["cat"], c["z"], c["w"], 8)
    check(c, ref, run(api, c, True, batch=2048), "n=4099")


def test_rejections_leave_the_library_usable(api):
    from gemma_amd import _lib as L
    lib = L.lib()
    c = CI.synth(3)
    bed, cat, z = c["bed"], c["cat"], c["z"]
    ind = c["indicator"]
    ip = ind.ctypes.data_as(C.c_void_p)
    ld = bed.shape[1]
    out = np.zeros((bed.shape[0], 3))

    def xwz(cat_, ld_=ld):
        return lib.gemma_hip_ci_xwz(L.GENO_PLINK_2BIT, bed.ctypes.data_as(C.c_void_p), bed.shape[0], ld_, cat_.ctypes.data_as(C.c_void_p),
                                    z.ctypes.data_as(C.c_void_p), None, None)

    def xtxwz():
        return lib.gemma_hip_ci_xtxwz(L.GENO_PLINK_2BIT, bed.ctypes.data_as(C.c_void_p), bed.shape[0], ld, out.ctypes.data_as(C.c_void_p))

    api.CI.Release()
    assert xwz(cat) == L.EINVAL and xtxwz() == L.EINVAL and lib.gemma_hip_ci_xwz_end(None, None) == L.EINVAL  # before begin
    assert lib.gemma_hip_ci_begin(ind.size, ip, 9) == L.EINVAL
    assert lib.gemma_hip_ci_begin(ind.size, ip, 3) == L.OK
    assert xtxwz() == L.EINVAL  # pass 2 before xwz_end
    bad = cat.copy()
    bad[100] = 3
    assert xwz(bad) == L.EINVAL
    bad[100] = -1
    assert xwz(bad) == L.EINVAL
    assert xwz(cat, ld - 1) == L.EINVAL  # a row of 1030 individuals takes 258 bytes
    # the session is still open and clean: nothing of the refused blocks was accumulated
    assert xwz(cat) == L.OK
    Xz = np.zeros((c["G_test"].shape[1], 3))
    assert lib.gemma_hip_ci_xwz_end(Xz.ctypes.data_as(C.c_void_p), None) == L.OK
    assert xwz(cat) == L.EINVAL  # pass 1 is over
    assert xtxwz() == L.OK
    ref = CI.synth_ref(3, False)
    CI.check_pass1(Xz, Xz, ref)
    CI.check_pass2(out, c["G_test"], Xz, ref["skipped"])
    api.CI.Release()
    # after ci_release an MQS run of -vc 1 still passes
    import mqscases as M
    mc = M.case("Q2")
    m = api.MQS(mc["indicator"], mc["W"], mc["n_vc"])
    m.AnalyzePlink(mc["geno"], mc["cat"], None)
    S, Svar, ns = m.Finish()
    S_ref, Svar_ref, ns_ref, _ = M.fixture_S("Q2")
    np.testing.assert_allclose(S, S_ref, rtol=1e-9, atol=0)
    assert np.array_equal(ns, ns_ref)
    api.MQS.Release()


def test_device_entry_refuses_a_bad_category_and_accumulates_nothing(api):
    """gemma_hip_ci_xwz_d finds a category outside 0 .. n_vc - 1 on the device (the flag of ci_table_kernel): EINVAL, nothing of
    the block is accumulated, and the same session then takes the good blocks and holds the bars; tensors of the wrong type are
    refused before any call"""
    import torch
    from gemma_amd import _lib as L
    lib = L.lib()
    c = CI.synth(3)
    ref = CI.synth_ref(3, True)
    bed = torch.as_tensor(c["bed"]).cuda()
    z, w = torch.as_tensor(c["z"]).cuda(), torch.as_tensor(c["w"]).cuda()
    good = torch.as_tensor(c["cat"]).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    skipped = C.c_size_t(0)

    def xwz(cat_t, s0, s1):
        return lib.gemma_hip_ci_xwz_d(L.GENO_PLINK_2BIT, C.c_void_p(bed[s0:s1].data_ptr()), s1 - s0, bed.shape[1],
                                      C.c_void_p(cat_t[s0:s1].data_ptr()), C.c_void_p(z[s0:s1].data_ptr()), C.c_void_p(w[s0:s1].data_ptr()),
                                      C.byref(skipped), st)

    ind = c["indicator"]
    assert lib.gemma_hip_ci_begin(ind.size, ind.ctypes.data_as(C.c_void_p), 3) == L.OK
    assert xwz(good, 0, 200) == L.OK
    for v in (3, -1):
        bad = good.clone()
        bad[317] = v
        assert xwz(bad, 200, 400) == L.EINVAL
    assert xwz(good, 200, 400) == L.OK and xwz(good, 400, 523) == L.OK
    n = c["G_test"].shape[1]
    Xz, XWz = np.zeros((n, 3)), np.zeros((n, 3))
    assert lib.gemma_hip_ci_xwz_end(Xz.ctypes.data_as(C.c_void_p), XWz.ctypes.data_as(C.c_void_p)) == L.OK
    CI.check_pass1(Xz, XWz, ref)
    api.CI.Release()
    ci = api.CI(ind, 3)
    with pytest.raises(ValueError):
        ci.AnalyzePlink(bed, good.to(torch.int64), z, w)
    with pytest.raises(ValueError):
        ci.AnalyzePlink(bed, good, z.to(torch.float32), w)
    with pytest.raises(ValueError):
        ci.AnalyzePlink(bed, good, z, w[::2])


# ------------------------------------------------------------------------------------------------ the chains on the reference's runs
@pytest.mark.parametrize("tag", ["C1_2", "C1_2c", "C1_2a", "C2_2", "C2_3c"])
def test_ci_chain_against_the_reference_log(api, tag):
    """readers -> UpdateWeight -> UpdateSNPnZ -> api.CI -> api.CalcCIss against the estimate lines of the reference's -ci log"""
    c, x = CI.case(tag), CI.ci_inputs(tag)
    Xz, XWz, XtXWz, n_skipped = api.CI(c["indicator"], c["n_vc"]).AnalyzePlink(x["bed"], x["vec_cat"], x["z"], x["w_pass"], batch=257)
    assert n_skipped == 0
    est = api.CalcCIss(Xz, XWz, XtXWz, x["S"], x["Svar"], x["w"], x["z"], x["s_vec"], x["vec_cat"], x["pve"])
    CI.check_log(est, tag, CI.LOG_KEYS_CI)


@pytest.mark.parametrize("tag", CI.VC_TAGS)
def test_vc2_beta_chain_against_the_reference(api, tag):
    """-vc 2 -beta: K in slot 0, the LDSC weights from the first round's pve, A through slot 2 (on top of the kept K, as the
    reference's PlinkKin leaves it); the log at six digits, S / Vq / q at 1e-9, size exactly"""
    def calc_S(c, bed, cat, weight, slot):
        m = api.MQS(c["indicator"], c["W"], c["n_vc"])
        m.AnalyzePlink(bed, cat, weight, slot=slot, batch=257)
        return m.Finish()
    est, S2, Vq, q, size = CI.vc2_chain(tag, calc_S)
    CI.check_log(est, tag, CI.LOG_KEYS_VC)
    CI.check_vc2_files(tag, S2, Vq, q, size)
    api.MQS.Release()


# ------------------------------------------------------------------------------------------------ the file driver
@pytest.fixture(scope="module")
def driver(api, tmp_path_factory):
    import mqscases as M
    libdir = os.path.join(M.ROOT, "gemma_amd")
    tmp = tmp_path_factory.mktemp("mqsdrv")
    exe = str(tmp / "mqs_file_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(M.ROOT, "include"),
                           os.path.join(M.ROOT, "tests", "cpp", "mqs_file_driver.cpp"), "-L" + libdir, "-lgemma_hip",
                           "-Wl,-rpath," + libdir, "-lz", "-pthread", "-o", exe])
    pheno = str(tmp / "pheno.txt")  # P.fam's column 6 with -9 written as NA, as the fixtures' runs
    with open(os.path.join(CI.TXT, "P.fam")) as f, open(pheno, "w") as g:
        for line in f:
            v = line.split()[5]
            g.write(("NA" if v == "-9" else v) + "\n")
    return exe, pheno, str(tmp)


def _drive(driver, tag, *args):
    exe, pheno, out = driver
    r = subprocess.run([exe, "-bfile", os.path.join(CI.TXT, "P"), "-p", pheno, "-o", tag, "-outdir", out] + [str(a) for a in args],
                       capture_output=True, text=True, env=dict(os.environ, GEMMA_HIP_IO_BLOCK="257"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    log = {}
    for line in open(os.path.join(out, tag + ".log.txt")):
        if line.startswith("## ") and "=" in line:
            k, v = line[3:].split("=", 1)
            log[k.strip()] = v.split()
    return log, os.path.join(out, tag)


def _same_lines(log, tag, keys):
    want = CI.fixture_log(tag)
    for key in keys:
        np.testing.assert_allclose([float(v) for v in log[key]], [float(v) for v in want[key]], rtol=5e-6, atol=0, err_msg=key)


def test_file_driver_ci(driver):
    """tests/cpp/mqs_file_driver.cpp on C1_2a: files -> first pass -> readers -> PlinkXwz / PlinkXtXwz in blocks of 257 -> CalcCIss"""
    t = lambda name: os.path.join(CI.TXT, name)  # noqa: E731
    log, _ = _drive(driver, "C1_2a", "-cat", t("mqs_cat2.txt"), "-beta", t("ci_beta_a1.txt"), "-ref", t("G2"), "-pve", 0.3, 0.2, "-ci", 1)
    _same_lines(log, "C1_2a", CI.LOG_KEYS_CI)
    assert log["number of analyzed SNPs/var"] == CI.fixture_log("C1_2a")["number of analyzed SNPs/var"].split()
    assert log["number of SNPs/var with a weight"] == [str(len(CI.ci_inputs("C1_2a")["z"]))]
    assert log["number of skipped SNPs/var"] == ["0"]


def test_file_driver_vc2(driver):
    """... and on V2_2: both rounds of -vc 2 -beta, the four files as the reference wrote them"""
    t = lambda name: os.path.join(CI.TXT, name)  # noqa: E731
    log, prefix = _drive(driver, "V2_2", "-cat", t("mqs_cat2.txt"), "-wcat", t("ci_wcat2.txt"), "-beta", t("mqs_beta.txt"), "-vc", 2)
    _same_lines(log, "V2_2", CI.LOG_KEYS_VC)
    rd = lambda p: np.loadtxt(p, ndmin=2)  # noqa: E731
    for suf in (".S.txt", ".Vq.txt", ".q.txt"):
        np.testing.assert_allclose(rd(prefix + suf), rd(t("V2_2" + suf)), rtol=1e-9, atol=0, err_msg=suf)
    assert open(prefix + ".size.txt").read() == open(t("V2_2.size.txt")).read()


def test_file_driver_ci_from_a_bimbam_file(driver, tmp_path):
    """-g / -a on the P set written as a BIMBAM mean-genotype file (rs, minor, major, then the minor-allele counts, NA = missing):
    the first pass, BimbamXwz / BimbamXtXwz in blocks of 257 and CalcCIss give the lines of C1_2a, because the library takes the
    individuals its indicator names"""
    G = CI.decode_bed(np.fromfile(os.path.join(CI.TXT, "P.bed"), dtype=np.uint8)[3:].reshape(800, -1), 240)
    bim = [l.split() for l in open(os.path.join(CI.TXT, "P.bim")) if l.strip()]
    geno, anno = str(tmp_path / "P.geno.txt"), str(tmp_path / "P.anno.txt")
    with open(geno, "w") as f, open(anno, "w") as a:
        for b, row in zip(bim, G):
            f.write(", ".join([b[1], b[4], b[5]] + ["NA" if np.isnan(v) else "%d" % v for v in row]) + "\n")
            a.write("%s, %s, %s\n" % (b[1], b[3], b[0]))
    t = lambda name: os.path.join(CI.TXT, name)  # noqa: E731
    exe, pheno, out = driver
    r = subprocess.run([exe, "-g", geno, "-a", anno, "-p", pheno, "-o", "B1_2a", "-outdir", out, "-cat", t("mqs_cat2.txt"), "-beta",
                        t("ci_beta_a1.txt"), "-ref", t("G2"), "-pve", "0.3", "0.2", "-ci", "1"], capture_output=True, text=True,
                       env=dict(os.environ, GEMMA_HIP_IO_BLOCK="257"))
    assert r.returncode == 0, (r.stdout, r.stderr)
    log = {}
    for line in open(os.path.join(out, "B1_2a.log.txt")):
        if line.startswith("## ") and "=" in line:
            k, v = line[3:].split("=", 1)
            log[k.strip()] = v.split()
    _same_lines(log, "C1_2a", CI.LOG_KEYS_CI)
    assert log["number of SNPs/var with a weight"] == [str(len(CI.ci_inputs("C1_2a")["z"]))]

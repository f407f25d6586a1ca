"""MQS summary statistics (-gs, -vc 1 -beta) without a GPU: the numpy restatement and the exact O(n^2) form of the jackknife
against the reference binary's files (tests/golden/make_mqs_fixtures.py) and against a long-double restatement of the reference's
loops; the C++ host mirror (include/gemma_io_host.hpp) as a stand-alone program; the Python mirror of Calcq / CalcVCss."""
import gzip
import os
import shutil
import subprocess

import numpy as np
import pytest

import mqscases as M

ROOT = M.ROOT
TXT = M.TXT
Q_TAGS = ["Q2", "Q2c", "Q3", "Q3c"]
LOG_KEYS = ("pve estimates", "se(pve)", "total pve", "se(total pve)", "sigma2 estimates", "se(sigma2)", "enrichment", "se(enrichment)")
API_KEYS = dict(zip(LOG_KEYS, ("pve", "se_pve", "pve_total", "se_pve_total", "sigma2", "se_sigma2", "enrich", "se_enrich")))


@pytest.mark.parametrize("tag", M.ALL_TAGS)
def test_closed_form_reproduces_the_reference_files(tag):
    """S and Svar of every fixture at rtol = 1e-9 (the files carry 10 significant digits: half an ulp is 5e-10), size.txt exact."""
    _, S, Svar, ns = M.case_ref(tag)
    fS, fSvar, fns, fn = M.fixture_S(tag)
    np.testing.assert_allclose(S, fS, rtol=1e-9, atol=0)
    np.testing.assert_allclose(Svar, fSvar, rtol=1e-9, atol=0)
    assert np.array_equal(ns, fns) and fn == int(M.case(tag)["indicator"].sum())


def test_closed_form_against_the_long_double_loops_on_P():
    K, S, Svar, _ = M.case_ref("G2")
    S_ld, V_ld = M.brute_force(K, K, 1)
    eS, eV = M.block_err(S, S_ld), M.block_err(Svar, V_ld)
    print("P (n = 154, c = 1): float64 closed form against the long-double loops: S %.3g, Svar %.3g" % (eS, eV))
    assert eS < 1e-7 and eV < 1e-7


@pytest.mark.parametrize("n,c", [(61, 1), (128, 3)])
def test_closed_form_against_the_long_double_loops_synthetic(n, c):
    """A != K, three categories of which the middle one is empty: its rows and columns are exactly 0 in both.  The float64 error
    per block is measured (and kept for the device's bar in tests/test_gpu_mqs.py), asserted only below 1e-7."""
    S_ld, V_ld, eS, eV = M.synth_errors(n, c)
    print("synthetic n = %d, c = %d: float64 closed form against the long-double loops: S %.3g, Svar %.3g" % (n, c, eS, eV))
    assert eS < 1e-7 and eV < 1e-7
    assert np.all(S_ld[1] == 0) and np.all(S_ld[:, 1] == 0) and np.all(V_ld[1] == 0) and np.all(V_ld[:, 1] == 0)
    assert np.all(S_ld[[0, 0, 2, 2], [0, 2, 0, 2]] != 0)
    A, K = M.synth_AK(n, c)
    assert not np.allclose(A[0], K[0])


def test_variance_around_the_mean_is_what_the_reference_means():
    """mean(d^2) - m^2 (src/param.cpp:1697-1701) and the two-pass variance agree in long double; the closed form uses the latter."""
    A, K = M.synth_AK(61, 1)
    _, V_ld = M.brute_force(A, K, 1)
    _, V = M.closed_form(A, K, 1, dtype=np.longdouble)
    assert M.block_err(V, V_ld) < 1e-12


# ------------------------------------------------------------------------------------------------ C++ host mirror
def _build(tmp, flags=()):
    out = os.path.join(str(tmp), "mqs_host_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "mqs_host_check.cpp"), "-lz", "-pthread", "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mqshost"))


def _run_host(exe, tag, tmp):
    snps = os.path.join(str(tmp), tag + ".snps")
    with gzip.open(os.path.join(TXT, "G" + tag[1:] + ".snps.txt.gz"), "rt") as f, open(snps, "w") as g:
        g.write(f.read())
    out = os.path.join(str(tmp), tag)
    r = subprocess.run([exe, os.path.join(TXT, "P.bim"), snps, os.path.join(TXT, M.CAT_FILE[tag[1]]), os.path.join(TXT, "mqs_beta.txt"),
                        os.path.join(TXT, tag + ".S.txt"), os.path.join(TXT, tag + ".size.txt"), "200", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    vals = {}
    for line in r.stdout.splitlines():
        for key in LOG_KEYS + ("q", "Vq", "size"):
            if line.startswith(key + " "):
                vals[key] = np.array([float(x) for x in line[len(key):].split()])
    return vals, out


def _check_host(vals, out, tag):
    q, Vq = np.loadtxt(os.path.join(TXT, tag + ".q.txt")), M.read_matrix(os.path.join(TXT, tag + ".Vq.txt"))
    size = np.loadtxt(os.path.join(TXT, tag + ".size.txt"))
    np.testing.assert_allclose(vals["q"], q, rtol=1e-9, atol=0)
    got_Vq = vals["Vq"].reshape(Vq.shape)
    np.testing.assert_allclose(got_Vq, Vq, rtol=1e-9, atol=0)
    assert np.array_equal(got_Vq == 0, Vq == 0)  # exact zeros stay exact
    assert np.array_equal(vals["size"], size)
    log = M.fixture_log(tag)
    for key in LOG_KEYS:
        np.testing.assert_allclose(vals[key], [float(x) for x in log[key]], rtol=5e-6, atol=0, err_msg=key)
    for suf in (".S.txt", ".Vq.txt", ".q.txt", ".size.txt"):  # the writers: 10 significant digits, as the reference's files
        assert open(out + suf).read() == open(os.path.join(TXT, tag + suf)).read(), suf


@pytest.mark.parametrize("tag", Q_TAGS)
def test_cpp_host_mirror(exe, tag, tmp_path):
    """ReadFile_cat / ReadFile_beta / ObtainWeight / UpdateSNP / Calcq / CalcVCss of include/gemma_io_host.hpp with S from the
    fixture: q, Vq and size at 1e-9 with exact zeros exact, the log's estimate lines at 5e-6 (six printed digits)."""
    vals, out = _run_host(exe, tag, tmp_path)
    _check_host(vals, out, tag)


def test_cpp_host_mirror_under_sanitizers(tmp_path):
    """The same stand-alone program (its own main: no preloading) built with -fsanitize=address,undefined, where g++ links it."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    if subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    exe = _build(tmp_path, flags)
    vals, out = _run_host(exe, "Q3c", tmp_path)
    _check_host(vals, out, "Q3c")


def test_header_spellings(tmp_path):
    """ReadHeader_io's spellings through the Python and the C++ reader: beta + se, chisq and p-value forms of the same z-scores,
    chr:pos in place of rs, n from nobs + nmis."""
    from gemma_amd import api
    rows = [("rs1", "1", "100", 1.5, 150), ("rs2", "1", "200", -0.7, 149), ("rs3", "2", "50", 2.2, 151)]
    from math import erfc, sqrt
    forms = {
        "z": ("SNP Z N", lambda r: "%s %.12g %d" % (r[0], r[3], r[4])),
        "beta": ("MarkerName\tb\tSE\tNOBS\tNMIS", lambda r: "%s\t%.12g\t%.12g\t%d\t%d" % (r[0], r[3] * 0.05, 0.05, r[4] - 3, 3)),
        "chisq": ("rsid,CHISQ,n_total", lambda r: "%s,%.12g,%d" % (r[0], r[3] ** 2, r[4])),
        "p": ("RS PVALUE NTOTAL", lambda r: "%s %.15g %d" % (r[0], erfc(abs(r[3]) / sqrt(2)), r[4])),
        "chrpos": ("CHR BP zscore ncase ncontrol", lambda r: "%s %s %.12g %d %d" % (r[1], r[2], r[3], r[4] - 50, 50)),
    }
    for name, (hdr, fmt) in forms.items():
        path = tmp_path / (name + ".txt")
        path.write_text(hdr + "\n" + "\n".join(fmt(r) for r in rows) + "\n")
        got = api.ReadFile_beta(str(path), {}, {})
        np.testing.assert_allclose(got["vec_z2"], [r[3] ** 2 for r in rows], rtol=1e-9, err_msg=name)
        assert list(got["vec_ni"]) == [r[4] for r in rows] and got["ni_total"] == 151 and got["ns_test"] == 3
    h = api.ReadHeader_io("rs INC_ALLELE DEC_ALLELE a1 catA cont_c")
    assert h["a1_col"] == 4 and h["cat_cols"] == [2, 3, 5, 6]  # the two names the reference's sets leave out are categories there


# ------------------------------------------------------------------------------------------------ Python mirror
@pytest.mark.parametrize("tag", Q_TAGS)
def test_api_calcq_and_calcvcss(tag):
    from gemma_amd import api
    vec, n_block = M.q_inputs(tag)
    S, Svar, ns, _ = M.fixture_S(tag)
    Vq, q, s = api.Calcq(n_block, vec["vec_cat"], vec["vec_ni"], vec["vec_weight"], vec["vec_z2"], len(ns))
    fq, fVq = np.loadtxt(os.path.join(TXT, tag + ".q.txt")), M.read_matrix(os.path.join(TXT, tag + ".Vq.txt"))
    np.testing.assert_allclose(q, fq, rtol=1e-9, atol=0)
    np.testing.assert_allclose(Vq, fVq, rtol=1e-9, atol=0)
    assert np.array_equal(Vq == 0, fVq == 0)
    est = api.CalcVCss(Vq, S, Svar, q, ns, vec["ni_total"])
    log = M.fixture_log(tag)
    for key in LOG_KEYS:
        np.testing.assert_allclose(np.atleast_1d(est[API_KEYS[key]]), [float(x) for x in log[key]], rtol=5e-6, atol=0, err_msg=key)
    assert str(vec["ni_total"]) == log["number of total individuals in the sample"]


def test_new_header_symbols_are_bound():
    import re
    from gemma_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    declared = set(re.findall(r"\b(gemma_hip_mqs_[A-Za-z0-9_]+)\s*\(", hdr))
    assert declared == {"gemma_hip_mqs_begin", "gemma_hip_mqs_add", "gemma_hip_mqs_add_d", "gemma_hip_mqs_end", "gemma_hip_mqs_get",
                        "gemma_hip_mqs_S", "gemma_hip_mqs_S_d", "gemma_hip_mqs_release"}
    assert declared <= set(_lib.SYMBOLS)
    L = _lib.lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None, name
    assert shutil.which("g++")

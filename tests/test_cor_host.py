"""-calccor without a GPU: VARCOV::CalcNB and VARCOV::WriteCov in the Python mirror (gemma_amd/api.py) and the C++ mirror
(include/gemma_io_host.hpp through tests/cpp/cor_host_check.cpp, also under -fsanitize=address,undefined) against the reference
binary's files (tests/golden/make_cor_fixtures.py) and a numpy restatement of the column and of Calc_Cor in fp64
(tests/corcases.py).  Numeric fields are compared at the resolution of the file: |d| <= 1e-6 |ref| + 1e-12."""
import os
import re
import subprocess

import numpy as np
import pytest

import corcases as CC

ROOT = CC.ROOT
TAGS = ["C188ns", "C188bp", "CBXD"]


def inputs(tag):
    """dict(indicator_idv, indicator_snp, chr, cM, bp, G_test (analysed SNPs x analysed individuals, NaN = missing))"""
    if tag == "CBXD":
        d = CC.bxd()
        want = [r["text"][1] for r in CC.golden(tag)]
        ind_snp = np.zeros(len(d["rs"]), dtype=np.int32)
        pos = {r: t for t, r in enumerate(d["rs"])}
        ind_snp[[pos[r] for r in want]] = 1  # the first pass is the device's (tests/test_gpu_cor.py runs it); here: the file's SNPs
        G = d["G"][ind_snp != 0][:, d["indicator_idv"] != 0]
        return dict(indicator_idv=d["indicator_idv"], indicator_snp=ind_snp, chr=d["chr"], cM=d["cM"], bp=d["bp"], G_test=G)
    d = CC.issue188()
    G = CC.decode_bed(d["bed"][d["keep"]], d["ni_total"])[:, d["indicator_idv"] != 0]
    return dict(indicator_idv=d["indicator_idv"], indicator_snp=d["indicator_snp"], chr=d["chr"], cM=d["cM"], bp=d["bp"], G_test=G)


def varcov(api, c, **windows):
    return api.VARCOV(c["indicator_idv"], c["indicator_snp"], c["chr"], c["cM"], c["bp"], **windows)


@pytest.fixture(scope="module")
def api():
    from gemma_amd import api
    return api


# ------------------------------------------------------------------------------------------------------------------- CalcNB
@pytest.mark.parametrize("tag", TAGS)
def test_calcnb_equals_the_window_sizes_of_the_reference(api, tag):
    c = inputs(tag)
    nb = varcov(api, c, **CC.WINDOWS[tag]).CalcNB()
    want = np.array([r["window"] for r in CC.golden(tag)])
    assert np.array_equal(nb[c["indicator_snp"] != 0], want)
    assert not nb[c["indicator_snp"] == 0].any()
    assert np.array_equal(nb, CC.calc_nb(c["indicator_snp"], c["chr"], c["cM"], c["bp"], **CC.WINDOWS[tag]))


#            name                          ind        chr                      cM                       bp               windows              n_nb
SYNTHETIC = [
    ("window_ns cap",                      [1] * 6,   ["1"] * 6,               [0] * 6,                 [1, 2, 3, 4, 5, 6], dict(window_ns=2),   [2, 2, 2, 2, 1, 0]),
    ("cM-only window",                     [1] * 5,   ["1"] * 5,               [0, 0.4, 0.9, 1.0, 1.3], [5, 4, 3, 2, 1],    dict(window_cm=1.0), [2, 3, 2, 1, 0]),
    ("cM = -9 with window_cm != 0",        [1] * 4,   ["1"] * 4,               [0, -9, 0.5, 0.6],       [1, 2, 3, 4],       dict(window_cm=1.0), [3, 0, 1, 0]),
    ("cM = -9 without window_cm",          [1] * 4,   ["1"] * 4,               [0, -9, 0.5, 0.6],       [1, 2, 3, 4],       dict(window_bp=10),  [3, 2, 1, 0]),
    ("bp = -9 with window_bp != 0",        [1] * 4,   ["1"] * 4,               [0] * 4,                 [1, -9, 3, 4],      dict(window_bp=10),  [3, 0, 1, 0]),
    ("chr -9",                             [1] * 5,   ["1", "-9", "-9", "1", "1"], [0] * 5,             [1, 2, 3, 4, 5],    dict(window_bp=10),  [0, 0, 0, 1, 0]),
    ("chromosome change inside a window",  [1] * 5,   ["1", "1", "2", "2", "1"], [0] * 5,               [1, 2, 3, 4, 5],    dict(window_bp=100), [1, 0, 1, 0, 0]),
    ("filtered SNPs between neighbours",   [1, 0, 0, 1, 0, 1, 0], ["1"] * 7,  [0] * 7,                  [1, 2, 3, 4, 5, 6, 7], dict(window_ns=5), [2, 0, 0, 1, 0, 0, 0]),
    ("filtered SNP on another chromosome", [1, 0, 1], ["1", "2", "1"],         [0] * 3,                 [1, 2, 3],          dict(window_ns=5),   [0, 0, 0]),
    ("last SNP, also when it is alone",    [1],       ["1"],                   [0],                     [1],                dict(window_ns=5),   [0]),
    ("all three windows 0: 1 Mb",          [1] * 4,   ["1"] * 4,               [0] * 4,                 [1, 1000000, 1000001, 1000002], dict(), [1, 2, 1, 0]),
    ("bp window is strict",                [1] * 3,   ["1"] * 3,               [0] * 3,                 [10, 15, 20],       dict(window_bp=10),  [1, 1, 0]),
    ("all three windows at once",          [1] * 5,   ["1"] * 5,               [0, 1, 2, 3, 4],         [0, 10, 20, 30, 40], dict(window_cm=2.5, window_bp=25, window_ns=2), [2, 2, 2, 1, 0]),
]


@pytest.mark.parametrize("case", SYNTHETIC, ids=[c[0] for c in SYNTHETIC])
def test_calcnb_branches(api, case):
    """each branch of src/varcov.cpp:168-217; the expected windows are worked out by hand from the definition"""
    _, ind, chr_, cM, bp, win, want = case
    v = api.VARCOV(np.ones(3, dtype=np.int32), ind, chr_, cM, bp, **win)
    assert v.CalcNB().tolist() == want
    assert CC.calc_nb(ind, chr_, cM, bp, **win).tolist() == want
    if not win:
        assert v.window_bp == 1000000  # src/param.cpp:629-630


# ----------------------------------------------------------------------------------------------------------------- WriteCov
@pytest.mark.parametrize("tag", TAGS)
def test_writecov_reproduces_the_reference_files(api, tag, tmp_path):
    c = inputs(tag)
    v = varcov(api, c, **CC.WINDOWS[tag])
    nb = v.CalcNB()[c["indicator_snp"] != 0]
    var, cor, off = CC.calc_cor(c["G_test"], nb)
    info = CC.snpinfo_of(c["G_test"], [r["text"] for r in CC.golden(tag)])
    path = str(tmp_path / (tag + ".cor.txt"))
    v.WriteCov(path, info, var, cor, off)
    CC.compare_file(path, tag)


# ----------------------------------------------------------------------------------------------------------- the C++ mirror
def _build(tmp, flags=()):
    out = os.path.join(str(tmp), "cor_host_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", *flags, "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "cor_host_check.cpp"), "-lz", "-pthread", "-o", out])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("corhost"))


def _write_snps(path, ind, chr_, cM, bp, info=None):
    """one line per SNP of the file; info: snpinfo_of() of the analysed ones"""
    j = 0
    with open(path, "w") as f:
        for t in range(len(ind)):
            if info is not None and ind[t]:
                _, rs, _, n_miss, n_idv, a1, a0, maf = info[j]
                j += 1
            else:
                rs, n_miss, n_idv, a1, a0, maf = "s%d" % t, 0, 0, "A", "C", 0.0
            f.write("%d %s %s %r %d %s %s %d %d %s\n" % (ind[t], chr_[t], rs, float(cM[t]), bp[t], a1, a0, n_miss, n_idv, float(maf).hex()))


def _cpp_nb(exe, tmp, ind, chr_, cM, bp, window_cm=0, window_bp=0, window_ns=0):
    if window_cm == 0 and window_bp == 0 and window_ns == 0:
        window_bp = 1000000  # PARAM::CheckParam's default, set by the caller of VARCOV as in the reference
    snps = os.path.join(str(tmp), "snps.txt")
    _write_snps(snps, ind, chr_, cM, bp)
    r = subprocess.run([exe, "nb", snps, repr(float(window_cm)), str(window_bp), str(window_ns)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [int(v) for v in r.stdout.split()]


def _check_cpp(exe, tmp, tag):
    c = inputs(tag)
    nb_all = _cpp_nb(exe, tmp, c["indicator_snp"], c["chr"], c["cM"], c["bp"], **CC.WINDOWS[tag])
    gold = CC.golden(tag)
    nb = np.array(nb_all)[c["indicator_snp"] != 0]
    assert np.array_equal(nb, [r["window"] for r in gold])
    var, cor, off = CC.calc_cor(c["G_test"], nb)
    info = CC.snpinfo_of(c["G_test"], [r["text"] for r in gold])
    snps, rows = os.path.join(str(tmp), "snps.txt"), os.path.join(str(tmp), "rows.txt")
    _write_snps(snps, c["indicator_snp"], c["chr"], c["cM"], c["bp"], info)
    with open(rows, "w") as f:
        for j in range(len(nb)):
            f.write(" ".join(float(v).hex() for v in [var[j]] + list(cor[off[j]:off[j + 1]])) + "\n")
    r = subprocess.run([exe, "write", snps, rows, str(tmp), tag], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    CC.compare_file(os.path.join(str(tmp), tag + ".cor.txt"), tag)


@pytest.mark.parametrize("tag", TAGS)
def test_cpp_calcnb_and_writecov(exe, tag, tmp_path):
    _check_cpp(exe, tmp_path, tag)


@pytest.mark.parametrize("case", SYNTHETIC, ids=[c[0] for c in SYNTHETIC])
def test_cpp_calcnb_branches(exe, case, tmp_path):
    _, ind, chr_, cM, bp, win, want = case
    assert _cpp_nb(exe, tmp_path, ind, chr_, cM, bp, **win) == want


def test_cpp_host_mirror_under_sanitizers(tmp_path):
    """The same stand-alone program (its own main: no preloading) built with -fsanitize=address,undefined."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]
    # a toolchain that cannot link or run the sanitizers' runtime is a failure here, not a reason to skip: the check is required
    r = subprocess.run(["g++", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    assert r.returncode == 0, "g++ does not link -fsanitize=address,undefined:\n" + r.stderr
    assert subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0
    exe = _build(tmp_path, flags)
    _check_cpp(exe, tmp_path, "C188bp")
    for case in SYNTHETIC:
        assert _cpp_nb(exe, tmp_path, *case[1:5], **case[5]) == case[6], case[0]


# ---------------------------------------------------------------------------------------------------------------------- ABI
def test_new_header_symbols_are_bound():
    from gemma_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    declared = set(re.findall(r"\b(gemma_hip_cor_[A-Za-z0-9_]+)\s*\(", hdr))
    assert declared == {"gemma_hip_cor_begin", "gemma_hip_cor_block", "gemma_hip_cor_block_d", "gemma_hip_cor_release"}
    assert declared <= set(L.SYMBOLS)
    assert re.search(r"#define\s+GEMMA_HIP_ABI_VERSION\s+4\b", hdr)  # additive: the version stays

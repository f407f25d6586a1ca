"""-calccor on the device: gemma_hip_cor_begin / _block / _block_d / _release and api.VARCOV against the reference binary's files
(tests/golden/make_cor_fixtures.py), the exact value of the integer route from Python integers, a long-double restatement for the
fp64 route (tests/corcases.py), and the file-driven run through tests/cpp/cor_file_driver.cpp."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import corcases as CC

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EXACT_RTOL = 8 * U  # the combine is five correctly rounded operations (<= 2.25 ulp); the bar is twice that, rounded up


@pytest.fixture(scope="module")
def api(gpu_api):
    return gpu_api


def _p(a):
    return C.c_void_p(a.ctypes.data)


def run_plink(api, G, n_nb, indicator=None, batch=20000):
    """G: analysed SNPs x ALL individuals of 0 / 1 / 2 / NaN -> (var, cor, off) through the .bed route"""
    ind = np.ones(G.shape[1], dtype=np.int32) if indicator is None else indicator
    p = G.shape[0]
    v = api.VARCOV(ind, np.ones(p, dtype=np.int32), ["1"] * p, np.zeros(p), np.arange(p), window_ns=1)
    v.n_nb = np.asarray(n_nb, dtype=np.int32)
    return v.AnalyzePlink(CC.encode_bed(G), batch=batch)


def run_f64(api, G, n_nb, indicator=None, batch=20000):
    ind = np.ones(G.shape[1], dtype=np.int32) if indicator is None else indicator
    p = G.shape[0]
    v = api.VARCOV(ind, np.ones(p, dtype=np.int32), ["1"] * p, np.zeros(p), np.arange(p), window_ns=1)
    v.n_nb = np.asarray(n_nb, dtype=np.int32)
    return v.AnalyzeBimbam(np.ascontiguousarray(G, dtype=np.float64), batch=batch)


def windows(rng, p, hi=200):
    """random in 0 .. hi, inside the block: zero windows, windows wider than a tile, windows that end at the last row"""
    nb = np.minimum(rng.integers(0, hi + 1, size=p), p - 1 - np.arange(p)).astype(np.int32)
    nb[rng.random(p) < 0.1] = 0
    nb[5] = min(hi, p - 1 - 5)
    nb[p - 2] = 1  # ends at the last row
    return nb


def hard_calls(seed, n, p=300, miss=0.0):
    """p SNPs over n individuals; SNP 10 has a single called genotype, SNP 11 none, SNP 12 is monomorphic"""
    rng = np.random.default_rng(seed)
    af = rng.uniform(0.05, 0.5, size=p)
    G = rng.binomial(2, af[:, None], size=(p, n)).astype(np.float64)
    G[rng.random((p, n)) < miss] = np.nan
    G[10] = np.nan
    G[10, n // 2] = 2
    G[11] = np.nan
    G[12] = np.where(np.isnan(G[12]), np.nan, 1.0)
    return G, windows(rng, p)


# ------------------------------------------------------------------------------------------------------------------ goldens
def _check_records(tag, nb, var, cor, off):
    want = CC.golden(tag)
    assert len(nb) == len(want)
    assert np.array_equal(nb, [r["window"] for r in want])
    assert CC.close_to_print(var, [r["var"] for r in want])
    assert CC.close_to_print(cor, np.concatenate([r["cor"] for r in want]))
    assert off[-1] == cor.size


@pytest.mark.parametrize("tag", ["C188ns", "C188bp"])
def test_issue188_against_the_reference_file(api, tag):
    """n = 876 = 13 * 64 + 44 analysed of 1 008 individuals (the indicator map of the ingest), real missing calls"""
    d = CC.issue188()
    v = api.VARCOV(d["indicator_idv"], d["indicator_snp"], d["chr"], d["cM"], d["bp"], **CC.WINDOWS[tag])
    nb = v.CalcNB()[d["indicator_snp"] != 0]
    var, cor, off = v.AnalyzePlink(d["bed"][d["keep"]])
    _check_records(tag, nb, var, cor, off)


def test_bxd_against_the_reference_file(api, tmp_path):
    """BIMBAM dosages, 67 of 198 individuals analysed, 20 chromosomes; the first pass on the device; WriteCov on the result"""
    from gemma_amd import _lib as L
    d = CC.bxd()
    ind_snp, maf, n_miss = api.SnpQC(d["G"], L.GENO_F64_SNP_MAJOR, d["indicator_idv"], np.ones((int(d["indicator_idv"].sum()), 1)))
    v = api.VARCOV(d["indicator_idv"], ind_snp, d["chr"], d["cM"], d["bp"], **CC.WINDOWS["CBXD"])
    keep = ind_snp != 0
    nb = v.CalcNB()[keep]
    var, cor, off = v.AnalyzeBimbam(d["G"][keep])
    _check_records("CBXD", nb, var, cor, off)
    ni_test = int(d["indicator_idv"].sum())
    info = [(d["chr"][t], d["rs"][t], int(d["bp"][t]), int(n_miss[t]), ni_test - int(n_miss[t]), d["a1"][t], d["a0"][t], maf[t])
            for t in np.nonzero(keep)[0]]
    path = str(tmp_path / "CBXD.cor.txt")
    v.WriteCov(path, info)
    CC.compare_file(path, "CBXD")


@pytest.fixture(scope="module")
def driver(api, tmp_path_factory):
    libdir = os.path.join(CC.ROOT, "gemma_amd")
    exe = str(tmp_path_factory.mktemp("cordrv") / "cor_file_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(CC.ROOT, "include"),
                           os.path.join(CC.ROOT, "tests", "cpp", "cor_file_driver.cpp"), "-L" + libdir, "-lgemma_hip",
                           "-Wl,-rpath," + libdir, "-lz", "-pthread", "-o", exe])
    return exe


def _drive(exe, block, *args):
    return subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, GEMMA_HIP_IO_BLOCK=str(block)))


def test_file_driver_writes_the_reference_file(driver, tmp_path):
    """tests/cpp/cor_file_driver.cpp: .bed / .bim / .fam -> first pass -> CalcNB -> blocks of 500 outputs with their halos -> WriteCov"""
    pre = str(tmp_path / "i188")
    CC.write_issue188_plink(pre)
    r = _drive(driver, 500, "-bfile", pre, "-calccor", "-windowbp", 300, "-o", "drv", "-outdir", tmp_path)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "ns_test=1850" in r.stdout
    CC.compare_file(str(tmp_path / "drv.cor.txt"), "C188bp")


def test_file_driver_bimbam_feeder_writes_the_reference_file(driver, tmp_path):
    """-g / -p / -a on the BXD text files: VARCOV::AnalyzeBimbam in blocks of 1 000 outputs, the text file opened again for every
    block and the lines in front of it dropped"""
    r = _drive(driver, 1000, "-g", os.path.join(CC.TXT, "bxd_mean_genotypes.txt.gz"), "-p", os.path.join(CC.TXT, "bxd_trait.txt.gz"),
               "-a", os.path.join(CC.TXT, "bxd_anno.txt.gz"), "-calccor", "-windowbp", CC.WINDOWS["CBXD"]["window_bp"], "-o", "bx",
               "-outdir", tmp_path)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "ns_test=%d" % len(CC.golden("CBXD")) in r.stdout
    CC.compare_file(str(tmp_path / "bx.cor.txt"), "CBXD")


def test_file_driver_fails_on_a_truncated_bed(driver, tmp_path):
    """a .bed 100 rows short of its .bim: non-zero exit and no success line (the first pass meets the short file before the feeder
    does; the feeder sets VARCOV::error on the same condition and the driver leaves with status 3 on it)"""
    pre = str(tmp_path / "i188")
    CC.write_issue188_plink(pre)
    size = os.path.getsize(pre + ".bed")
    with open(pre + ".bed", "r+b") as f:
        f.truncate(size - 100 * 252)
    r = _drive(driver, 500, "-bfile", pre, "-calccor", "-windowbp", 300, "-o", "cut", "-outdir", tmp_path)
    assert r.returncode != 0
    assert "out=" not in r.stdout


# -------------------------------------------------------------------------------------------------------- the integer route
def _check_exact(G, nb, var, cor, off):
    var_x, cor_x, off_x = CC.exact_cor(G, nb)
    assert np.array_equal(off, off_x)
    c = ~np.isnan(G)
    N = c.sum(1)
    g = np.where(c, G, 0)
    D = N * (g * g).sum(1) - g.sum(1) ** 2
    assert np.array_equal(np.isnan(var), N[:len(nb)] == 0)  # 0 / 0 exactly where no genotype is called
    bad = (N == 0) | (D == 0)
    pair_bad = np.concatenate([bad[t] | bad[t + 1:t + 1 + w] for t, w in enumerate(nb)] + [np.zeros(0, dtype=bool)])
    assert np.array_equal(np.isnan(cor), pair_bad)  # NaN exactly where N = 0 or D = 0
    assert np.array_equal(np.isnan(cor_x), pair_bad)
    fv, fc = ~np.isnan(var), ~pair_bad
    ev = np.abs(var[fv] - var_x[fv]) / np.where(var_x[fv] == 0, 1.0, np.abs(var_x[fv]))
    ec = np.abs(cor[fc] - cor_x[fc]) / np.where(cor_x[fc] == 0, 1.0, np.abs(cor_x[fc]))
    print("exact: worst var %.3g ulp, worst cor %.3g ulp over %d correlations" % (ev.max() / U, ec.max() / U if ec.size else 0.0, ec.size))
    assert ev.max() <= EXACT_RTOL
    assert ec.size == 0 or ec.max() <= EXACT_RTOL
    assert np.all(cor[fc][cor_x[fc] == 0] == 0)


@pytest.mark.parametrize("miss", [0.0, 0.05, 0.5])
@pytest.mark.parametrize("n", [5, 63, 64, 65, 1000])
def test_integer_route_is_exact_and_repeats(api, n, miss):
    """Every finite r and var within 8 * 2^-53 relative of the value from Python integers rounded once; NaN exactly where N = 0
    or D = 0; a second run agrees bit for bit."""
    G, nb = hard_calls(1000 * n + int(100 * miss), n, miss=miss)
    var, cor, off = run_plink(api, G, nb)
    _check_exact(G, nb, var, cor, off)
    var2, cor2, _ = run_plink(api, G, nb)
    assert var.tobytes() == var2.tobytes() and cor.tobytes() == cor2.tobytes()


def test_integer_route_with_an_indicator_map(api):
    """40 of 105 individuals dropped: the map path of the ingest against the same exact value"""
    G, nb = hard_calls(77, 105, miss=0.05)
    ind = np.ones(105, dtype=np.int32)
    ind[np.random.default_rng(3).choice(105, 40, replace=False)] = 0
    var, cor, off = run_plink(api, G, nb, indicator=ind)
    _check_exact(G[:, ind != 0], nb, var, cor, off)


@pytest.mark.parametrize("n", [65, 1000])
def test_block_split_changes_no_bit(api, n):
    """one call against blocks of 70 outputs with their halos"""
    for miss in (0.0, 0.05):
        G, nb = hard_calls(5 * n + int(100 * miss), n, miss=miss)
        var, cor, off = run_plink(api, G, nb)
        var_b, cor_b, off_b = run_plink(api, G, nb, batch=70)
        assert np.array_equal(off, off_b)
        assert var.tobytes() == var_b.tobytes() and cor.tobytes() == cor_b.tobytes()


@pytest.mark.parametrize("n", [65, 1000])
def test_complete_tiles_and_masked_tiles_agree_bit_for_bit(api, n):
    """data without a missing call (every tile pair runs P1 alone) against the same data with one missing call planted in one SNP
    of every tile (every tile pair runs the four products), on the pairs that do not involve a planted SNP"""
    rng = np.random.default_rng(n)
    p = 300
    G = rng.binomial(2, rng.uniform(0.05, 0.5, size=p)[:, None], size=(p, n)).astype(np.float64)
    nb = windows(rng, p)
    var, cor, off = run_plink(api, G, nb)
    assert not np.isnan(var).any()
    Gm = G.copy()
    planted = np.arange(3, p, 64)
    Gm[planted, rng.integers(0, n, size=planted.size)] = np.nan
    var_m, cor_m, _ = run_plink(api, Gm, nb)
    touched = np.zeros(p, dtype=bool)
    touched[planted] = True
    pair = np.concatenate([touched[t] | touched[t + 1:t + 1 + w] for t, w in enumerate(nb)])
    assert (~pair).sum() > 1000 and pair.sum() > 100
    assert cor[~pair].tobytes() == cor_m[~pair].tobytes()
    assert var[~touched].tobytes() == var_m[~touched].tobytes()
    _check_exact(Gm, nb, var_m, cor_m, off)


# ----------------------------------------------------------------------------------------------------------- the fp64 route
def _check_f64(G, nb, var, cor, n):
    var_x, cor_x, _ = CC.calc_cor(G, nb, dtype=np.longdouble)
    bound = 2 * (n + 4) * U  # sum |x_a x_b| <= sqrt(v_a v_b): n + 1 roundings of the dot, and the two variances
    nan = np.isnan(np.asarray(cor_x, dtype=np.float64))
    assert np.array_equal(np.isnan(cor), nan)
    ec = np.abs(cor[~nan] - cor_x[~nan]).astype(np.float64)
    nv = np.isnan(np.asarray(var_x, dtype=np.float64))
    assert np.array_equal(np.isnan(var), nv)
    ev = (np.abs(var[~nv] - var_x[~nv]) / np.where(var_x[~nv] == 0, 1, var_x[~nv])).astype(np.float64)
    print("fp64 n = %d: worst |dr| %.3g, worst var %.3g relative, bound %.3g" % (n, ec.max(), ev.max(), bound))
    assert ec.max() <= bound and ev.max() <= bound


@pytest.mark.parametrize("n", [5, 65, 1000])
def test_fp64_route_against_long_double(api, n):
    """dosages k / 100 with NaN at 5 %: |dr| <= 2 (n + 4) 2^-53, var within the same bound relative"""
    rng = np.random.default_rng(40 + n)
    p = 300
    G = rng.integers(0, 201, size=(p, n)).astype(np.float64) / 100.0
    G[rng.random((p, n)) < 0.05] = np.nan
    G[11] = np.nan  # no called genotype
    nb = windows(rng, p)
    var, cor, off = run_f64(api, G, nb)
    _check_f64(G, nb, var, cor, n)
    var_b, cor_b, _ = run_f64(api, G, nb, batch=70)  # blocks of 70 with their halos: the same bound
    _check_f64(G, nb, var_b, cor_b, n)
    var2, cor2, _ = run_f64(api, G, nb)
    assert var.tobytes() == var2.tobytes() and cor.tobytes() == cor2.tobytes()


@pytest.mark.parametrize("n", [65, 1000])
def test_both_routes_agree_on_hard_calls(api, n):
    G, nb = hard_calls(9 * n, n, miss=0.05)
    var_i, cor_i, _ = run_plink(api, G, nb)
    var_f, cor_f, _ = run_f64(api, G, nb)
    bound = 2 * (n + 4) * U
    # compared where the exact value exists (elsewhere the integer route is 0 / 0)
    fin = ~np.isnan(cor_i)
    assert not np.isnan(cor_f[fin]).any()
    assert np.abs(cor_i[fin] - cor_f[fin]).max() <= bound
    fv = ~np.isnan(var_i) & (var_i != 0)
    assert np.array_equal(np.isnan(var_i), np.isnan(var_f))
    assert (np.abs(var_i[fv] - var_f[fv]) / var_i[fv]).max() <= bound


# ---------------------------------------------------------------------------------------------------------------- ABI edges
def test_abi_edges(api):
    from gemma_amd import _lib as L
    lib = L.lib()
    G, nb = hard_calls(5, 65, p=40, miss=0.05)
    nb = np.minimum(nb, 39 - np.arange(40)).astype(np.int32)
    bed = CC.encode_bed(G)
    ld = bed.shape[1]
    ind = np.ones(65, dtype=np.int32)
    var, cor = np.zeros(40), np.zeros(max(int(nb.sum()), 1))
    api.VARCOV.Release()
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 40, _p(nb), _p(var), _p(cor)) == L.EINVAL  # before begin
    assert lib.gemma_hip_cor_begin(65, _p(ind)) == L.OK
    bad = nb.copy()
    bad[7] = 40 - 7  # one past the last row of the block
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 40, _p(bad), _p(var), _p(cor)) == L.EINVAL
    bad = nb.copy()
    bad[3] = -1
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 40, _p(bad), _p(var), _p(cor)) == L.EINVAL
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld - 1, 40, _p(nb), _p(var), _p(cor)) == L.EINVAL  # ld too short
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 40, _p(nb), _p(var), _p(cor)) == L.OK
    var_x, cor_x, off = CC.exact_cor(G, nb)
    _check_exact(G, nb, var, cor[:off[-1]], off)
    # l_out = 1 with its halo
    v1, c1 = np.zeros(1), np.zeros(max(int(nb[0]), 1))
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 1, _p(nb), _p(v1), _p(c1)) == L.OK
    assert v1.tobytes() == var[:1].tobytes() and c1[:nb[0]].tobytes() == cor[:nb[0]].tobytes()
    # l_out == l_in, every window empty: var only, cor may be NULL
    zero = np.zeros(40, dtype=np.int32)
    v0 = np.zeros(40)
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 40, _p(zero), _p(v0), None) == L.OK
    assert v0.tobytes() == var.tobytes()
    Gf = np.ascontiguousarray(G)
    vf = np.zeros(40)
    assert lib.gemma_hip_cor_block(L.GENO_F64_SNP_MAJOR, _p(Gf), 40, 65, 40, _p(zero), _p(vf), None) == L.OK
    assert np.array_equal(np.isnan(vf), np.isnan(var))
    # a larger block after a smaller one: the buffers grow
    G2, nb2 = hard_calls(6, 65, p=300, miss=0.05)
    var2, cor2, off2 = run_plink(api, G2, nb2)
    _check_exact(G2, nb2, var2, cor2, off2)
    # the library stays correct across shutdown + init
    lib.gemma_hip_shutdown()
    api.init(0, verbose=0)
    assert lib.gemma_hip_cor_block(L.GENO_PLINK_2BIT, _p(bed), 40, ld, 40, _p(nb), _p(var), _p(cor)) == L.EINVAL  # the session is gone
    var3, cor3, _ = run_plink(api, G2, nb2)
    assert var2.tobytes() == var3.tobytes() and cor2.tobytes() == cor3.tobytes()
    api.VARCOV.Release()


def test_device_pointers_give_the_same_bits(api):
    import torch
    G, nb = hard_calls(8, 130, miss=0.05)
    var, cor, off = run_plink(api, G, nb)
    p = G.shape[0]
    v = api.VARCOV(np.ones(130, dtype=np.int32), np.ones(p, dtype=np.int32), ["1"] * p, np.zeros(p), np.arange(p), window_ns=1)
    v.n_nb = nb
    var_d, cor_d, off_d = v.AnalyzePlink(torch.as_tensor(CC.encode_bed(G)).cuda(), batch=70)
    assert np.array_equal(off, off_d)
    assert var_d.cpu().numpy().tobytes() == var.tobytes() and cor_d.cpu().numpy().tobytes() == cor.tobytes()

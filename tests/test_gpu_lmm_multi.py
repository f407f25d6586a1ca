"""T univariate LMMs over one U^T x (gemma_hip_lmm_multi_*, LMM.setup_multi / batch_multi / AnalyzeMulti) on the MI355X.

The criterion is BIT IDENTITY with the single-phenotype path, which the rest of the suite pins on the oracle and the reference: for
every phenotype t and every field the records equal those of LMM.setup(U, eval, UtW, UtY[:, t]) + LMM.batch with l_mle_null[t] /
logl_mle_H0[t] on the same blocks in the same order, in the same process and environment (np.array_equal, NaN == NaN).  Shapes are
the smallest at which the new code can go wrong: n = 203 (one K slice of the table product, ragged last chunk) and n = 1031 (two
K slices), blocks of 1, 130 and 300 SNPs twice in a row (ragged row groups of the shared table, the PLINK carry across blocks),
T = 7 at c = 1 (two passes of the shared table: 4 + 3 phenotypes) and at c = 4 (no room to share: every phenotype its own table)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import filecases as fc
import multicases as mc

pytestmark = pytest.mark.gpu

BLOCKS = (1, 1, 130, 130, 300, 300)  # l in {1, 130, 300}, each over two consecutive batches
FIELDS = ("beta", "se", "lambda_remle", "lambda_mle", "p_wald", "p_lrt", "p_score", "logl_H1")


@functools.lru_cache(maxsize=None)
def _panel(n, c, T, dosage=False):
    from oracle import oracle as O
    O.lib()
    h2s = tuple(np.linspace(0.0, 0.95, T)) if T > 1 else (0.5,)
    return mc.panel(O, n, sum(BLOCKS), c, h2s, seed=1000 * n + 10 * c + T, dosage=dosage)


def _cut(X, sizes=BLOCKS):
    out, s0 = [], 0
    for l in sizes:
        out.append(np.ascontiguousarray(X[s0:s0 + l]))
        s0 += l
    return out


def _nulls(api, ev, UtW, UtY, n_region=10):
    fits = [api.CalcLambdaNull(ev, UtW, np.ascontiguousarray(UtY[:, t]), n_region=n_region) for t in range(UtY.shape[1])]
    return np.array([f["l_mle_null"] for f in fits]), np.array([f["logl_mle_H0"] for f in fits])


def _single(api, mode, U, ev, UtW, UtY, t, nulls, blocks, kind, plink=False, ind=None, n_region=10):
    lmm = api.LMM(a_mode=mode, n_region=n_region, l_mle_null=float(nulls[0][t]), logl_mle_H0=float(nulls[1][t]))
    lmm.setup(U, ev, UtW, np.ascontiguousarray(UtY[:, t]), plink=plink)
    try:
        if ind is not None:
            lmm.set_indicator(ind)
        return np.concatenate([lmm.batch(b, kind) for b in blocks])
    finally:
        lmm.finish()


def _multi(api, mode, U, ev, UtW, UtY, nulls, blocks, kind, plink=False, ind=None, n_region=10):
    lmm = api.LMM(a_mode=mode, n_region=n_region)
    lmm.setup_multi(U, ev, UtW, UtY, nulls[0], nulls[1], plink=plink)
    try:
        if ind is not None:
            lmm.set_indicator(ind)
        return np.concatenate([lmm.batch_multi(b, kind) for b in blocks], axis=1)
    finally:
        lmm.finish()


def _same(got, want, tag):
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    for k in FIELDS:
        assert np.array_equal(got[k], want[k], equal_nan=True), (tag, k, int((~((got[k] == want[k]) | (np.isnan(got[k]) & np.isnan(want[k])))).sum()))


def _check(api, mode, data, kind, tag, **kw):
    X, U, ev, UtW, UtY = data[:5]
    blocks = kw.pop("blocks", None) or _cut(X)
    nulls = _nulls(api, ev, UtW, UtY, kw.get("n_region", 10))
    got = _multi(api, mode, U, ev, UtW, UtY, nulls, blocks, kind, **kw)
    assert got.shape == (UtY.shape[1], sum(len(b) for b in blocks))
    for t in range(UtY.shape[1]):
        _same(got[t], _single(api, mode, U, ev, UtW, UtY, t, nulls, blocks, kind, **kw), "%s mode=%d t=%d" % (tag, mode, t))
    return got


@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_multi_equals_single_one_k_slice(gpu_api, c, T):
    """n = 203: one K slice with a ragged last chunk; fp64 hard calls (the int8-digit product); T = 1 is the single path itself"""
    from gemma_amd import _lib as L
    for mode in (1, 4):
        got = _check(gpu_api, mode, _panel(203, c, T), L.GENO_F64_SNP_MAJOR, "n=203 c=%d T=%d" % (c, T))
        assert np.isfinite(got["p_wald"]).mean() > 0.9


@pytest.mark.parametrize("c", [1, 4])
def test_multi_equals_single_two_k_slices_seven_phenotypes(gpu_api, c):
    """n = 1031: two K slices; T = 7: two passes of the shared table at c = 1 (4 + 3), none at c = 4"""
    from gemma_amd import _lib as L
    data = _panel(1031, c, 7)
    blocks = _cut(data[0], (300, 130, 1))
    for mode in (1, 4):
        _check(gpu_api, mode, data, L.GENO_F64_SNP_MAJOR, "n=1031 c=%d" % c, blocks=blocks)


@pytest.mark.parametrize("mode", [2, 3, 9])
def test_multi_other_modes(gpu_api, mode):
    from gemma_amd import _lib as L
    _check(gpu_api, mode, _panel(203, 2, 3), L.GENO_F64_SNP_MAJOR, "modes")


def _plink_panel():
    """254 individuals, 20 % dropped, 3 % missing calls; monomorphic and all-missing SNPs at the start, inside and at the end of
    blocks: PLINK's beta / se carry (plink_nan_rule) crosses block boundaries in every phenotype's own chain"""
    from oracle import oracle as O
    O.lib()
    rng = np.random.default_rng(77)
    ni_total, p = 254, sum(BLOCKS)
    ind = (rng.random(ni_total) > 0.2).astype(np.int32)
    codes = rng.choice([0, 1, 2, 3], size=(p, ni_total), p=[0.25, 0.03, 0.42, 0.30]).astype(np.uint8)
    for s in (0, 1, 2, 57, 131, 132, 262, 300, 561, 562, p - 1):
        codes[s] = 1 if s % 2 else 3  # all missing / monomorphic
    raw = mc.pack_bed(codes)
    n = int(ind.sum())
    Kg = rng.binomial(2, 0.3, size=(400, n)).astype(np.float64)  # the kinship: SNPs of their own
    U, ev, _ = O.eigen_decomp_zeroed(O.center_matrix(O.calc_kin(Kg, 1)))
    x40 = np.nan_to_num(O.bed_decode(raw, ni_total, ind)[40])
    Y = np.stack([rng.standard_normal(n), Kg.T @ rng.standard_normal(400) * 0.2 + 0.3 * rng.standard_normal(n),
                  0.5 * x40 + rng.standard_normal(n)], axis=1)
    return raw, U, ev, U.T @ np.ones((n, 1)), np.ascontiguousarray(U.T @ Y), ind


def test_multi_plink_blocks_with_their_carry_chains(gpu_api):
    from gemma_amd import _lib as L
    data = _plink_panel()
    for mode in (1, 4):
        got = _check(gpu_api, mode, data, L.GENO_PLINK_2BIT, "plink", plink=True, ind=data[5])
        assert gpu_api.last_utx_path() == 1  # the int8-digit product of 2-bit blocks


def test_multi_real_valued_dosages(gpu_api):
    from gemma_amd import _lib as L
    _check(gpu_api, 1, _panel(203, 1, 3, dosage=True), L.GENO_F64_SNP_MAJOR, "dosage")
    assert gpu_api.last_utx_path() == 0  # real-valued: the fp64 GEMM


def test_multi_plain_loop_generic_kernel_and_streaming(gpu_api):
    """c = 5 (generic kernel, no tables) and n_region = 7 (no table for that weight count): the plain per-phenotype loop"""
    from gemma_amd import _lib as L
    _check(gpu_api, 4, _panel(203, 5, 3), L.GENO_F64_SNP_MAJOR, "c=5", blocks=_cut(_panel(203, 5, 3)[0], (130, 300)))
    _check(gpu_api, 4, _panel(203, 2, 3), L.GENO_F64_SNP_MAJOR, "n_region=7", blocks=_cut(_panel(203, 2, 3)[0], (130, 300)), n_region=7)


def test_shared_table_switch_and_repeat_are_bit_identical(gpu_api, monkeypatch):
    """GEMMA_HIP_MULTI_TABLE=0 (every phenotype computes its own fixed-lambda table) and =1 (default: one read of U^T x per group
    of phenotypes) give the same bits; so do two runs"""
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = _panel(1031, 1, 7)
    blocks = _cut(X, (300, 130, 1))
    nulls = _nulls(gpu_api, ev, UtW, UtY)
    res, scopes = {}, {}
    gpu_api.profile_enable(True)
    try:
        for key, env in (("on", "1"), ("off", "0"), ("again", "1")):
            monkeypatch.setenv("GEMMA_HIP_MULTI_TABLE", env)
            gpu_api.reload_env()
            gpu_api.profile_read(L.STAGE_ASSOC, reset=True)
            res[key] = _multi(gpu_api, 4, U, ev, UtW, UtY, nulls, blocks, L.GENO_F64_SNP_MAJOR)
            scopes[key] = gpu_api.profile_read(L.STAGE_ASSOC, reset=True)[1]
    finally:
        gpu_api.profile_enable(False)
        monkeypatch.delenv("GEMMA_HIP_MULTI_TABLE")
        gpu_api.reload_env()
    # that the shared table ran at all: a profiled block has one per-SNP-stage scope per phenotype, and with the shared table one
    # more per group of 4 phenotypes (7 = 4 + 3)
    assert scopes == {"on": 3 * (7 + 2), "off": 3 * 7, "again": 3 * (7 + 2)}, scopes
    _same(res["off"], res["on"], "table off / on")
    _same(res["again"], res["on"], "second run")


def test_low_and_high_heritability_side_by_side(gpu_api):
    """lambda-hat at l_min for most SNPs of the noise trait, large for the heritable one, in one scan: a slot mix-up would show"""
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = _panel(203, 1, 2)  # h2 = 0 and 0.95
    got = _check(gpu_api, 1, (X, U, ev, UtW, UtY), L.GENO_F64_SNP_MAJOR, "low / high")
    lo, hi = got["lambda_remle"][0], got["lambda_remle"][1]
    assert np.nanmedian(lo) < 0.1 * np.nanmedian(hi), (np.nanmedian(lo), np.nanmedian(hi))
    assert (lo <= 1.0001e-5).mean() > (hi <= 1.0001e-5).mean()


def test_analyze_multi_fits_missing_nulls(gpu_api):
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = _panel(203, 2, 3)
    lmm = gpu_api.LMM(a_mode=4)
    got = lmm.AnalyzeMulti(U, ev, UtW, UtY, X, L.GENO_F64_SNP_MAJOR, False, None, batch=300)
    assert got.shape == (3, len(X)) and lmm.sumStat is got
    nulls = _nulls(gpu_api, ev, UtW, UtY)
    blocks = [X[s:s + 300] for s in range(0, len(X), 300)]
    for t in range(3):
        _same(got[t], _single(gpu_api, 4, U, ev, UtW, UtY, t, nulls, blocks, L.GENO_F64_SNP_MAJOR), "AnalyzeMulti t=%d" % t)


def test_multi_state_errors(gpu_api):
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = _panel(203, 1, 2)
    lib = L.lib()
    n = U.shape[0]
    out = np.zeros((2, 4), dtype=gpu_api.SUMSTAT_DTYPE)
    blk = np.ascontiguousarray(X[:4])
    # multi batch before any setup
    assert lib.gemma_hip_lmm_multi_batch(L.GENO_F64_SNP_MAJOR, blk.ctypes.data, 4, n, out.ctypes.data) == L.ESTATE
    lmm = gpu_api.LMM(a_mode=1)
    for T in (0, 65):
        with pytest.raises(L.GemmaHipError) as e:
            lmm.setup_multi(U, ev, UtW, np.zeros((n, T)))
        assert e.value.code == L.EINVAL
    with pytest.raises(L.GemmaHipError) as e:  # modes that read the nulls need them
        gpu_api.LMM(a_mode=4).setup_multi(U, ev, UtW, UtY)
    assert e.value.code == L.EINVAL
    lmm.setup_multi(U, ev, UtW, UtY)
    with pytest.raises(L.GemmaHipError) as e:  # single-phenotype batch after a multi setup
        lmm.batch(blk, L.GENO_F64_SNP_MAJOR)
    assert e.value.code == L.ESTATE
    assert lmm.batch_multi(blk, L.GENO_F64_SNP_MAJOR).shape == (2, 4)
    lmm.finish()
    lmm.setup(U, ev, UtW, np.ascontiguousarray(UtY[:, 0]))
    with pytest.raises(L.GemmaHipError) as e:  # multi batch after a single-phenotype setup
        lmm.batch_multi(blk, L.GENO_F64_SNP_MAJOR)
    assert e.value.code == L.ESTATE
    assert len(lmm.batch(blk, L.GENO_F64_SNP_MAJOR)) == 4
    lmm.finish()


_FRESH = """
import sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, %r)
from gemma_amd import api, _lib as L
d = np.load(sys.argv[1])
api.init(0, 0)
lmm = api.LMM(a_mode=1)
lmm.setup(d["U"], d["ev"], d["UtW"], d["Uty"])
out = np.concatenate([lmm.batch(np.ascontiguousarray(d["X"][s:s + 300]), L.GENO_F64_SNP_MAJOR) for s in (0, 300)])
lmm.finish()
np.save(sys.argv[2], out)
"""


def test_finish_then_single_setup_matches_a_fresh_process(gpu_api, tmp_path):
    from gemma_amd import _lib as L
    X, U, ev, UtW, UtY = _panel(203, 1, 3)
    X = np.ascontiguousarray(X[:600])
    blocks = [X[:300], X[300:]]
    _multi(gpu_api, 1, U, ev, UtW, UtY, (None, None), blocks, L.GENO_F64_SNP_MAJOR)
    Uty = np.ascontiguousarray(UtY[:, 1])
    here = _single(gpu_api, 1, U, ev, UtW, UtY, 1, (np.zeros(3), np.zeros(3)), blocks, L.GENO_F64_SNP_MAJOR)
    np.savez(tmp_path / "in.npz", U=U, ev=ev, UtW=UtW, Uty=Uty, X=X)
    script = tmp_path / "fresh.py"
    script.write_text(_FRESH % (fc.ROOT, os.path.join(fc.ROOT, "tests")))
    r = subprocess.run([sys.executable, str(script), str(tmp_path / "in.npz"), str(tmp_path / "out.npy")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    _same(here, np.load(tmp_path / "out.npy"), "fresh process")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    from gemma_amd import build
    build.build()
    tmp = tmp_path_factory.mktemp("drv")
    libdir = os.path.join(fc.ROOT, "gemma_amd")
    single = fc.build_driver(tmp, libdir)
    multi = os.path.join(str(tmp), "multi_file_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-Wall", "-I" + os.path.join(fc.ROOT, "include"),
                           os.path.join(fc.ROOT, "tests", "cpp", "multi_file_driver.cpp"), "-L" + libdir, "-lgemma_hip",
                           "-Wl,-rpath," + libdir, "-lz", "-pthread", "-o", multi])
    return single, multi


def test_multi_file_driver_writes_the_single_runs_files(drivers, tmp_path):
    """multi_file_driver -nsep 1 2 3 against three gemma_file_driver -n t runs on a 150 x 300 PLINK set whose three phenotype
    columns are complete: the .assoc.txt files are byte-equal; and against what the reference printed for `-lmm 4 -n t`
    (tests/golden/ref_multi.npz, tests/golden/make_multi_fixtures.py) under the bounds of filecases.compare_assoc."""
    single, multi = drivers
    out = str(tmp_path)
    codes, pheno = mc.plink_set()
    pre = os.path.join(out, "M")
    mc.write_plink(pre, codes, pheno)
    base = ["-bfile", pre, "-outdir", out]
    fc.drive(single, *base, "-gk", "-o", "M")
    cxx = os.path.join(out, "M.cXX.txt")
    kv = fc.drive(multi, *base, "-k", cxx, "-lmm", 4, "-nsep", 1, 2, 3, "-o", "run")
    assert int(kv["ni_test"]) == 150 and int(kv["n_ph"]) == 3 and int(kv["snps"]) == int(kv["ns_test"]) > 250
    ref = np.load(mc.REF_NPZ)
    assert np.array_equal(ref["codes"], codes) and np.array_equal(ref["pheno"], pheno)
    for t in (1, 2, 3):
        fc.drive(single, *base, "-k", cxx, "-lmm", 4, "-n", t, "-o", "one%d" % t)
        got = open(os.path.join(out, "run.%d.assoc.txt" % t), "rb").read()
        assert got == open(os.path.join(out, "one%d.assoc.txt" % t), "rb").read(), t
        (tmp_path / ("ref%d.assoc.txt" % t)).write_bytes(ref["assoc%d" % t].tobytes())
        fc.compare_assoc(os.path.join(out, "run.%d.assoc.txt" % t), str(tmp_path / ("ref%d.assoc.txt" % t)))
    # mode 1 through the same driver: each phenotype's own PLINK carry chain
    fc.drive(multi, *base, "-k", cxx, "-lmm", 1, "-nsep", 3, 1, "-o", "m1")
    for t in (3, 1):
        fc.drive(single, *base, "-k", cxx, "-lmm", 1, "-n", t, "-o", "s1_%d" % t)
        assert open(os.path.join(out, "m1.%d.assoc.txt" % t), "rb").read() == open(os.path.join(out, "s1_%d.assoc.txt" % t), "rb").read()


def test_multi_file_driver_refuses_an_empty_set_of_individuals(drivers, tmp_path):
    """the analysed individuals are those with EVERY selected phenotype: two columns that are never present together leave none"""
    _, multi = drivers
    codes, pheno = mc.plink_set(ni=40, ns=30)
    pre = str(tmp_path / "E")
    mc.write_plink(pre, codes, pheno)
    lines = open(pre + ".fam").read().strip().split("\n")
    with open(pre + ".fam", "w") as f:
        for i, l in enumerate(lines):
            w = l.split()
            w[5 + (i % 2)] = "-9"
            f.write(" ".join(w) + "\n")
    np.savetxt(tmp_path / "K.txt", np.eye(40), fmt="%.10g", delimiter="\t")
    r = subprocess.run([multi, "-bfile", pre, "-k", str(tmp_path / "K.txt"), "-lmm", "1", "-nsep", "1", "2", "-outdir", str(tmp_path)],
                       capture_output=True, text=True)
    assert r.returncode == 3 and not os.path.exists(tmp_path / "result.1.assoc.txt")
    assert "analyzed individuals equals 0" in r.stdout or "nothing to analyse" in r.stdout

"""The hits form of the score panel without a GPU: the exported prototypes and struct layouts, no CPU fall-back, the file driver on
the product library, the restatement tests/scorehitcases.select on hand-made records, and api.reduce_score_best against it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import scorecases as sc
import scorehitcases as sh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gemma_hip_lmm_score_panel_hits_batch", "gemma_hip_lmm_score_panel_hits_batch_d", "gemma_hip_lmm_score_panel_hits_assoc_d")
NAN = float("nan")


def test_hits_symbols_and_prototypes():
    from gemma_amd import _lib, build
    so = build.build()
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    lib = _lib.lib()
    raw = C.CDLL(so)
    kinds = {"size_t": C.c_size_t, "int": C.c_int, "double": C.c_double}
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/gemma_hip.h"
        assert hasattr(raw, name), name + " is not exported by the library"
        assert name in _lib.SYMBOLS
        params = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        bound = getattr(lib, name).argtypes
        assert bound is not None and len(bound) == len(params), (name, len(params))
        for decl, ct in zip(params, bound):
            if "*" in decl:
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, decl, ct)
            else:
                assert ct is kinds[decl.split()[-2]], (name, decl, ct)
    assert "ARRIVAL ORDER" in hdr  # the _d forms say that their list is unsorted


def test_hit_and_best_layouts():
    from gemma_amd import _lib, api
    assert C.sizeof(_lib.ScoreHit) == 32 and C.sizeof(_lib.ScoreBest) == 32
    assert api.SCORE_HIT_DTYPE.itemsize == 32 and api.SCORE_BEST_DTYPE.itemsize == 32
    assert api.SCORE_HIT_DTYPE == sh.HIT_DTYPE and api.SCORE_BEST_DTYPE == sh.BEST_DTYPE
    for ct, dt in ((_lib.ScoreHit, api.SCORE_HIT_DTYPE), (_lib.ScoreBest, api.SCORE_BEST_DTYPE)):
        assert [f[0] for f in ct._fields_] == list(dt.names)
        assert [getattr(ct, k).offset for k in dt.names] == [dt.fields[k][1] for k in dt.names]
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    assert re.search(r"typedef struct \{\s*uint32_t snp, pheno;\s*double beta, se, p_score;\s*\} gemma_score_hit;", hdr)
    assert re.search(r"typedef struct \{\s*double beta, se, p_score;\s*int64_t snp;\s*\} gemma_score_best;", hdr)


def test_hits_entry_points_need_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_score_hits.py")
    from gemma_amd import _lib
    lib = _lib.lib()
    x = np.zeros((4, 8))
    cnt = C.c_ulonglong(7)
    assert lib.gemma_hip_lmm_score_panel_hits_batch(_lib.GENO_F64_SNP_MAJOR, x.ctypes.data, 4, 8, 0.5, None, 0, C.addressof(cnt),
                                                    None) == _lib.ENODEV
    assert lib.gemma_hip_lmm_score_panel_hits_batch_d(_lib.GENO_F64_SNP_MAJOR, x.ctypes.data, 4, 8, 0.5, None, 0, C.addressof(cnt),
                                                      None, None) == _lib.ENODEV
    assert lib.gemma_hip_lmm_score_panel_hits_assoc_d(x.ctypes.data, 4, 8, 0.5, None, 0, C.addressof(cnt), None, None) == _lib.ENODEV
    assert cnt.value == 7  # nothing was computed


def test_file_driver_on_the_product_library_fails_loudly_without_gpu(tmp_path):
    """tests/cpp/score_panel_file_driver.cpp builds with plain g++ -std=c++11 -Wall against the product library; without a GPU
    the run stops at gemma_hip_init with the no-device message and writes no hits file"""
    import torch
    from gemma_amd import build
    so = build.build()
    exe = str(tmp_path / "sfd")
    r = subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "score_panel_file_driver.cpp"), "-L" + os.path.dirname(so),
                        "-lgemma_hip", "-Wl,-rpath," + os.path.dirname(so), "-lz", "-pthread", "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    if torch.cuda.is_available():
        return  # the run itself is covered by tests/test_gpu_score_hits.py
    P =os.path.join(ROOT, "tests", "golden", "text", "P")
    r = subprocess.run([exe, "-bfile", P, "-k", "none", "-lmm", "3", "-pmax", "1e-3", "-o", "run", "-outdir", str(tmp_path)],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "no CPU fallback" in r.stderr, (r.returncode, r.stderr[-2000:])
    assert not os.path.exists(tmp_path / "run.hits.txt")


def _records(p, beta=None):
    p = np.asarray(p, dtype=np.float64)
    rec = np.zeros(p.shape, dtype=sc.SCORE_DTYPE)
    rec["p_score"] = p
    rec["beta"] = np.arange(p.size, dtype=np.float64).reshape(p.shape) + 0.5 if beta is None else beta
    rec["se"] = 2.0 * rec["beta"]
    rec["beta"][np.isnan(p)] = NAN
    rec["se"][np.isnan(p)] = NAN
    return rec


#            snp 0   1     2     3     4
HAND = [[0.50, 0.01, NAN, 0.01, 0.20],   # a tie at the minimum: snp 1 wins over snp 3
        [NAN, NAN, NAN, NAN, NAN],       # an empty phenotype
        [0.30, 1e-9, NAN, 0.02, 1.00],   # NaN column 2: the degenerate row
        [0.00, 0.70, NAN, 0.05, 0.05]]   # p = 0 and p = p_max


def test_select_on_hand_made_records():
    rec = _records(HAND)
    hits, best = sh.select(rec, 0.05)
    assert [(int(h["pheno"]), int(h["snp"])) for h in hits] == [(0, 1), (0, 3), (2, 1), (2, 3), (3, 0), (3, 3), (3, 4)]
    for h in hits:  # the pair at p == p_max is a hit, and a hit carries its record
        assert all(h[k] == rec[k][h["pheno"], h["snp"]] for k in sh.STATS)
    assert list(best["snp"]) == [1, -1, 1, 0]
    assert np.isnan(best[1]["beta"]) and np.isnan(best[1]["se"]) and np.isnan(best[1]["p_score"])
    assert best[0]["beta"] == rec["beta"][0, 1] and best[3]["p_score"] == 0.0
    hits, _ = sh.select(rec, 0.0)
    assert [(int(h["pheno"]), int(h["snp"])) for h in hits] == [(3, 0)]  # only a p_score of exactly 0
    hits, _ = sh.select(rec, 1.0)
    assert len(hits) == int((~np.isnan(rec["p_score"])).sum()) == 12 and not (hits["snp"] == 2).any()
    hits, best = sh.select(rec, 0.05, offset=100)
    assert hits["snp"].min() == 100 and list(best["snp"]) == [101, -1, 101, 100]
    hits, best = sh.select(np.zeros((3, 0), dtype=sc.SCORE_DTYPE), 0.5)  # an empty block
    assert len(hits) == 0 and list(best["snp"]) == [-1, -1, -1] and np.isnan(best["p_score"]).all()


def test_best_is_reduced_over_blocks_as_over_one():
    """api.reduce_score_best over per-block bests against select on the concatenated records: a tie across blocks goes to the
    smaller index, a NaN block never wins, an empty phenotype stays -1"""
    from gemma_amd import api
    rec = _records([[0.50, 0.01, NAN, 0.01, 0.20, 0.01, 0.90],
                    [NAN, NAN, NAN, NAN, NAN, NAN, NAN],
                    [NAN, NAN, NAN, 0.02, 1.00, 1e-9, 1e-9],
                    [0.70, 0.70, NAN, NAN, NAN, 0.70, 0.80]])
    _, want = sh.select(rec, 1.0)
    for cuts in ((0, 3, 5, 7), (0, 1, 2, 3, 4, 5, 6, 7), (0, 7), (0, 2, 2, 7)):
        blocks = [(a, sh.select(rec[:, a:b], 1.0)[1]) for a, b in zip(cuts, cuts[1:])]
        got = api.reduce_score_best(blocks, 4)
        assert sh.same_bits(got, want), (cuts, got, want)
        got = api.reduce_score_best(blocks[::-1], 4)  # the order of the blocks does not matter
        assert sh.same_bits(got, want), (cuts, "reversed")
    none = api.reduce_score_best([], 2)
    assert list(none["snp"]) == [-1, -1] and np.isnan(none["beta"]).all()

"""The checker of tests/test_gpu_firstpass.py checked on the CPU: every reference of tests/firstpasscases.py agrees with the
oracle's restatement of the same routine (two independent restatements), every planted row does what its name says in the
reference alone, every QC case keeps a middling share of its SNPs, and the recorded -lm bar is what its measurement gives."""
from fractions import Fraction

import numpy as np
import pytest

import firstpasscases as FC

U = FC.U


# ----------------------------------------------------------------------------------------------------------------- .bed
@pytest.mark.parametrize("ni", [1, 2, 3, 4, 5, 63, 64, 65, 66, 67])
def test_bed_round_trip_and_oracle_decode(oracle, ni):
    rng = np.random.default_rng(ni)
    G = FC.hard_calls(rng, 5, ni, miss=0.2)
    ind = (rng.random(ni) < 0.7).astype(np.int32)
    ind[rng.integers(ni)] = 1
    for ld in (None, (ni + 3) // 4 + 3):
        raw = FC.pack_bed(FC.geno_to_codes(G), ld=ld)
        assert raw.shape[1] == ((ni + 3) // 4 if ld is None else ld)
        assert np.array_equal(FC.bed_decode(raw, ni), G, equal_nan=True)
        assert np.array_equal(FC.bed_decode(raw, ni, ind), G[:, ind == 1], equal_nan=True)
        tight = np.ascontiguousarray(raw[:, :(ni + 3) // 4])
        assert np.array_equal(oracle.bed_decode(tight, ni, ind), G[:, ind == 1], equal_nan=True)
    # the stated layout: individual p at byte p >> 2, bits 2 * (p & 3); code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing
    assert FC.pack_bed(np.array([[0, 1, 2, 3]], dtype=np.uint8))[0, 0] == 0b11100100
    assert np.array_equal(FC.bed_decode(np.array([[0b11100100]], dtype=np.uint8), 4), [[2.0, np.nan, 1.0, 0.0]], equal_nan=True)


@pytest.mark.parametrize("pattern", FC.PATTERNS)
def test_indicator_patterns(pattern):
    for n in FC.N_LIST:
        for rem in range(4):
            ind = FC.indicator(n, pattern, rem)
            ni = ind.size
            assert int(ind.sum()) == n and ni % 4 == rem and ni > n
            per_byte = [ind[4 * b:4 * b + 4] for b in range((ni + 3) // 4)]
            if pattern == "first":
                assert ind[0] == 0 and ind[-1] == 1
            if pattern == "last":
                assert ind[0] == 1 and ind[-1] == 0
            if pattern == "every_byte":
                assert all(0 in b for b in per_byte)
            if pattern == "last_lane":
                assert all(b.sum() <= 1 and (b.sum() == 0 or b[-1] == 1) for b in per_byte) and sum(b.sum() == 0 for b in per_byte) <= 1


# ------------------------------------------------------------------------------------------------------------------- QC
def _ref(cs, **over):
    cfg = dict(cs.get("cfg", {}))
    cfg.update(over)
    return FC.qc_reference(cs["G"], cs["ind"], cs["W"], cs["plink"], **cfg)


@pytest.mark.parametrize("n,pattern,rem,plink,seed", FC.qc_sweep_list())
def test_qc_sweep_reference_against_the_oracle(oracle, n, pattern, rem, plink, seed):
    cs = FC.qc_sweep_case(n, pattern, rem, plink, seed)
    ref = _ref(cs)
    kept = sum(ref["indicator"])
    if n == 1:  # one call is never polymorphic: nothing can be kept
        assert kept == 0
    else:  # a condition on the case (it must not pass on "all dropped"), not a measurement
        assert 0.2 <= kept / 9 <= 0.8, (kept, ref["why"])
    assert ref["why"][1] == "miss" and np.isnan(ref["maf"][1]) and ref["n_miss"][1] == n
    assert ref["n_miss"][7] == n - 1 and ref["indicator"][5] == 0
    for r2 in ref["r2"]:  # no decision of the sweep sits at the r2 level, where float64 and the rationals could part
        assert r2 is None or abs(float(r2) - 0.9999) > 1e-6
    if plink:
        o_i = oracle.qc_snps_bed(cs["G"][:, cs["ind"] == 1], cs["W"], maf_level=0.05, miss_level=0.05)
    else:
        o_i, o_maf, o_nm = oracle.qc_snps(cs["G"], cs["ind"], cs["W"], maf_level=0.05, miss_level=0.05)
        assert np.array_equal(o_nm, ref["n_miss"])
        assert np.array_equal(o_maf, ref["maf"], equal_nan=True)  # sums of hard calls are exact in numpy too
    assert np.array_equal(o_i, ref["indicator"])


def test_qc_sweep_covers_the_shapes():
    cases = FC.qc_sweep_list()
    assert {c[0] for c in cases} == set(FC.N_LIST) and {c[1] for c in cases} == set(FC.PATTERNS)
    for plink in (True, False):
        assert {FC.indicator(c[0], c[1], c[2]).size % 4 for c in cases if c[3] == plink} == {0, 1, 2, 3}


@pytest.mark.parametrize("plink", [True, False])
def test_qc_planted_rows_do_what_they_say(oracle, plink):
    cs, row = FC.qc_planted_case(plink)
    ref = _ref(cs)
    why = {k: ref["why"][i] for k, i in row.items()}
    maf = {k: ref["maf"][i] for k, i in row.items()}
    assert why["all_missing_analysed"] == "miss" and np.isnan(maf["all_missing_analysed"])
    assert not np.all(np.isnan(cs["G"][row["all_missing_analysed"]]))  # observed among the dropped
    assert why["one_observed"] == "miss" and ref["n_miss"][row["one_observed"]] == 63 and maf["one_observed"] == 0.5
    assert why["mono0"] == "maf" and why["mono2"] == "maf" and why["mono1"] == "poly"
    assert why["no_class0"] is None and why["no_class1"] is None and why["no_class2"] is None
    for k, empty in (("no_class0", "n0"), ("no_class1", "n1"), ("no_class2", "n2")):
        assert ref[empty][row[k]] == 0
    assert ref["n_miss"][row["miss_at_level"]] == 4 and why["miss_at_level"] is None
    assert ref["n_miss"][row["miss_above_level"]] == 5 and why["miss_above_level"] == "miss"
    assert maf["maf_at_level"] == 0.125 and why["maf_at_level"] is None and why["maf_below_level"] == "maf"
    assert maf["maf_at_one_minus_level"] == 0.875 and why["maf_at_one_minus_level"] is None
    assert why["maf_above_one_minus_level"] == "maf"
    assert why["equals_covariate"] == "r2" and ref["r2"][row["equals_covariate"]] == 1
    assert why["regular"] is None and why["no_het"] is None
    kept = sum(ref["indicator"])
    assert 0.2 <= kept / len(row) <= 0.8
    for r2 in ref["r2"]:
        assert r2 is None or r2 == 1 or float(r2) < 0.99
    # maf_level = -1 switches the maf AND the HWE filter off: the polymorphism rule still holds
    off = _ref(cs, maf_level=-1, hwe_level=FC.QC_PLANT_HWE)
    for k in ("maf_below_level", "maf_above_one_minus_level", "no_het"):
        assert off["why"][row[k]] is None
    assert off["why"][row["mono0"]] == off["why"][row["mono1"]] == off["why"][row["mono2"]] == "poly"
    # HWE on: the row without heterozygotes goes, and sits far from the level
    on = _ref(cs, hwe_level=FC.QC_PLANT_HWE)
    assert on["why"][row["no_het"]] == "hwe" and on["hwe"][row["no_het"]] < Fraction(FC.QC_PLANT_HWE) / 10
    for i, p in enumerate(on["hwe"]):
        assert p is None or p < Fraction(FC.QC_PLANT_HWE) / 10 or p > Fraction(FC.QC_PLANT_HWE) * 10, (i, float(p))
    assert 0.2 <= sum(on["indicator"]) / len(row) <= 0.8
    # one covariate: the r2 test is skipped
    one = FC.qc_reference(cs["G"], cs["ind"], np.ones((cs["n"], 1)), plink, **cs["cfg"])
    assert one["why"][row["equals_covariate"]] is None
    if not plink:  # 0.5 is n0, 1.5 is n2: 16 / 32 / 16 is in HWE, and a boundary value counted as a heterozygote is far from it
        i = row["dosage_boundaries"]
        assert (ref["n0"][i], ref["n1"][i], ref["n2"][i]) == (16, 32, 16) and maf["dosage_boundaries"] == 0.5
        assert on["why"][i] is None and on["hwe"][i] > Fraction(1, 2)
        for wrong in ((0, 16, 48), (16, 0, 48), (0, 0, 64)):
            assert FC.hwe_exact(*wrong) < Fraction(FC.QC_PLANT_HWE) / 10
    # the oracle's cascade on the same rows
    if plink:
        for hwe in (0.0, FC.QC_PLANT_HWE):
            o = oracle.qc_snps_bed(cs["G"][:, cs["ind"] == 1], cs["W"], maf_level=0.125, miss_level=4 / 64, hwe_level=hwe)
            assert np.array_equal(o, (on if hwe else ref)["indicator"])
    else:
        o, o_maf, o_nm = oracle.qc_snps(cs["G"], cs["ind"], cs["W"], maf_level=0.125, miss_level=4 / 64)
        assert np.array_equal(o, ref["indicator"]) and np.array_equal(o_nm, ref["n_miss"])
        assert np.array_equal(o_maf, ref["maf"], equal_nan=True)


def test_hwe_exact_against_the_oracle_and_by_hand(oracle):
    # two genotypes, two copies of the rare allele: h = 2 has weight 4 / 2! = 2, h = 0 has weight 1
    assert FC.hwe_exact(0, 0, 2) == 1 and FC.hwe_exact(1, 1, 0) == Fraction(1, 3)
    assert FC.hwe_exact(0, 0, 0) == 1
    for t in FC.HWE_COUNTS + ((3, 7, 11), (50, 50, 100), (0, 9, 1)):
        assert FC.hwe_exact(t[0], t[1], t[2]) == FC.hwe_exact(t[1], t[0], t[2])
        assert abs(oracle.calc_hwe(*t) - float(FC.hwe_exact(*t))) <= 1e-12 * float(FC.hwe_exact(*t))


@pytest.mark.parametrize("plink", [True, False])
def test_hwe_case_sits_away_from_its_levels(plink):
    cs, trip = FC.hwe_case(plink)
    assert any(t[2] == 0 for t in trip) and any(t[0] > t[1] for t in trip) and any(t[0] < t[1] for t in trip)
    assert plink or any(t[0] == 0 and t[1] == 0 for t in trip)
    levels = FC.hwe_levels(trip)
    base = FC.qc_reference(cs["G"], cs["ind"], cs["W"], plink, maf_level=0.0, miss_level=1.0, hwe_level=0.0)
    assert all(w is None for w in base["why"])  # polymorphic, so HWE alone decides below
    assert [(a, b, c) for a, b, c in zip(base["n0"], base["n2"], base["n1"])] == list(trip)
    for t in trip:
        p = float(FC.hwe_exact(*t))
        far = [lv for lv in levels if lv >= 10 * p * (1 - 1e-12) or lv <= p / 10 * (1 + 1e-12)]
        assert any(lv > p for lv in far) and any(lv < p for lv in far)


# -------------------------------------------------------------------------------------------------------------- ingest
def test_impute_reference_against_the_oracle(oracle):
    rng = np.random.default_rng(3)
    X = FC.hard_calls(rng, 40, 65, miss=0.2)
    assert np.array_equal(FC.impute_reference(X), oracle.impute_mean(X))
    assert np.all(np.isnan(FC.impute_reference(np.full((1, 5), np.nan))))


@pytest.mark.parametrize("n", FC.N_LIST)
@pytest.mark.parametrize("k_mode", [1, 2])
def test_kin_reference_against_the_oracle(oracle, n, k_mode):
    G = FC.kin_case(n, 300 + n)
    assert np.all(G[5] == 2.0) and np.isfinite(G[11]).sum() == 1 and not np.any(np.all(np.isnan(G), axis=1))
    K, bound = FC.kin_reference(G, k_mode)
    assert np.array_equal(K, K.T)
    o = oracle.calc_kin(G, k_mode)
    assert np.all(np.abs(o - K) <= bound), float(np.max(np.abs(o - K) - bound))
    assert float(bound.max()) < 1e-12 * max(1.0, float(np.abs(K).max()))  # the bar is a rounding bar
    if n > 1:  # the monomorphic row contributes nothing: K p is the kinship of the other rows times (p - 1)
        K2, _ = FC.kin_reference(np.delete(G, 5, axis=0), k_mode)
        assert float(np.abs(K * 37 - K2 * 36).max()) < 1e-15 * 37


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_center_reference_against_the_oracle(oracle, n):
    G = FC.int_symmetric(np.random.default_rng(n), n)
    ref = FC.center_reference(G)
    o = oracle.center_matrix(G.copy())
    M = np.abs(G).max()
    assert float(np.abs(o - ref).max()) <= FC.CENTER_ULPS * U * M
    if n & (n - 1) == 0:  # a power of two: every step is exact
        assert np.array_equal(ref.astype(np.float64).astype(FC.LD), ref) and np.array_equal(o, ref.astype(np.float64))
    assert float(np.abs(ref.sum(axis=0)).max()) <= 1e-12 * M * n  # a centred matrix: its rows sum to zero


def test_center_reference_mirrors_the_upper_triangle():
    G = FC.int_symmetric(np.random.default_rng(5), 64)
    G[40, 3] += 7  # below the diagonal: changes the row sums, and nothing else
    ref = FC.center_reference(G)
    assert np.array_equal(ref, ref.T)
    Gw = G.sum(axis=1)
    assert ref[3, 40] == FC.LD(G[3, 40]) - FC.LD(Gw[3] + Gw[40]) / 64 + FC.LD(Gw.sum()) / 4096


def test_loco_and_eval_cases():
    Ka, Kc = np.full((3, 3), 12.0), np.full((3, 3), 4.0)
    assert np.array_equal(FC.loco_reference(Ka, 24, Kc, 8), np.full((3, 3), 16.0))
    for n in (1, 63, 64, 65, 1025):
        for seed in range(4 if n == 1 else 1):
            D, want, trace = FC.eval_case(n, seed)
            assert np.all((want == 0) | (want >= 1e-10)) and not np.any(np.signbit(want))
            if n > 1:
                assert want[3] == 1e-10 and np.all(want[:3] == 0) and sorted(np.diag(D))[2] == FC.EVAL_EDGE[1]
                assert FC.EVAL_EDGE[1] < 1e-10 and abs(trace - want.mean()) <= 1e-12 * trace


# ------------------------------------------------------------------------------------------------------------------ -lm
def test_lm_reference_against_the_oracle(oracle):
    for args in FC.lm_case_list():
        cs = FC.lm_case(*args)
        n, c = cs["n"], cs["c"]
        ref = FC.lm_reference(cs["W"], cs["y"], cs["X"])
        pv = FC.lm_pvalues(ref, n, c)
        o = oracle.lm_analyze(54, cs["W"], cs["y"], cs["X"])
        o3 = oracle.lm_analyze(53, cs["W"], cs["y"], cs["X"])
        for s, kind in enumerate(cs["kinds"]):
            if kind in ("monomorphic", "collinear"):
                assert ref["xPwx"][s] <= 1e-30 * ref["xx"][s]
            else:  # the oracle is float64 normal equations as well: the bar applies to it
                assert abs(o["beta"][s] - ref["beta"][s]) <= FC.LM_BAR * abs(ref["beta"][s]), (args, s)
                assert abs(o["se"][s] - ref["se_wald"][s]) <= FC.LM_BAR * ref["se_wald"][s], (args, s)
                assert abs(o3["se"][s] - ref["se_score"][s]) <= FC.LM_BAR * ref["se_score"][s], (args, s)
                for k in ("p_wald", "p_score", "p_lrt"):
                    p, bar, _ = pv[k]
                    assert abs(o[k][s] - p[s]) <= (bar[s] + 1e-9) * p[s], (args, s, k)  # (the oracle's own CDFs: 1e-9, as test_linear_model)
        if "single" in cs["kinds"]:
            assert np.nansum(cs["X"][3]) == 1.0


def test_lm_bar_is_the_measured_one():
    worst = FC.measure_lm_bar()
    print("measured worst relative difference of the reversed-order float64 normal equations: %.3e" % worst)
    assert worst <= FC.LM_MEASURED and worst > FC.LM_MEASURED / 2  # the recorded figure is the measurement, rounded up
    assert FC.LM_BAR == 8 * FC.LM_MEASURED


def test_a_block_of_one_snp_hands_over_its_width_as_row_stride():
    """numpy reports any stride it likes for an axis of length 1 (a one-row result of fancy indexing: 8 bytes): api.LM.Analyze
    handed that to lm_batch as ld = 1 and a block of one SNP was refused (test_lm_against_long_double_qr, l = 1)"""
    from gemma_amd import api
    one = np.zeros((1, 9))[:, np.arange(7)]
    assert one.flags.c_contiguous and api._row_ld(one) == 7 and api._row_ld(np.ascontiguousarray(one)) == 7
    wide = FC.widen(np.zeros((3, 7)), 10, 1.0)
    assert api._row_ld(wide) == 10 and api._row_ld(wide[:1]) == 7
    assert api._row_ld(np.zeros((4, 5), dtype=np.uint8)) == 5


def test_carry_case():
    G, failed = FC.carry_case()
    assert failed == (0, 3, 6, 7, 8, 12) and all(np.all(np.isnan(G[s])) for s in failed)
    assert all(not np.all(np.isnan(G[s])) for s in range(len(G)) if s not in failed)

"""Helpers of the score-panel hits tests (tests/test_score_hits_cpu.py, tests/test_gpu_score_hits.py).

select(records, p_max) restates what the hits form of the score panel hands out, from the full (T, l) records of the records form:
    hits   every pair with p_score <= p_max (a NaN p_score is never below anything), sorted by (pheno, snp);
    best   per phenotype the pair with the smallest p_score, the smallest row among equal p_score, NaN never; snp -1 and NaN
           fields where the phenotype has no pair with a p_score.
The device decides `best` on the largest finite F, and p_score falls in F, so the two agree wherever two rows of a phenotype do
not share their p_score at different F (none of the panels here has such rows at the minimum: the tests compare snp exactly)."""
import functools

import numpy as np

import multicases as mc
import scorecases as sc

HIT_DTYPE = np.dtype([("snp", "u4"), ("pheno", "u4"), ("beta", "f8"), ("se", "f8"), ("p_score", "f8")])
BEST_DTYPE = np.dtype([("beta", "f8"), ("se", "f8"), ("p_score", "f8"), ("snp", "i8")])
STATS = ("beta", "se", "p_score")
SHAPES = ((1, 17), (3, 100), (16, 17))  # (c, T)
P_MAXES = (0.05, 1e-3, 0.0, 1.0)


def select(records, p_max, offset=0):
    """(hits, best) of a (T, l) array of (beta, se, p_score) records; snp = offset + column"""
    records = np.asarray(records)
    T, l = records.shape
    p = records["p_score"]
    with np.errstate(invalid="ignore"):
        keep = p <= p_max  # False on NaN
    ts, ss = np.nonzero(keep)  # row-major: sorted by (pheno, snp)
    hits = np.zeros(len(ts), dtype=HIT_DTYPE)
    hits["snp"], hits["pheno"] = ss + offset, ts
    for k in STATS:
        hits[k] = records[k][ts, ss]
    best = np.zeros(T, dtype=BEST_DTYPE)
    for k in STATS:
        best[k] = np.nan
    best["snp"] = -1
    for t in range(T):
        ok = ~np.isnan(p[t])
        if ok.any():
            s = int(np.flatnonzero(ok)[np.argmin(p[t][ok])])  # argmin: the first of equals
            for k in STATS:
                best[k][t] = records[k][t, s]
            best["snp"][t] = s + offset
    return hits, best


def same_bits(a, b):
    """two structured arrays agree in every field, bit for bit (NaN equals NaN of the same bits)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def as_records(dev):
    """a (T, l, 3) device tensor of the records form -> (T, l) SCORE_DTYPE"""
    a = dev.cpu().numpy()
    rec = np.zeros(a.shape[:2], dtype=sc.SCORE_DTYPE)
    for j, k in enumerate(sc.FIELDS):
        rec[k] = a[:, :, j]
    return rec


def hits_of_dev(h):
    """api.ScoreHitsDev -> HIT_DTYPE array"""
    out = np.zeros(len(h.snp), dtype=HIT_DTYPE)
    out["snp"], out["pheno"] = h.snp.cpu().numpy(), h.pheno.cpu().numpy()
    st = h.stats.cpu().numpy()
    for j, k in enumerate(STATS):
        out[k] = st[:, j]
    return out


def best_of_dev(b):
    """api.ScoreBestDev -> BEST_DTYPE array"""
    out = np.zeros(len(b.snp), dtype=BEST_DTYPE)
    st = b.stats.cpu().numpy()
    for j, k in enumerate(STATS):
        out[k] = st[:, j]
    out["snp"] = b.snp.cpu().numpy()
    return out


@functools.lru_cache(maxsize=None)
def plink_panel(c=3, T=17):
    """254 individuals, 20 % dropped through the indicator, 1 % missing calls, maf >= 0.05, sum(sc.BLOCKS) SNPs, c covariates
    (the last one the intercept), T traits: raw 2-bit rows, U, eval, UtW, UtY, indicator"""
    from oracle import oracle as O
    O.lib()
    rng = np.random.default_rng(4117 + 100 * c + T)
    ni_total, p = 254, sum(sc.BLOCKS)
    ind = (rng.random(ni_total) > 0.2).astype(np.int32)
    maf = rng.uniform(0.05, 0.5, size=p)
    g = rng.binomial(2, maf[:, None], size=(p, ni_total))
    codes = np.array([3, 2, 0], dtype=np.uint8)[g]
    codes[rng.random(codes.shape) < 0.01] = 1
    raw = mc.pack_bed(codes)
    n = int(ind.sum())
    Kg = rng.binomial(2, 0.3, size=(400, n)).astype(np.float64)
    U, ev, _ = O.eigen_decomp_zeroed(O.center_matrix(O.calc_kin(Kg, 1)))
    W = np.hstack([rng.standard_normal((n, c - 1)), np.ones((n, 1))])
    gen = Kg.T @ rng.standard_normal((400, T)) / 20.0
    h2 = np.linspace(0.0, 0.95, T)
    Y = np.sqrt(h2) * gen / gen.std(axis=0) + np.sqrt(1 - h2) * rng.standard_normal((n, T))
    return raw, U, ev, U.T @ W, np.ascontiguousarray(U.T @ Y), ind


def golden_threshold(ref, lo=5):
    """p_max from tests/golden/ref_multi.npz alone: the geometric mean of two adjacent printed p_score values of the three
    phenotypes pooled and sorted, the first pair from `lo` rows up whose ratio is at least 1 + 1e-3.  Returns (p_max, rows
    below, rows in all, ratio, tables) with tables[t] = (rs names, printed p_score)."""
    tables = []
    for t in range(3):
        text = ref["assoc%d" % (t + 1)].tobytes().decode().strip().split("\n")
        hdr = text[0].split("\t")
        body = [ln.split("\t") for ln in text[1:]]
        tables.append(([r[hdr.index("rs")] for r in body], np.array([float(r[hdr.index("p_score")]) for r in body])))
    pooled = np.sort(np.concatenate([p for _, p in tables]))
    for k in range(lo, len(pooled) // 2 + 1):  # k rows lie below the gap
        if pooled[k] / pooled[k - 1] >= 1 + 1e-3:
            return float(np.sqrt(pooled[k] * pooled[k - 1])), k, len(pooled), float(pooled[k] / pooled[k - 1]), tables
    raise AssertionError("no gap of 1e-3 between adjacent printed p_score values in the golden")

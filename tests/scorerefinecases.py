"""Cases of the score panel's refinement (tests/test_score_refine_cpu.py, tests/test_gpu_score_refine.py): Wald and LRT of
(SNP, phenotype) pairs.

panel(oracle, n, c, T): the (n, c) case of tests/lmmdefcases.py -- U, eval, UtW, its planted and random rows of U^T x, its three
traits -- cut and filled to L_ROWS = 24 rows and T traits:
    rows 0 .. 21   the case's rows 0 .. 21 (its 12 planted rows first; (203, 16) has 16 rows: 16 .. 21 repeat 0 .. 5),
    row MONO       a monomorphic SNP: x = 2 for everybody, 2 U^T 1,
    row MISSING    a SNP with no called genotype: NaN,
    traits 0 .. 2  the case's (heritabilities 0, 0.3, 0.999); further traits are drawn in the rotated basis, U^T y ~ N(0, h2 eval + 1 - h2)
                   with h2 spread over 0.05 .. 0.9.
pair_lists(n, c, T): the lists of the bit tests, (m, 2) arrays of (snp, pheno).  def_sample(n, c, T): the pairs held to the
definition, per trait of the case."""
import numpy as np

import lmmdefcases as D

SHAPES = ((31, 1, 5), (65, 3, 17), (129, 4, 3), (203, 6, 4), (203, 16, 3))  # (n, c, T): FixedC<1, 4>, <3>, <4>, GenericC at 6 and 16
FORCED = (65, 2, 3)  # under GEMMA_HIP_FORCE_GENERIC=1
DEF_SHAPES = ((65, 3, 17), (203, 6, 4))
L_ROWS = 24
MONO, MISSING = 22, 23
DEF_PER_TRAIT = 12
_PANELS = {}


def panel(oracle, n, c, T):
    key = (n, c, T)
    if key not in _PANELS:
        d = D.case(oracle, n, c)
        rows = np.arange(L_ROWS - 2) % len(d["UtX"])
        UtX = np.empty((L_ROWS, n))
        UtX[:L_ROWS - 2] = d["UtX"][rows]
        UtX[MONO] = 2.0 * (d["U"].T @ np.ones(n))
        UtX[MISSING] = np.nan
        UtY = np.empty((n, T))
        k = min(T, 3)
        UtY[:, :k] = d["UtY"][:, :k]
        if T > k:
            rng = np.random.default_rng(61000 + 100 * n + 10 * c + T)
            h2 = np.linspace(0.05, 0.9, T - k)
            UtY[:, k:] = np.sqrt(np.maximum(d["ev"], 0.0)[:, None] * h2 + (1.0 - h2)) * rng.standard_normal((n, T - k))
        p = dict(U=d["U"], ev=d["ev"], UtW=d["UtW"], UtY=np.ascontiguousarray(UtY), UtX=np.ascontiguousarray(UtX), rows=rows)
        for a in p.values():
            a.setflags(write=False)
        _PANELS[key] = p
    return _PANELS[key]


def pair_lists(n, c, T):
    """name -> (m, 2) int64 array of (snp, pheno): m = 1; m = 5 (a ragged workgroup, with the monomorphic and the all-missing row);
    nine pairs in reversed (pheno, snp) order; a list with one pair three times; at (31, 1, 5) all T * L_ROWS pairs"""
    rng = np.random.default_rng(7300 + 100 * n + 10 * c + T)
    lists = {"one": np.array([[5, T - 1]]),
             "five": np.array([[0, 0], [MONO, T - 1], [13, T // 2], [MISSING, 0], [L_ROWS - 3, T - 1]])}
    nine = np.column_stack([rng.choice(L_ROWS - 2, 9, replace=False), rng.integers(0, T, 9)])
    nine = nine[np.lexsort((nine[:, 0], nine[:, 1]))]
    lists["reversed"] = nine[::-1].copy()
    rep = np.column_stack([rng.choice(L_ROWS - 2, 6, replace=False), rng.integers(0, T, 6)])
    lists["repeated"] = rep[[0, 1, 2, 1, 3, 4, 1, 5]]
    if (n, c, T) == SHAPES[0]:
        t, s = np.divmod(np.arange(T * L_ROWS), L_ROWS)
        lists["all"] = np.column_stack([s, t])
    return {k: np.ascontiguousarray(v, dtype=np.int64) for k, v in lists.items()}


def def_sample(n, c, T):
    """trait -> sorted rows of the panel (all below MONO: rows of the case itself) whose pairs are held to the definition"""
    rng = np.random.default_rng(9100 + 100 * n + 10 * c + T)
    return {t: np.sort(rng.choice(L_ROWS - 2, DEF_PER_TRAIT, replace=False)) for t in range(3)}

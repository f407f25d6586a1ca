"""Cases and plain references for the first-pass kernels: snp_qc_kernel (csrc/qc.hip.h), the ingest, transpose, centring, LOCO,
eigenvalue-zeroing and PLINK carry kernels (csrc/ingest.hip.h) and lm_assoc_kernel (csrc/lm_assoc.hip.h).

Nothing here touches the GPU, the library or the `oracle` module.  The references are written from the definitions in the
kernel headers' comments: Python integers and fractions.Fraction where the quantity is rational (QC statistics, the mean of hard
calls, the HWE exact test, centring and LOCO of integer matrices), numpy longdouble elsewhere (kinship, -lm by Householder QR).
tests/test_firstpass_cases_cpu.py checks every reference against the oracle's restatement of the same routine and every planted
row against its name; tests/test_gpu_firstpass.py holds the device to them.

The -lm bar (LM_BAR).  lm_assoc_kernel forms x'x - (W'x)'(W'W)^-1(W'x), which cancels, so no fixed rtol describes it.  The bar is
measured, never chosen and never taken from device output: lm_normal_equations() evaluates the kernel's formula in float64 numpy
with every sum taken sequentially in REVERSED order, lm_reference() is the long-double QR of [W x]; the worst relative difference
of beta-hat, the Wald se and the score se over every regular and every single-minor-allele row of lm_case_list() is

    LM_MEASURED = 1.5e-11      (measure_lm_bar() reproduces it; test_firstpass_cases_cpu.py asserts it)

and the bar is LM_FACTOR = 8 times that, for the device's different reduction tree: LM_BAR = 1.2e-10.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
U = 2.0 ** -53

N_LIST = (1, 2, 3, 63, 64, 65, 127, 129, 257)
L_LIST = (1, 3, 4, 5, 9)
PATTERNS = ("first", "last", "every_byte", "last_lane")

LM_MEASURED = 1.5e-11
LM_FACTOR = 8
LM_BAR = LM_FACTOR * LM_MEASURED


# ----------------------------------------------------------------------------------------------------------------- .bed
GENO_TO_CODE = {2: 0, 1: 2, 0: 3}  # code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing


def geno_to_codes(G):
    """0 / 1 / 2 / NaN -> the 2-bit codes of a .bed file"""
    G = np.asarray(G, dtype=np.float64)
    out = np.full(G.shape, 1, dtype=np.uint8)
    for g, code in GENO_TO_CODE.items():
        out[G == g] = code
    return out


def pack_bed(codes, ld=None, fill=0xFF):
    """codes (l x ni_total, values 0..3) -> SNP-major .bed rows: individual p sits in byte p >> 2 at bits 2 * (p & 3).  ld > the
    minimum leaves `fill` bytes behind each row; the unused lanes of the last byte hold the bits of `fill` as well."""
    codes = np.asarray(codes, dtype=np.uint8)
    l, ni = codes.shape
    nb = (ni + 3) // 4
    ld = nb if ld is None else ld
    raw = np.full((l, ld), fill, dtype=np.uint8)
    for s in range(l):
        for b in range(nb):
            v = fill
            for k in range(4):
                p = 4 * b + k
                if p < ni:
                    v = (v & ~(3 << (2 * k))) | (int(codes[s, p]) << (2 * k))
            raw[s, b] = v
    return raw


def bed_decode(raw, ni_total, indicator=None):
    """.bed rows -> doubles over the analysed individuals, NaN = missing"""
    raw = np.asarray(raw, dtype=np.uint8)
    keep = range(ni_total) if indicator is None else [p for p in range(ni_total) if indicator[p] != 0]
    value = {0: 2.0, 2: 1.0, 3: 0.0, 1: np.nan}
    out = np.empty((raw.shape[0], len(keep)))
    for s in range(raw.shape[0]):
        for j, p in enumerate(keep):
            out[s, j] = value[(int(raw[s, p >> 2]) >> (2 * (p & 3))) & 3]
    return out


# ----------------------------------------------------------------------------------------------------------- indicators
def indicator(n, pattern, rem):
    """An indicator_idv with exactly n analysed individuals and ni_total % 4 == rem.
    none: nobody dropped (rem is ignored); first / last: the first / last d individuals dropped, 1 <= d <= 4;
    every_byte: lane b % 4 of every byte b dropped (so every drop sits at another place of its byte), further drops from the
    front until n are left; last_lane: only the last individual of every byte is kept (ni_total = 4 (n - 1) + (rem or 4))."""
    if pattern == "none":
        return np.ones(n, dtype=np.int32)
    if pattern in ("first", "last"):
        d = (rem - n) % 4 or 4
        ind = np.ones(n + d, dtype=np.int32)
        if pattern == "first":
            ind[:d] = 0
        else:
            ind[n:] = 0
        return ind
    if pattern == "last_lane":
        ni = 4 * (n - 1) + (rem or 4)
        if ni == n:  # n = 1, rem = 1: a whole byte of dropped individuals in front
            ni += 4
        ind = np.zeros(ni, dtype=np.int32)
        ind[3::4] = 1
        ind[ni - 1] = 1
        if int(ind.sum()) > n:
            ind[3] = 0
        return ind
    if pattern == "every_byte":
        ni = n + 1
        while ni % 4 != rem or ni - (ni + 3) // 4 < n:
            ni += 1
        ind = np.ones(ni, dtype=np.int32)
        for b in range((ni + 3) // 4):
            ind[min(4 * b + b % 4, ni - 1)] = 0  # (the last byte may be short of lane b % 4: its last lane then)
        extra = int(ind.sum()) - n
        ind[np.flatnonzero(ind)[:extra]] = 0
        return ind
    raise ValueError(pattern)


def widen(A, ld, fill):
    """A copy of A inside rows of `ld` entries (the rest holds `fill`): returns the l x n view, whose row stride is ld"""
    buf = np.full((A.shape[0], ld), fill, dtype=A.dtype)
    buf[:, :A.shape[1]] = A
    return buf[:, :A.shape[1]]


# ------------------------------------------------------------------------------------------------------------------- QC
def hwe_exact(n_hom1, n_hom2, n_ab):
    """Wigginton, Cutler & Abecasis (2005): with N genotypes and n_A copies of the rare allele, P(h heterozygotes) is
    proportional to 2^h / (h_aa! h! h_bb!); the p-value is the mass of every h no likelier than the observed one.  Exact."""
    geno = n_hom1 + n_hom2 + n_ab
    if geno == 0:
        return Fraction(1)
    rare = 2 * min(n_hom1, n_hom2) + n_ab
    fact = [1]
    for k in range(1, geno + 1):
        fact.append(fact[-1] * k)
    w = {}
    for h in range(rare % 2, rare + 1, 2):
        aa = (rare - h) // 2
        w[h] = Fraction(2 ** h, fact[aa] * fact[h] * fact[geno - h - aa])
    return sum(v for v in w.values() if v <= w[n_ab]) / sum(w.values())


def _solve(A, b):
    """A z = b over the rationals (Gaussian elimination); None when A is singular"""
    c = len(b)
    M = [[Fraction(A[i][j]) for j in range(c)] + [Fraction(b[i])] for i in range(c)]
    for j in range(c):
        piv = next((i for i in range(j, c) if M[i][j] != 0), None)
        if piv is None:
            return None
        M[j], M[piv] = M[piv], M[j]
        for i in range(c):
            if i != j and M[i][j] != 0:
                f = M[i][j] / M[j][j]
                M[i] = [a - f * b_ for a, b_ in zip(M[i], M[j])]
    return [M[i][c] / M[i][i] for i in range(c)]


def qc_reference(G_all, ind, W, plink, maf_level=0.01, miss_level=0.05, hwe_level=0.0, r2_level=0.9999):
    """The first pass of ReadFile_geno / ReadFile_bed as csrc/qc.hip.h states it, over the analysed individuals of G_all
    (l x ni_total, NaN = missing): n_miss; maf = sum g / (2 (n - n_miss)) as ONE correctly rounded division of exact integers
    (NaN when nothing is observed); the classes n0 (0 <= g <= 0.5), n1 (0.5 < g < 1.5), n2 (1.5 <= g <= 2); and the cascade
    missingness > miss_level, maf outside [maf_level, 1 - maf_level] (unless maf_level == -1), polymorphism (BIMBAM: min < max;
    PLINK: fewer than two classes present), HWE (unless hwe_level == 0 or maf_level == -1), r2 = x'W (W'W)^-1 W'x / x'x >
    r2_level with missing calls at 2 maf (skipped for one covariate).  Comparisons are made on doubles, as the kernel's host side
    makes them; r2 and the HWE p-value are exact rationals.  Returns a dict of per-SNP lists."""
    G = np.asarray(G_all, dtype=np.float64)[:, np.asarray(ind) != 0]
    W = np.asarray(W, dtype=np.float64).reshape(G.shape[1], -1)
    l, n = G.shape
    c = W.shape[1]
    Wi = W.astype(np.int64)
    assert np.array_equal(Wi, W), "integer covariates only"
    WtW = (Wi.T @ Wi).tolist()
    out = {k: [] for k in ("indicator", "maf", "n_miss", "n0", "n1", "n2", "r2", "hwe", "why")}
    for s in range(l):
        g = G[s]
        miss = np.isnan(g)
        obs = g[~miss]
        n_miss = int(miss.sum())
        tot = sum((Fraction(float(v)) for v in obs), Fraction(0))
        maf = float(tot / (2 * (n - n_miss))) if n_miss < n else float("nan")
        n0 = int(((obs >= 0) & (obs <= 0.5)).sum())
        n1 = int(((obs > 0.5) & (obs < 1.5)).sum())
        n2 = int(((obs >= 1.5) & (obs <= 2.0)).sum())
        why, r2, hwe = None, None, None
        if float(Fraction(n_miss, n)) > miss_level:
            why = "miss"
        elif (maf < maf_level or maf > 1.0 - maf_level) and maf_level != -1:
            why = "maf"
        elif plink and ((n0 + n1) == 0 or (n1 + n2) == 0 or (n2 + n0) == 0):
            why = "poly"
        elif not plink and not (obs.size and obs.min() < obs.max()):
            why = "poly"
        if why is None and hwe_level != 0 and maf_level != -1:
            hwe = hwe_exact(n0, n2, n1)
            if hwe < Fraction(hwe_level):
                why = "hwe"
        if why is None and c != 1:
            fill = Fraction(maf) * 2
            if np.array_equal(obs, np.rint(obs)):
                oi = obs.astype(np.int64)
                Wtx = [int(Wi[~miss, a] @ oi) + fill * int(Wi[miss, a].sum()) for a in range(c)]
                v_x = int(oi @ oi) + fill * fill * n_miss
            else:
                x = [fill if m else Fraction(float(v)) for v, m in zip(g, miss)]
                Wtx = [sum(int(Wi[i, a]) * x[i] for i in range(n)) for a in range(c)]
                v_x = sum(v * v for v in x)
            z = _solve(WtW, Wtx)
            r2 = sum(a * b for a, b in zip(Wtx, z)) / v_x
            if r2 > Fraction(r2_level):
                why = "r2"
        for k, v in (("indicator", 0 if why else 1), ("maf", maf), ("n_miss", n_miss), ("n0", n0), ("n1", n1), ("n2", n2), ("r2", r2),
                     ("hwe", hwe), ("why", why)):
            out[k].append(v)
    return out


def int_covariates(rng, n, c):
    """n x c integers with |w| <= 4, the intercept last, W'W non-singular"""
    while True:
        W = np.hstack([rng.integers(-4, 5, size=(n, c - 1)), np.ones((n, 1), dtype=np.int64)]).astype(np.float64)
        if np.linalg.matrix_rank(W) == c:
            return W


def _place(rng, n, counts):
    """a row over n individuals with counts = {value: how many}, the rest NaN, at random places"""
    row = np.full(n, np.nan)
    vals = np.concatenate([np.full(k, v, dtype=np.float64) for v, k in counts.items()]) if counts else np.zeros(0)
    assert len(vals) <= n
    row[rng.permutation(n)[:len(vals)]] = vals
    return row


def qc_sweep_case(n, pattern, rem, plink, seed):
    """Nine SNPs over ni_total individuals for the statistics sweep: rows 0, 2, 4, 6, 8 are polymorphic and complete (row 4 with
    one missing call once n >= 40), rows 1, 3, 5, 7 are: all missing among the analysed (observed among the dropped), 30 %
    missing, monomorphic, one observed call.  The dropped individuals hold calls of their own everywhere.  n = 1 admits no
    polymorphic row and one covariate only."""
    rng = np.random.default_rng(seed)
    ind = indicator(n, pattern, rem)
    ni = ind.size
    c = min(3, max(1, n - 1))
    W = int_covariates(rng, n, c)
    G = rng.integers(0, 3, size=(9, ni)).astype(np.float64)  # what the dropped individuals hold
    sel = np.flatnonzero(ind)
    for s in range(9):
        if s % 2 == 0:
            while True:
                row = rng.binomial(2, rng.uniform(0.2, 0.5), size=n).astype(np.float64)
                if n == 1 or (len(set(row.tolist())) > 1 and 0.05 <= row.sum() / (2 * n) <= 0.95):
                    break
            if s == 4 and n >= 40:
                row[rng.integers(n)] = np.nan
        elif s == 1:
            row = np.full(n, np.nan)
        elif s == 3:
            row = rng.integers(0, 3, size=n).astype(np.float64)
            row[rng.permutation(n)[:max(1, (3 * n + 9) // 10)]] = np.nan
        elif s == 5:
            row = np.full(n, float(rng.integers(0, 3)))
        else:
            row = _place(rng, n, {float(rng.integers(0, 3)): 1})
        G[s, sel] = row
    return {"n": n, "ind": ind, "W": W, "G": G, "plink": plink, "cfg": dict(maf_level=0.05, miss_level=0.05)}


def qc_sweep_list():
    """every n with every indicator pattern; ni_total % 4 and the encoding rotate so that each takes every value"""
    out = []
    k = 0
    for n in N_LIST:
        for pattern in PATTERNS:
            out.append((n, pattern, k % 4, (k // 4 + k) % 2 == 0, 1000 + k))
            k += 1
    return out


QC_PLANT_N = 64
QC_PLANT_CFG = dict(maf_level=0.125, miss_level=4.0 / 64.0, hwe_level=0.0, r2_level=0.9999)
QC_PLANT_HWE = 0.01


def qc_planted_case(plink, seed=77):
    """n = 64 analysed of 86 (one drop in every byte): miss_level = 4/64 and maf_level = 8/64 are exact in binary.  Returns the case
    and {name: row}.  W = [h, integers, 1] with h a hard-call vector, so that the row `equals_covariate` has r2 = 1."""
    rng = np.random.default_rng(seed)
    n = QC_PLANT_N
    ind = indicator(n, "every_byte", 2)
    ni = ind.size
    sel = np.flatnonzero(ind)
    h = rng.binomial(2, 0.4, size=n).astype(np.float64)
    W = np.column_stack([h, rng.integers(-4, 5, size=n).astype(np.float64), np.ones(n)])
    assert np.linalg.matrix_rank(W) == 3
    rows = {
        "all_missing_analysed": {},
        "one_observed": {1.0: 1},
        "mono0": {0.0: 64}, "mono1": {1.0: 64}, "mono2": {2.0: 64},
        "no_class0": {1.0: 20, 2.0: 44}, "no_class1": {0.0: 40, 2.0: 24}, "no_class2": {0.0: 44, 1.0: 20},
        "miss_at_level": {0.0: 24, 1.0: 24, 2.0: 12},         # 4 missing of 64: 4/64 > 4/64 is false, kept
        "miss_above_level": {0.0: 23, 1.0: 24, 2.0: 12},      # 5 missing: dropped
        "maf_at_level": {0.0: 50, 1.0: 12, 2.0: 2},           # sum 16: maf = 16/128 = maf_level, kept
        "maf_below_level": {0.0: 51, 1.0: 11, 2.0: 2},        # sum 15: dropped
        "maf_at_one_minus_level": {0.0: 2, 1.0: 12, 2.0: 50},  # sum 112: maf = 1 - maf_level, kept
        "maf_above_one_minus_level": {0.0: 2, 1.0: 11, 2.0: 51},  # sum 113: dropped
        "no_het": {0.0: 32, 2.0: 32},                         # fails HWE whenever HWE is on
        "regular": {0.0: 25, 1.0: 30, 2.0: 9},
    }
    if not plink:  # class boundaries of dosages: 0.5 counts as n0, 1.5 as n2 (16 / 32 / 16 is in HWE; anything else is far from it)
        rows["dosage_boundaries"] = {0.5: 16, 1.0: 32, 1.5: 16}
    names = list(rows) + ["equals_covariate"]
    G = rng.integers(0, 3, size=(len(names), ni)).astype(np.float64)
    for s, name in enumerate(names):
        G[s, sel] = h if name == "equals_covariate" else _place(rng, n, rows[name])
    return {"n": n, "ind": ind, "W": W, "G": G, "plink": plink, "cfg": dict(QC_PLANT_CFG)}, {k: i for i, k in enumerate(names)}


HWE_COUNTS = ((20, 20, 0), (0, 0, 40), (0, 0, 2), (30, 5, 10), (5, 30, 10), (16, 16, 32), (40, 2, 6), (1, 1, 0), (12, 0, 8))


def hwe_case(plink, seed=5):
    """(n_hom1, n_hom2, n_ab) planted among n = 64 analysed individuals (the rest of each row is missing; the call sets
    miss_level = 1 and maf_level = 0, so only polymorphism and HWE decide): no heterozygotes, only heterozygotes, n_hom1 >
    n_hom2 and its mirror.  The fp64 rows use two dosages per class (0 / 0.25, 0.75 / 1.25, 1.75 / 2) so that even the
    only-heterozygotes rows are polymorphic; the PLINK rows hold the triples with at least two classes."""
    rng = np.random.default_rng(seed)
    n = 64
    ind = indicator(n, "last", 1)
    sel = np.flatnonzero(ind)
    trip = [t for t in HWE_COUNTS if not plink or sum(1 for v in t if v) >= 2]
    G = rng.integers(0, 3, size=(len(trip), ind.size)).astype(np.float64)
    for s, (h1, h2, ab) in enumerate(trip):
        if plink:
            counts = {0.0: h1, 2.0: h2, 1.0: ab}
        else:
            counts = {}
            for lo, hi, k in ((0.0, 0.25, h1), (1.75, 2.0, h2), (0.75, 1.25, ab)):
                if k:
                    counts[lo] = (k + 1) // 2
                if k // 2:
                    counts[hi] = k // 2
        G[s, sel] = _place(rng, n, {v: k for v, k in counts.items() if k})
    return {"n": n, "ind": ind, "W": np.ones((n, 1)), "G": G, "plink": plink}, trip


def hwe_levels(trip):
    """a level ten times above and one ten times below every triple's exact p-value"""
    lv = set()
    for t in trip:
        p = float(hwe_exact(*t))
        lv.add(p * 10.0)
        lv.add(p / 10.0)
    return sorted(lv)


# -------------------------------------------------------------------------------------------------------------- ingest
def impute_reference(X):
    """mean imputation of ingest_lmm_kernel: hard calls, so the mean is one correctly rounded division of integers; a row
    without an observed call is NaN throughout"""
    X = np.array(X, dtype=np.float64)
    for s in range(X.shape[0]):
        miss = np.isnan(X[s])
        obs = X[s][~miss]
        mean = float(sum((Fraction(float(v)) for v in obs), Fraction(0)) / len(obs)) if len(obs) else float("nan")
        X[s][miss] = mean
    return X


def hard_calls(rng, l, n, miss=0.1):
    G = rng.integers(0, 3, size=(l, n)).astype(np.float64)
    G[rng.random(G.shape) < miss] = np.nan
    return G


# ------------------------------------------------------------------------------------------------------------- kinship
def kin_case(n, seed, p=37):
    """p = 37 hard-call SNPs over n individuals with missing calls; row 5 monomorphic (variance 0: not scaled, contributes zeros),
    row 11 with a single observed call.  No row is missing throughout: QC removes such a SNP before the kinship is formed."""
    rng = np.random.default_rng(seed)
    G = hard_calls(rng, p, n, miss=0.1 if n > 3 else 0.0)
    for s in range(p):
        if np.all(np.isnan(G[s])):
            G[s, rng.integers(n)] = 1.0
    G[5] = 2.0
    G[11] = np.nan
    G[11, rng.integers(n)] = 1.0
    return G


def kin_reference(G, k_mode):
    """ingest_kin_kernel + X X^T / p in long double.  Returns (K, bound): bound[i][j] is what float64 arithmetic may differ by.

    Row s is a_s = (g - mean) * sc, sc = 1 / sqrt(var), var = (sum g^2 + mean^2 n_miss) / n - mean^2 (k_mode 2, var != 0).
    float64 rounds: the mean (1), the subtraction (1), and for k_mode 2 the product with sc (1), sqrt and the reciprocal (2) and
    var itself, whose three terms cancel: each of its 6 operations errs by at most u * T, T = sum g^2 / n + 2 mean^2, so var has
    relative error <= 6 u T / var and sc half of that.  Hence |fl(a) - a| <= e_s |a| + u |mean| sc with
    e_s = u (2 + [k_mode 2] (3 + 3 T / var)): the mean's own rounding shifts every entry by u |mean| sc, also where a is small.
    The product: a dot product of p terms in any order errs by p u sum |a_i b_i| (Higham, Accuracy and Stability, 3.1), the
    operands' errors add (2 e_s |a_i a_j| + u |mean| sc (|a_i| + |a_j|)) per term, and the scale 1 / p is two more roundings."""
    G = np.asarray(G, dtype=np.float64)
    p, n = G.shape
    A = np.zeros((p, n), dtype=LD)
    e = np.zeros(p, dtype=LD)
    shift = np.zeros(p, dtype=LD)
    for s in range(p):
        miss = np.isnan(G[s])
        obs = G[s][~miss].astype(LD)
        mean = obs.sum() / LD(len(obs))
        sq = (obs * obs).sum()
        var = (sq + mean * mean * LD(int(miss.sum()))) / LD(n) - mean * mean
        x = np.where(miss, mean, G[s].astype(LD)) - mean
        sc = LD(1)
        e[s] = 2 * U
        if k_mode == 2 and var != 0:
            sc = 1 / np.sqrt(var)
            e[s] = U * (5 + 3 * (sq / LD(n) + 2 * mean * mean) / var)
        A[s] = x * sc
        shift[s] = U * abs(mean) * sc
    K = (A.T @ A) / LD(p)
    absA = np.abs(A)
    S = absA.T @ absA
    bound = (p * U * S + 2 * (absA * e[:, None]).T @ absA + (absA * shift[:, None]).T @ np.ones((p, n), dtype=LD)
             + np.ones((n, p), dtype=LD) @ (absA * shift[:, None])) / LD(p) * (1 + 4 * U) + 2 * U * np.abs(K)
    return K, bound


# ------------------------------------------------------------------------------------------ centring, LOCO, eigenvalues
def int_symmetric(rng, n, hi=512):
    A = rng.integers(-hi, hi + 1, size=(n, n))
    return (np.triu(A) + np.triu(A, 1).T).astype(np.float64)


def center_reference(G):
    """CenterMatrix as csrc/ingest.hip.h states it, for an integer matrix: Gw = G 1 (row sums of G as given), d = sum Gw,
    G[i][j] + -(Gw[i] + Gw[j]) / n + d / n^2 on the UPPER triangle, the lower triangle its mirror.  Formed as the integer
    n^2 G - n (Gw_i + Gw_j) + d over n^2: below 2^63, so the one long-double division is correctly rounded."""
    Gi = np.asarray(G).astype(np.int64)
    assert np.array_equal(Gi, G)
    n = Gi.shape[0]
    Gw = Gi.sum(axis=1)
    d = int(Gw.sum())
    num = n * n * Gi - n * (Gw[:, None] + Gw[None, :]) + d
    assert np.abs(num).max() < 2 ** 62
    num = np.triu(num) + np.triu(num, 1).T
    return num.astype(LD) / LD(n * n)


# float64 against center_reference for an integer G with M = max |G| (row sums and the total are exact): alpha = -1 / n is rounded
# and so is each product alpha Gw (|.| <= M: 2 u M each), their sum (|.| <= 2 M: 2 u M), the sum with G (<= 3 M: 3 u M), beta =
# d / n^2 (<= M: u M) and the last sum (<= 4 M: 4 u M) -- three additions and the scalings, 14 u M in all
CENTER_ULPS = 14


def loco_reference(Ka, nsa, Kc, nsc):
    Ka = np.asarray(Ka).astype(np.int64)
    Kc = np.asarray(Kc).astype(np.int64)
    return (nsa * Ka - nsc * Kc).astype(LD) / LD(nsa - nsc)


EVAL_EDGE = (1e-10, float(np.nextafter(1e-10, 0.0)), -0.5, -0.0)  # kept (the test is <), zeroed, zeroed, zeroed


def eval_case(n, seed):
    """a diagonal matrix (eigenvalues in random order on the diagonal) holding EVAL_EDGE, and what EigenDecomp_Zeroed returns
    for it: ascending eigenvalues with every value < 1e-10 at +0, and their mean"""
    rng = np.random.default_rng(seed)
    if n == 1:
        ev = np.array([EVAL_EDGE[seed % 4]])
    else:
        rest = rng.integers(1, 1 << 20, size=max(0, n - 4)) / 1024.0
        ev = np.concatenate([EVAL_EDGE, rest])[:n]
    ev = rng.permutation(ev)
    want = np.sort(ev)
    want = np.where(want < 1e-10, 0.0, want)
    trace = float(want.astype(LD).sum() / LD(n))
    return np.diag(ev), want, trace


# ------------------------------------------------------------------------------------------------------------------ -lm
def _householder_qr(A):
    """R and the reflectors of A (m x k, long double)"""
    A = np.array(A, dtype=LD)
    m, k = A.shape
    vs = []
    for j in range(k):
        x = A[j:, j].copy()
        alpha = -np.copysign(np.sqrt((x * x).sum()), x[0])
        v = x
        v[0] -= alpha
        nv = (v * v).sum()
        if nv != 0:
            A[j:, j:] -= np.outer(v, (2 / nv) * (v @ A[j:, j:]))
        vs.append((v, nv))
    return A, vs


def _apply_qt(vs, y):
    y = np.array(y, dtype=LD)
    for j, (v, nv) in enumerate(vs):
        if nv != 0:
            y[j:] -= v * ((2 / nv) * (v @ y[j:]))
    return y


def lm_reference(W, y, X):
    """OLS of y on [W x] for every row x of X (mean-imputed first) by long-double Householder QR: with Q^T y = q and R the
    triangle, beta-hat = q_c / R_cc, x'P_w x = R_cc^2, y'P_w y = sum_{i >= c} q_i^2, y'P_wx y = sum_{i > c} q_i^2; the Wald se
    sqrt(y'P_wx y / (df x'P_w x)), the score se sqrt(y'P_w y / (n x'P_w x)), the LRT statistic n log(y'P_w y / y'P_wx y), df =
    n - c - 1.  Returns long-double arrays beta, se_wald, se_score, lrt, xPwx, xx."""
    W = np.asarray(W, dtype=np.float64).reshape(len(y), -1)
    n, c = W.shape
    X = impute_reference(X)
    df = LD(n - c - 1)
    out = {k: np.zeros(X.shape[0], dtype=LD) for k in ("beta", "se_wald", "se_score", "lrt", "xPwx", "xx")}
    for s in range(X.shape[0]):
        R, vs = _householder_qr(np.column_stack([W, X[s]]))
        q = _apply_qt(vs, y)
        rcc = R[c, c]
        yPxy = (q[c + 1:] ** 2).sum()
        yPwy = yPxy + q[c] ** 2
        xPwx = rcc * rcc
        with np.errstate(divide="ignore", invalid="ignore"):
            out["beta"][s] = q[c] / rcc
            out["se_wald"][s] = np.sqrt(yPxy / (df * xPwx))
            out["se_score"][s] = np.sqrt(yPwy / (LD(n) * xPwx))
            out["lrt"][s] = LD(n) * np.log(yPwy / yPxy)
        out["xPwx"][s] = xPwx
        out["xx"][s] = (X[s].astype(LD) ** 2).sum()
    return out


def _rsum(a):
    """sequential float64 sum, last element first"""
    return np.cumsum(np.asarray(a, dtype=np.float64)[::-1])[-1] if len(a) else np.float64(0.0)


def lm_normal_equations(W, y, X):
    """lm_assoc_kernel's formula in float64 numpy with reversed sequential sums -- the yardstick of LM_BAR, not a reference"""
    W = np.asarray(W, dtype=np.float64).reshape(len(y), -1)
    n, c = W.shape
    X = impute_reference(X)
    WtW = np.array([[_rsum(W[:, a] * W[:, b]) for b in range(c)] for a in range(c)])
    WtWi = np.linalg.inv(WtW)
    Wty = np.array([_rsum(W[:, a] * y) for a in range(c)])
    yPwy = _rsum(y * y) - _rsum([_rsum(WtWi[a] * Wty) * Wty[a] for a in range(c)])
    df = np.float64(n - c - 1)
    out = {k: np.zeros(X.shape[0]) for k in ("beta", "se_wald", "se_score")}
    for s in range(X.shape[0]):
        x = X[s]
        Wtx = np.array([_rsum(W[:, a] * x) for a in range(c)])
        t = np.array([_rsum(WtWi[a] * Wtx) for a in range(c)])
        xPwx = _rsum(x * x) - _rsum(t * Wtx)
        xPwy = _rsum(x * y) - _rsum(t * Wty)
        with np.errstate(divide="ignore", invalid="ignore"):
            yPxy = yPwy - xPwy * xPwy / xPwx
            out["beta"][s] = xPwy / xPwx
            out["se_wald"][s] = np.sqrt(yPxy / (df * xPwx))
            out["se_score"][s] = np.sqrt(yPwy / (n * xPwx))
    return out


LM_NKINDS = ("c+2", 63, 64, 65, 129)
LM_CS = (1, 2, 16)


def lm_case(nkind, c, l, seed):
    """n analysed individuals behind an indicator that drops one individual in every byte; W = [hard-call column, normals, 1]
    (c = 1: the intercept alone), y normal plus an effect of row 0.  l = 1: one regular row.  l = 5: rows 0 and 4 regular, row
    1 monomorphic (x'P_w x = 0), row 2 equal to the first covariate (c >= 2; c = 1: regular), row 3 a single minor allele."""
    rng = np.random.default_rng(seed)
    n = c + 2 if nkind == "c+2" else nkind
    ind = indicator(n, "every_byte", seed % 4)
    sel = np.flatnonzero(ind)
    while True:
        h = rng.integers(0, 3, size=n).astype(np.float64)
        W = np.column_stack([h] + [rng.standard_normal(n) for _ in range(c - 2)] + [np.ones(n)]) if c >= 2 else np.ones((n, 1))
        if np.linalg.matrix_rank(W) == c and (c == 1 or len(set(h.tolist())) > 1):
            break
    kinds = ["regular"] if l == 1 else ["regular", "monomorphic", "collinear" if c >= 2 else "regular", "single", "regular"]
    G = rng.integers(0, 3, size=(l, ind.size)).astype(np.float64)
    for s, kind in enumerate(kinds):
        if kind == "regular":
            while True:
                row = hard_calls(rng, 1, n, miss=0.05 if n > 20 else 0.0)[0]
                x = impute_reference(row[None, :])[0]
                res = x - W @ np.linalg.lstsq(W, x, rcond=None)[0]
                if res @ res > 1e-3 * (x @ x):  # not (nearly) in the span of W
                    break
        elif kind == "monomorphic":
            row = np.full(n, 1.0)
        elif kind == "collinear":
            row = h.copy()
        else:
            row = np.zeros(n)
            row[rng.integers(n)] = 1.0
        G[s, sel] = row
    X = G[:, sel]
    y = rng.standard_normal(n) + 0.5 * np.nan_to_num(X[0], nan=1.0)
    return {"n": n, "c": c, "ind": ind, "W": W, "y": y, "G": G, "X": X, "kinds": kinds}


def lm_case_list():
    return [(nk, c, l, 4000 + 100 * i + 10 * j + l) for i, nk in enumerate(LM_NKINDS) for j, c in enumerate(LM_CS) for l in (1, 5)]


def measure_lm_bar():
    """the worst relative difference between lm_normal_equations and lm_reference over the regular and single-minor-allele rows
    of lm_case_list() (the monomorphic and collinear rows have x'P_w x = 0: nothing to be relative to)"""
    worst = 0.0
    for args in lm_case_list():
        cs = lm_case(*args)
        ref = lm_reference(cs["W"], cs["y"], cs["X"])
        ne = lm_normal_equations(cs["W"], cs["y"], cs["X"])
        for s, kind in enumerate(cs["kinds"]):
            if kind in ("regular", "single"):
                for k in ("beta", "se_wald", "se_score"):
                    worst = max(worst, float(abs(LD(ne[k][s]) - ref[k][s]) / abs(ref[k][s])))
    return worst


def lm_pvalues(ref, n, c):
    """p_wald, p_score (F(1, df) upper tails) and p_lrt (chi-square, 1 df) of the reference statistics, with the relative bar of
    each: a statistic t = (beta / se)^2 carries 2 (LM_BAR + LM_BAR), and p = Q(t) turns a relative change of t into
    t |Q'(t)| / Q(t) times as much; the LRT statistic n (log y'P_w y - log y'P_wx y) carries the ABSOLUTE error n (2 LM_BAR +
    2 LM_BAR) (y'P_wx y = df x'P_w x se^2: the squares of two quantities under the bar), turned into |Q'| / Q times as much."""
    from scipy import stats
    df = n - c - 1
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        for name, se in (("p_wald", ref["se_wald"]), ("p_score", ref["se_score"])):
            t = np.asarray((ref["beta"] / se) ** 2, dtype=np.float64)
            p = stats.f.sf(t, 1, df)
            gain = np.where(p > 0, t * stats.f.pdf(t, 1, df) / p, np.inf)
            out[name] = (p, 4 * LM_BAR * np.maximum(gain, 1.0), stats.f.logsf(t, 1, df) / np.log(10.0))
        t = np.asarray(ref["lrt"], dtype=np.float64)
        p = stats.chi2.sf(t, 1)
        gain = np.where(p > 0, stats.chi2.pdf(t, 1) / p, np.inf)
        out["p_lrt"] = (p, 4 * LM_BAR * (1.0 + n * gain), stats.chi2.logsf(t, 1) / np.log(10.0))
    return out


# --------------------------------------------------------------------------------------------------------- carry chain
def carry_case(seed=9, n=40, l=14):
    """l = 14 hard-call SNPs over n individuals for AnalyzePlink in batches of 4 (0-3, 4-7, 8-11, 12-13).  Rows missing throughout
    (a failed SNP: logl_H1 is NaN) at 0 (position 0 of the first batch), 3 (the last position of a batch), 6, 7, 8 (a run of
    three across the boundary 7 | 8) and 8, 12 (position 0 of a later batch)."""
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(l, n)).astype(np.float64)
    G[rng.random(G.shape) < 0.05] = np.nan
    failed = (0, 3, 6, 7, 8, 12)
    for s in failed:
        G[s] = np.nan
    return G, failed

"""Inputs and restatements shared by tests/test_cor_host.py and tests/test_gpu_cor.py (-calccor, VARCOV of src/varcov.cpp):

* the reference's files tests/golden/text/C188ns / C188bp / CBXD .cor.txt.gz (tests/golden/make_cor_fixtures.py), parsed;
* the inputs of those runs, rebuilt without the reference tree: issue188 from tests/golden/ref_issue188.npz (its .bed byte for byte,
  phenotype column 6, the indices of the analysed SNPs) with chr / rs / ps / alleles of the analysed SNPs from the golden file
  itself -- the 150 filtered SNPs get chromosome "1" like every other SNP of that set and position 0, which CalcNB never reads
  (src/varcov.cpp:190-211 looks at the chromosome and the indicator of a filtered SNP only); BXD from the committed text files;
* numpy restatements: the column x = c (g - mu) of Plink_ReadOneSNP / Bimbam_ReadOneSNP (src/gemma_io.cpp:1069-1184), Calc_Cor
  (src/varcov.cpp:220-238) in fp64 and long double, and the exact value of the integer route from Python integers."""
import decimal
import functools
import gzip
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TXT = os.path.join(GOLDEN, "text")
WINDOWS = {"C188ns": dict(window_ns=12), "C188bp": dict(window_bp=300), "CBXD": dict(window_bp=35000)}
PRINT_RTOL, PRINT_ATOL = 1e-6, 1e-12  # the file carries 7 significant digits


@functools.lru_cache(maxsize=None)
def golden(tag):
    """records of a .cor.txt: dict(text = the 8 leading fields as strings, window, var, cor (array))"""
    out = []
    with gzip.open(os.path.join(TXT, tag + ".cor.txt.gz"), "rt") as f:
        header = f.readline().split()
        assert header == ["chr", "rs", "ps", "n_mis", "n_obs", "allele1", "allele0", "af", "window_size", "var", "cor"]
        for line in f:
            t = line.rstrip("\n").split("\t")
            cor = np.array([], dtype=np.float64) if t[10] == "NA" else np.array([float(v) for v in t[10].split(",")])
            out.append(dict(text=t[:8], window=int(t[8]), var=float(t[9]), cor=cor))
    return out


def decode_bed(rows, ni):
    """PLINK 2-bit rows -> float64 with NaN (code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing)"""
    rows = np.asarray(rows, dtype=np.uint8)
    codes = np.stack([(rows >> (2 * k)) & 3 for k in range(4)], axis=-1).reshape(rows.shape[0], -1)[:, :ni]
    return np.array([2.0, np.nan, 1.0, 0.0])[codes]


def encode_bed(G):
    """float matrix of 0 / 1 / 2 / NaN (SNP-major) -> PLINK 2-bit rows"""
    p, n = G.shape
    code = np.full((p, (n + 3) // 4 * 4), 3, dtype=np.uint8)  # the padding of the last byte is never read
    c = np.where(np.isnan(G), 1, np.where(G == 2, 0, np.where(G == 1, 2, 3))).astype(np.uint8)
    code[:, :n] = c
    code = code.reshape(p, -1, 4)
    return np.ascontiguousarray(code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6))


@functools.lru_cache(maxsize=None)
def issue188():
    """dict(bed (2000 x 252 uint8), ni_total, indicator_idv, indicator_snp, chr, cM, bp over all SNPs, keep = analysed indices)"""
    fx = np.load(os.path.join(GOLDEN, "ref_issue188.npz"))
    ni = int(fx["n_total"])
    nb = (ni + 3) // 4
    bed = np.ascontiguousarray(fx["bed"][3:].reshape(-1, nb))
    ind = np.array([0 if s in ("-9", "NA") else 1 for s in fx["pheno_col6"]], dtype=np.int32)
    keep = np.asarray(fx["lmm1_snp"], dtype=np.int64)
    ns = bed.shape[0]
    ind_snp = np.zeros(ns, dtype=np.int32)
    ind_snp[keep] = 1
    rec = golden("C188bp")
    assert len(rec) == keep.size
    chr_, bp = ["1"] * ns, np.zeros(ns, dtype=np.int64)
    rs, a1, a0 = ["f%d" % t for t in range(ns)], ["A"] * ns, ["C"] * ns
    for j, t in enumerate(keep):
        chr_[t], rs[t], bp[t], a1[t], a0[t] = rec[j]["text"][0], rec[j]["text"][1], int(rec[j]["text"][2]), rec[j]["text"][5], rec[j]["text"][6]
    return dict(bed=bed, ni_total=ni, indicator_idv=ind, indicator_snp=ind_snp, chr=chr_, cM=np.zeros(ns), bp=bp, keep=keep, rs=rs, a1=a1,
                a0=a0, pheno=[str(s) for s in fx["pheno_col6"]])


def write_issue188_plink(prefix):
    """the set as .bed / .bim / .fam files (the rebuilt .bim: see the module docstring)"""
    d = issue188()
    with open(prefix + ".bed", "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(d["bed"].tobytes())
    with open(prefix + ".bim", "w") as f:
        for t in range(d["bed"].shape[0]):
            f.write("%s\t%s\t0\t%d\t%s\t%s\n" % (d["chr"][t], d["rs"][t], d["bp"][t], d["a1"][t], d["a0"][t]))
    with open(prefix + ".fam", "w") as f:
        for i, v in enumerate(d["pheno"]):
            f.write("f%d i%d 0 0 1 %s\n" % (i, i, v))


@functools.lru_cache(maxsize=None)
def bxd():
    """dict(G (p x 198 with NaN), ni_total, indicator_idv, rs, a1, a0, chr, cM, bp): the -g / -p / -a inputs of CBXD"""
    rs, a1, a0, rows = [], [], [], []
    with gzip.open(os.path.join(TXT, "bxd_mean_genotypes.txt.gz"), "rt") as f:
        for line in f:
            t = line.replace(",", " ").split()
            if not t:
                continue
            rs.append(t[0]); a1.append(t[1]); a0.append(t[2])
            rows.append([np.nan if v == "NA" else float(v) for v in t[3:]])
    G = np.array(rows)
    with gzip.open(os.path.join(TXT, "bxd_trait.txt.gz"), "rt") as f:
        tok = [l.split()[0] for l in f if l.strip()]
    ind = np.array([0 if t == "NA" else 1 for t in tok], dtype=np.int32)
    anno = {}
    with gzip.open(os.path.join(TXT, "bxd_anno.txt.gz"), "rt") as f:
        for line in f:
            t = line.replace(",", " ").split()
            if t:
                anno[t[0]] = (t[2], int(t[1]), float(t[3]) if len(t) > 3 else -9.0)  # ReadFile_anno, src/gemma_io.cpp:222-297
    chr_ = [anno[r][0] if r in anno else "-9" for r in rs]
    bp = np.array([anno[r][1] if r in anno else -9 for r in rs], dtype=np.int64)
    cM = np.array([anno[r][2] if r in anno else -9.0 for r in rs])
    return dict(G=G, ni_total=G.shape[1], indicator_idv=ind, rs=rs, a1=a1, a0=a0, chr=chr_, cM=cM, bp=bp)


# ------------------------------------------------------------------------------------------------------------ restatements
def calc_nb(indicator_snp, chr_, cM, bp, window_cm=0, window_bp=0, window_ns=0):
    """VARCOV::CalcNB (src/varcov.cpp:168-217) written from its definition, not its loop: for an analysed SNP t that is usable, the
    analysed SNPs after it on the same unbroken run of its chromosome are taken while each passes the distance tests and fewer
    than window_ns are taken."""
    if window_cm == 0 and window_bp == 0 and window_ns == 0:
        window_bp = 1000000
    ns = len(indicator_snp)
    out = np.zeros(ns, dtype=np.int32)
    for t in range(ns):
        if not indicator_snp[t] or chr_[t] == "-9" or (cM[t] == -9 and window_cm != 0) or (bp[t] == -9 and window_bp != 0):
            continue
        k = 0
        for u in range(t + 1, ns):
            if chr_[u] != chr_[t]:
                break
            if not indicator_snp[u]:
                continue
            if window_cm != 0 and not cM[u] - cM[t] < window_cm:
                break
            if window_bp != 0 and not bp[u] - bp[t] < window_bp:
                break
            if window_ns != 0 and not k < window_ns:
                break
            k += 1
        out[t] = k
    return out


def centred(G_test, dtype=np.float64):
    """rows of called genotypes with NaN -> x = c (g - mu), mu = sum g / sum c (a row without a call: NaN)"""
    G = np.asarray(G_test, dtype=dtype)
    c = ~np.isnan(G)
    g = np.where(c, G, dtype(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = g.sum(axis=1) / c.sum(axis=1).astype(dtype)
    return np.where(c, g - mu[:, None], np.where(np.isnan(mu)[:, None], dtype(np.nan), dtype(0)))


def calc_cor(G_test, n_nb, dtype=np.float64):
    """Calc_Cor per analysed SNP: (var, cor, off) with cor[off[t]:off[t + 1]] the window of SNP t"""
    X = centred(G_test, dtype)
    n = X.shape[1]
    v = (X * X).sum(axis=1)
    off = np.zeros(len(n_nb) + 1, dtype=np.int64)
    np.cumsum(n_nb, out=off[1:])
    cor = np.zeros(int(off[-1]), dtype=dtype)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t, w in enumerate(n_nb):
            if w:
                nbr = X[t + 1:t + 1 + w]
                cor[off[t]:off[t + 1]] = (nbr @ X[t]) / np.sqrt(v[t] * v[t + 1:t + 1 + w])
        var = v[:len(n_nb)] / dtype(n)
    return var, cor, off


def exact_cor(G_test, n_nb):
    """the integer route's value, rounded once: numI / sqrt(Da Nb Db Na) and D / (N n) from Python integers (60 digits);
    also the masks of the pairs / SNPs whose value is 0 / 0"""
    G = np.asarray(G_test)
    c = ~np.isnan(G)
    g = np.where(c, G, 0).astype(np.int64)
    ci = c.astype(np.int64)
    n = G.shape[1]
    P1, P2, P3, P4 = g @ g.T, ci @ g.T, g @ ci.T, ci @ ci.T  # int64: exact at these sizes
    N, S, S2 = [int(v) for v in ci.sum(1)], [int(v) for v in g.sum(1)], [int(v) for v in (g * g).sum(1)]
    D = [N[t] * S2[t] - S[t] * S[t] for t in range(len(N))]
    off = np.zeros(len(n_nb) + 1, dtype=np.int64)
    np.cumsum(n_nb, out=off[1:])
    cor = np.zeros(int(off[-1]))
    ctx = decimal.Context(prec=60)
    var = np.array([float(ctx.divide(decimal.Decimal(D[t]), decimal.Decimal(N[t] * n))) if N[t] else np.nan for t in range(len(n_nb))])
    for t, w in enumerate(n_nb):
        for k in range(1, int(w) + 1):
            b = t + k
            num = int(P1[t, b]) * N[t] * N[b] - S[t] * N[b] * int(P2[t, b]) - S[b] * N[t] * int(P3[t, b]) + S[t] * S[b] * int(P4[t, b])
            q = D[t] * N[b] * D[b] * N[t]
            cor[off[t] + k - 1] = float(ctx.divide(decimal.Decimal(num), ctx.sqrt(decimal.Decimal(q)))) if q else np.nan
    return var, cor, off


def snpinfo_of(G_test, text):
    """(chr, rs, ps, n_miss, n_idv, a_minor, a_major, maf) per analysed SNP: chr / rs / ps / alleles from `text` (the golden file's
    own fields stand for the .bim / annotation), the counts and the frequency from the genotypes as the first pass computes them
    (src/gemma_io.cpp:700-760 / :960-1030: maf = sum g / (2 called), n_idv = ni_test - n_miss)."""
    G = np.asarray(G_test)
    c = ~np.isnan(G)
    n_miss = (~c).sum(1)
    maf = np.where(c, G, 0).sum(1) / (2.0 * c.sum(1))
    return [(t[0], t[1], int(t[2]), int(n_miss[j]), int(G.shape[1] - n_miss[j]), t[5], t[6], float(maf[j])) for j, t in enumerate(text)]


def close_to_print(got, want):
    """|got - want| <= 1e-6 |want| + 1e-12 elementwise, NaN where NaN"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got[~nan] - want[~nan]) <= PRINT_RTOL * np.abs(want[~nan]) + PRINT_ATOL))


def compare_file(path, tag):
    """a written .cor.txt against golden `tag`: text fields identical, numeric fields at the print resolution"""
    want = golden(tag)
    with open(path) as f:
        lines = f.read().splitlines()
    assert lines[0].split("\t") == ["chr", "rs", "ps", "n_mis", "n_obs", "allele1", "allele0", "af", "window_size", "var", "cor"]
    assert len(lines) - 1 == len(want), (len(lines) - 1, len(want))
    for line, w in zip(lines[1:], want):
        t = line.split("\t")
        assert t[:8] == w["text"], (t[:8], w["text"])
        assert int(t[8]) == w["window"], (t[:3], t[8], w["window"])
        assert close_to_print([float(t[9])], [w["var"]]), (t[:3], t[9], w["var"])
        cor = np.array([]) if t[10] == "NA" else np.array([float(v) for v in t[10].split(",")])
        assert (t[10] == "NA") == (w["window"] == 0)
        assert close_to_print(cor, w["cor"]), (t[:3], cor, w["cor"])

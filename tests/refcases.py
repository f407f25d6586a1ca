"""Shared by test_reference_pin.py (CPU: oracle vs reference) and test_gpu_reference.py / test_gpu_vc.py (GPU: HIP path vs
reference): loads tests/golden/ref_*.npz -- outputs of the reference itself (oracle/_ref/gemma, see
tests/golden/make_ref_fixtures.py) -- and the input decoding both need, and records / replays in-process calls of the
reference (Calls, tests/golden/ref_calls/).  Nothing here computes a statistic."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

# .assoc.txt column -> SUMSTAT field (src/lmm.cpp:101-225)
COLS = {"beta": "beta", "se": "se", "logl_H1": "logl_H1", "l_remle": "lambda_remle", "l_mle": "lambda_mle",
        "p_wald": "p_wald", "p_lrt": "p_lrt", "p_score": "p_score"}
# the reference prints 7 significant digits ("%.6e"): half a unit of the last digit is 5e-7 relative
PRINT_TOL = 1.5e-6


def load(name):
    d = np.load(os.path.join(GOLD, name))
    return {k: d[k] for k in d.files}


def rel_err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    e[np.isnan(got) & np.isnan(ref)] = 0.0
    return e


def assert_stats(got, fx, tag, tol=PRINT_TOL, lam_tol=None, lam_frac=1.0):
    """Every column the reference printed for run `tag` against SUMSTAT records `got`."""
    seen = 0
    for col, field in COLS.items():
        key = "%s_%s" % (tag, col)
        if key not in fx:
            continue
        seen += 1
        e = rel_err(got[field], fx[key])
        if col in ("l_remle", "l_mle") and lam_tol is not None:
            assert np.mean(e <= tol) >= lam_frac, (tag, col, float(np.mean(e <= tol)))
            assert np.nanmax(e) <= lam_tol, (tag, col, float(np.nanmax(e)))
        else:
            assert np.nanmax(e) <= tol, (tag, col, float(np.nanmax(e)), int(np.nanargmax(e)))
    assert seen >= 1, tag


def issue188_inputs(fx):
    """bed rows (p x ceil(n/4) uint8), n_total, phenotype vector (-9 where missing) and its indicator."""
    n_total = int(fx["n_total"])
    nb = (n_total + 3) // 4
    raw = np.ascontiguousarray(fx["bed"][3:].reshape(-1, nb))
    ph = fx["pheno_col6"]
    indp = np.array([0 if s in ("-9", "NA") else 1 for s in ph], dtype=np.int32)
    y_all = np.array([(-9.0 if s in ("-9", "NA") else float(s)) for s in ph])
    return raw, n_total, y_all, indp


def mv_case_inputs(fx, f188, tag):
    """(bed rows, n_total, Y_all (n_total x d), indicator over all traits, indicator of trait 1 -- what the `-gk` run,
    which reads phenotype column 1 only, filtered its SNPs with)."""
    if tag == "a":
        Y = fx["a_pheno"]
        n_total = Y.shape[0]
        bed = fx["a_bed"]
        ind = np.ones(n_total, dtype=np.int32)
        ind1 = ind
    elif tag == "c":
        Y = fx["c_pheno"]
        n_total = Y.shape[0]
        bed = f188["bed"]
        ind = np.ones(n_total, dtype=np.int32)
        ind1 = ind
    else:
        txt = fx["b_pheno_txt"]
        n_total = txt.shape[0]
        bed = f188["bed"]
        ind = np.array([0 if "NA" in row else 1 for row in txt], dtype=np.int32)
        ind1 = np.array([0 if row[0] == "NA" else 1 for row in txt], dtype=np.int32)
        Y = np.array([[(-9.0 if x == "NA" else float(x)) for x in row] for row in txt])
    nb = (n_total + 3) // 4
    return np.ascontiguousarray(bed[3:].reshape(-1, nb)), n_total, Y, ind, ind1


def mv_ref_table(fx, tag, mode, d):
    """The reference's mvLMM columns for one run as a dict shaped like MVLMM.sumStat."""
    pre = "%s_m%d_" % (tag, mode)
    out = {"beta": np.column_stack([fx[pre + "beta_%d" % (i + 1)] for i in range(d)]),
           "Vbeta": np.column_stack([fx[pre + "Vbeta_%d_%d" % (i + 1, j + 1)] for i in range(d) for j in range(i, d)])}
    for c in ("p_wald", "p_lrt", "p_score"):
        if pre + c in fx:
            out[c] = fx[pre + c]
    return out


def mv_row_err(got, ref):
    """Per-SNP worst relative error over the printed fields, each field scaled by its largest entry in that row."""
    l = ref["beta"].shape[0]
    worst = np.zeros(l)
    for k, r in ref.items():
        g = np.asarray(got[k]).reshape(l, -1)
        r = np.asarray(r).reshape(l, -1)
        scale = np.maximum(np.abs(r).max(axis=1, keepdims=True), 1e-300)
        worst = np.maximum(worst, (np.abs(g - r) / scale).max(axis=1))
    return worst


def dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


CALLS = os.path.join(GOLD, "ref_calls")


class Calls:
    """The in-process calls of the reference one test makes: live through oracle/_ref/libgemma_ref.so (so) or the oracle's
    bridges (orc), or, with so = None, replayed from tests/golden/ref_calls/<name>.npz after checking that each call gets
    the inputs the recorded one had.  GEMMA_REF_RECORD=1 with a live library rewrites the recording (save())."""

    def __init__(self, name, so, orc):
        self.path = os.path.join(CALLS, name.replace("[", "_").replace("]", "") + ".npz")
        self.so, self.orc, self.i, self.rec = so, orc, 0, {}
        self.live = so is not None
        self.record = self.live and os.environ.get("GEMMA_REF_RECORD") == "1"
        if not self.live:
            d = np.load(self.path)
            self.rec = {k: d[k] for k in d.files}

    def ref(self, name, *args):
        """so.<name>(*args) (ctypes; numpy arrays go in as double *)"""
        fn = (lambda *a: getattr(self.so, name)(*[dp(x) if isinstance(x, np.ndarray) else x for x in a])) if self.live else None
        return self._call(fn, args, {})

    def oracle(self, name, *args, **kw):
        """oracle.<name>(*args, **kw): the in-process bridges to the reference (ref_lmm_analyze, ref_plink_kin, ...)"""
        return self._call(getattr(self.orc, name) if self.live else None, args, kw)

    def _call(self, fn, args, kw):
        k = "c%d_" % self.i
        self.i += 1
        arrs = [(j, a) for j, a in enumerate(args) if isinstance(a, np.ndarray)]
        fp = [v for _, a in arrs for v in (float(np.nansum(a)), float(np.nansum(np.abs(a))))]
        fp += [float(a) for a in list(args) + list(kw.values()) if isinstance(a, (int, float, np.floating, np.integer))]
        fp = np.array(fp, dtype=np.float64)
        if not self.live:
            want = self.rec[k + "fp"]
            assert want.shape == fp.shape and np.all(np.abs(fp - want) <= 1e-9 * np.abs(want) + 1e-300), (self.path, k, fp, want)
            for j, a in arrs:
                if k + "a%d" % j in self.rec:
                    np.copyto(a, self.rec[k + "a%d" % j])
            if k + "r" in self.rec:
                return self.rec[k + "r"][()] if self.rec[k + "r"].ndim == 0 else self.rec[k + "r"]
            return tuple(self.rec[k + "r%d" % t][()] if self.rec[k + "r%d" % t].ndim == 0 else self.rec[k + "r%d" % t]
                         for t in range(int(self.rec[k + "nr"])))
        before = [a.copy() for _, a in arrs]
        ret = fn(*args, **kw)
        if self.record:
            self.rec[k + "fp"] = fp
            for (j, a), b in zip(arrs, before):
                if not np.array_equal(a, b, equal_nan=True):
                    self.rec[k + "a%d" % j] = a.copy()
            if isinstance(ret, tuple):
                self.rec[k + "nr"] = np.array(len(ret))
                for t, r in enumerate(ret):
                    self.rec[k + "r%d" % t] = np.asarray(r)
            else:
                self.rec[k + "r"] = np.asarray(ret)
        return ret

    def save(self):
        if self.record:
            os.makedirs(CALLS, exist_ok=True)
            np.savez_compressed(self.path, **self.rec)

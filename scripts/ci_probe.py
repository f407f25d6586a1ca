"""The two genotype passes of the MQS confidence intervals (-ci 1 / -ci 2) at size on one MI355X: pass 1 (Xz and XWz) and pass 2
(XtXWz) on a PLINK 2-bit block of --snps SNPs x --n individuals with 1 % missing calls, for n_vc = 1 and 8 and for w given and
NULL, each timed with HIP events after warm-up (median of --reps), beside two yardsticks taken in the same process:

* the time to read the block once at the achievable HBM rate DESIGN.md uses (6.3 TB/s);
* the single-vector kernels called once per column, which is what a caller could do before these entry points existed:
  gemma_hip_prdt_add_d (X~ w) 2 n_vc times for pass 1, gemma_hip_ridge_batch_d (X_c' r) n_vc times for pass 2.

    python scripts/ci_probe.py [--n 20000] [--snps 20000] [--reps 7]

Every pair is measured in three alternating runs (new, loop, new, loop, ...).  Prints one JSON line; `ok` (and the exit status) is
the condition of DESIGN.md section 15: at n_vc = 8 each new pass is faster than its per-column loop by more than the spread of
the three runs."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import _lib as L  # noqa: E402
from gemma_amd import api  # noqa: E402
from prdt_probe import median_ms, packed_block  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    api.init(0)
    import torch
    lib = L.lib()
    n, l = a.n, a.snps
    rng = np.random.default_rng(1)
    rows = packed_block(rng, l, n)
    ld = rows.shape[1]
    ind = np.ones(n, dtype=np.int32)
    dev = torch.from_numpy(rows).cuda()
    gp = C.c_void_p(dev.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    z = torch.from_numpy(rng.standard_normal(l)).cuda()
    w = torch.from_numpy(rng.uniform(0.5, 20.0, l)).cuda()
    out = {"n": n, "snps": l, "block_bytes": int(rows.nbytes), "reps": a.reps, "hbm_floor_ms_at_6.3TBps": rows.nbytes / 6.3e9, "cases": []}
    # the per-column loops: X~ w wants the individuals as its "test" group (indicator 0), X_c' r as its analysed group (indicator 1)
    ind0 = np.zeros(n, dtype=np.int32)
    used = torch.empty(l, dtype=torch.int32, device="cuda")
    alpha = torch.empty(l, dtype=torch.float64, device="cuda")
    skipped = C.c_size_t(0)
    ok = True
    for n_vc in (1, 8):
        cat = torch.from_numpy(rng.integers(0, n_vc, l).astype(np.int32)).cuda()
        for weighted in (False, True):
            wp = C.c_void_p(w.data_ptr()) if weighted else None
            res = {"n_vc": n_vc, "w": weighted}

            def new1():
                L.check(lib.gemma_hip_ci_xwz_d(L.GENO_PLINK_2BIT, gp, l, ld, C.c_void_p(cat.data_ptr()), C.c_void_p(z.data_ptr()), wp,
                                               C.byref(skipped), st), "ci_xwz_d")

            def loop1():
                for _ in range(2 * n_vc):
                    L.check(lib.gemma_hip_prdt_add_d(L.GENO_PLINK_2BIT, gp, l, ld, C.c_void_p(z.data_ptr()), C.c_void_p(used.data_ptr()), st),
                            "prdt_add_d")

            xt = torch.empty((l, n_vc), dtype=torch.float64, device="cuda")

            def new2():
                L.check(lib.gemma_hip_ci_xtxwz_d(L.GENO_PLINK_2BIT, gp, l, ld, C.c_void_p(xt.data_ptr()), st), "ci_xtxwz_d")

            def loop2():
                for _ in range(n_vc):
                    L.check(lib.gemma_hip_ridge_batch_d(L.GENO_PLINK_2BIT, gp, l, ld, C.c_void_p(alpha.data_ptr()), st), "ridge_batch_d")

            t_new1, t_loop1, t_new2, t_loop2 = [], [], [], []
            for _ in range(3):  # alternating runs
                L.check(lib.gemma_hip_ci_begin(n, ind.ctypes.data, n_vc), "ci_begin")
                t_new1.append(median_ms(new1, a.reps)[0])
                L.check(lib.gemma_hip_prdt_begin(ind0.ctypes.data, n), "prdt_begin")
                t_loop1.append(median_ms(loop1, a.reps, warm=1)[0])
                y = np.zeros(n)
                L.check(lib.gemma_hip_prdt_end(0.0, 0, y.ctypes.data), "prdt_end")
                L.check(lib.gemma_hip_ci_xwz_end(None, None), "ci_xwz_end")
                t_new2.append(median_ms(new2, a.reps)[0])
                api.ridge_set_r(np.ones(n), 1.0)
                api.ridge_set_indicator(ind)
                t_loop2.append(median_ms(loop2, a.reps, warm=1)[0])
                api.ridge_finish()
            for name, tn, tl in (("pass1", t_new1, t_loop1), ("pass2", t_new2, t_loop2)):
                spread = max(max(tn) - min(tn), max(tl) - min(tl))
                res[name] = {"new_ms": tn, "loop_ms": tl, "spread_ms": spread, "of_hbm_floor": float(np.median(tn)) / out["hbm_floor_ms_at_6.3TBps"],
                             "faster": bool(max(tn) + spread < min(tl))}
                if n_vc == 8:
                    ok = ok and res[name]["faster"]
            out["cases"].append(res)
    lib.gemma_hip_ci_release()
    out["ok"] = ok
    print(json.dumps(out))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

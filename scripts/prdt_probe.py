"""The two genotype matrix-vector passes of genomic prediction at size on one MI355X: X_c' r (ridge effects, -bslmm 2) and X~ w
(-predict) on a PLINK 2-bit block of --snps SNPs x --n individuals with 1 % missing calls, each timed with HIP events after
warm-up (median of --reps), beside the host-to-device copy of the same block in the same run (pinned and pageable) and beside
the block's bytes over the measured device copy bandwidth as the HBM floor.

    python scripts/prdt_probe.py [--n 20000] [--snps 20000] [--reps 15] [--check] [--cpu-n 4000]

Each pass is timed twice: repeated on one block, which then sits in the 256 MB Infinity Cache (`xtr_ms`, `xw_ms`), and on four
copies of the block in turn, 400 MB, so that every call reads from HBM (`*_cold_ms`; the fractions of the copy and of the HBM
floor are of these).  Prints one JSON line (after the parity line of --check).  `ok` (and the exit status) is the condition of
DESIGN.md: each pass, in either timing, takes no longer than the block's own (pinned) host-to-device copy, so a pass over a file
is bound by feeding the device, as the association loop's ingest is -- and, with --check, both parity ratios are at most 1.
--check adds `parity`: the largest error over the derived dot-product bound of both passes against numpy on the block's first
512 SNPs.  --cpu-n > 0 adds
the CPU leg at a size where the reference's dense UtX fits in memory: numpy's U'X_c (the dgemm of CalcUtX) followed by the dgemv
of BSLMM::RidgeR, beside the device's X_c' (U b) on the same block."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import _lib as L  # noqa: E402
from gemma_amd import api  # noqa: E402

EPS = np.finfo(np.float64).eps


def packed_block(rng, l, n, miss=0.01):
    """random .bed rows: code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing"""
    rows = np.zeros((l, (n + 3) // 4), dtype=np.uint8)
    for k in range(4):
        m = len(range(k, n, 4))
        g = rng.choice(np.array([3, 2, 0, 1], dtype=np.uint8), size=(l, m), p=[0.49 * (1 - miss), 0.42 * (1 - miss), 0.09 * (1 - miss), miss])
        rows[:, :m] |= g << (2 * k)
    return rows


def unpack(rows, n):
    code = np.stack([(rows >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(rows.shape[0], -1)[:, :n]
    return np.array([2.0, np.nan, 1.0, 0.0])[code]


def median_ms(fn, reps, warm=3):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--cpu-n", type=int, default=0)
    a = ap.parse_args()
    api.init(0)
    import torch
    lib = L.lib()
    n, l = a.n, a.snps
    rng = np.random.default_rng(1)
    rows = packed_block(rng, l, n)
    ind = np.ones(n, dtype=np.int32)
    ind[rng.choice(n, n // 3, replace=False)] = 0
    n_train = int(ind.sum())
    r, w = rng.standard_normal(n_train), rng.standard_normal(l)
    out = {"n": n, "snps": l, "block_bytes": int(rows.nbytes), "reps": a.reps}

    # the copies of the same block: host -> device (pinned, pageable) and device -> device (the HBM floor)
    pinned = torch.from_numpy(rows).pin_memory()
    pageable = torch.from_numpy(rows)
    dev = torch.empty(rows.shape, dtype=torch.uint8, device="cuda")
    dev2 = torch.empty_like(dev)
    out["h2d_pinned_ms"], _ = median_ms(lambda: dev.copy_(pinned, non_blocking=True), a.reps)
    out["h2d_pageable_ms"], _ = median_ms(lambda: dev.copy_(pageable), a.reps, warm=1)
    d2d, _ = median_ms(lambda: dev2.copy_(dev), a.reps)
    out["d2d_copy_ms"] = d2d
    out["copy_GBps"] = 2 * rows.nbytes / d2d / 1e6  # a copy reads and writes the block
    out["hbm_floor_ms"] = rows.nbytes / (out["copy_GBps"] * 1e6)
    out["hbm_floor_ms_at_6.29TBps"] = rows.nbytes / 6.29e9

    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    alpha = torch.empty(l, dtype=torch.float64, device="cuda")
    api.ridge_set_r(r, 1.0)
    api.ridge_set_indicator(ind)
    xtr = lambda: L.check(lib.gemma_hip_ridge_batch_d(L.GENO_PLINK_2BIT, C.c_void_p(dev.data_ptr()), l, rows.shape[1],
                                                      C.c_void_p(alpha.data_ptr()), st), "ridge_batch_d")
    out["xtr_ms"], out["xtr_min_ms"] = median_ms(xtr, a.reps)
    got_alpha = alpha.cpu().numpy()
    # the same pass on four copies of the block in turn (400 MB against 256 MB of Infinity Cache): every call meets a block the
    # calls before it have pushed out, where the repeated call above re-reads one that is resident
    ring = [dev] + [dev.clone() for _ in range(3)]
    turn = [0]

    def xtr_cold():
        turn[0] += 1
        L.check(lib.gemma_hip_ridge_batch_d(L.GENO_PLINK_2BIT, C.c_void_p(ring[turn[0] % 4].data_ptr()), l, rows.shape[1],
                                            C.c_void_p(alpha.data_ptr()), st), "ridge_batch_d")
    out["xtr_cold_ms"], _ = median_ms(xtr_cold, a.reps, warm=4)
    api.ridge_finish()

    wd = torch.from_numpy(w).cuda()
    used = torch.empty(l, dtype=torch.int32, device="cuda")
    L.check(lib.gemma_hip_prdt_begin(ind.ctypes.data, n), "prdt_begin")
    xw = lambda: L.check(lib.gemma_hip_prdt_add_d(L.GENO_PLINK_2BIT, C.c_void_p(dev.data_ptr()), l, rows.shape[1],
                                                  C.c_void_p(wd.data_ptr()), C.c_void_p(used.data_ptr()), st), "prdt_add_d")
    out["xw_ms"], out["xw_min_ms"] = median_ms(xw, a.reps)

    def xw_cold():
        turn[0] += 1
        L.check(lib.gemma_hip_prdt_add_d(L.GENO_PLINK_2BIT, C.c_void_p(ring[turn[0] % 4].data_ptr()), l, rows.shape[1],
                                         C.c_void_p(wd.data_ptr()), C.c_void_p(used.data_ptr()), st), "prdt_add_d")
    out["xw_cold_ms"], _ = median_ms(xw_cold, a.reps, warm=4)
    y = np.zeros(n - n_train)  # the sum over the warm-up and the timed calls: not looked at
    L.check(lib.gemma_hip_prdt_end(0.0, 0, y.ctypes.data), "prdt_end")
    for k in ("xtr", "xw"):
        out[k + "_of_h2d_pinned"] = out[k + "_cold_ms"] / out["h2d_pinned_ms"]
        out[k + "_hbm_fraction"] = out["hbm_floor_ms"] / out[k + "_cold_ms"]  # of the floor's bandwidth: floor time over pass time
        out[k + "_GBps"] = rows.nbytes / out[k + "_cold_ms"] / 1e6
    # the condition, on the slower of the two timings of each pass
    out["ok"] = bool(max(out["xtr_ms"], out["xtr_cold_ms"], out["xw_ms"], out["xw_cold_ms"]) <= out["h2d_pinned_ms"])

    if a.check:
        m = min(512, l)
        G = unpack(rows[:m], n)
        Ga = G[:, ind == 1]
        miss = np.isnan(Ga)
        mean = np.where(miss, 0.0, Ga).sum(1) / (~miss).sum(1)
        Xc = np.where(miss, 0.0, Ga - mean[:, None])
        ref = Xc @ r
        bound = 4 * n_train * EPS * (np.abs(Xc) @ np.abs(r))
        par = {"xtr_max_err_over_bound": float(np.max(np.abs(got_alpha[:m] - ref) / bound)), "snps_checked": m}
        # X~ w on the same rows alone, one call
        Gp = G[:, ind == 0]
        xm = np.where(np.isnan(Gp), 0.0, Gp).sum(1) / (~np.isnan(Gp)).sum(1)
        X = np.where(np.isnan(Gp), (xm - mean)[:, None], Gp - mean[:, None])
        yref = (X * w[:m, None]).sum(0)
        ybound = 4 * m * EPS * (np.abs(X) * np.abs(w[:m, None])).sum(0)
        L.check(lib.gemma_hip_prdt_begin(ind.ctypes.data, n), "prdt_begin")
        L.check(lib.gemma_hip_prdt_add_d(L.GENO_PLINK_2BIT, C.c_void_p(dev.data_ptr()), m, rows.shape[1], C.c_void_p(wd.data_ptr()),
                                         C.c_void_p(used.data_ptr()), st), "prdt_add_d")
        y1 = np.zeros(n - n_train)
        L.check(lib.gemma_hip_prdt_end(0.0, 0, y1.ctypes.data), "prdt_end")
        par["xw_max_err_over_bound"] = float(np.max(np.abs(y1 - yref) / ybound))
        out["parity"] = par
        out["ok"] = bool(out["ok"] and par["xtr_max_err_over_bound"] <= 1.0 and par["xw_max_err_over_bound"] <= 1.0)
        print("parity[prdt n=%d 2-bit block, %d SNPs vs numpy] X_c' r: max err / bound %.3e (bound 4 n eps sum|xc||r|); "
              "X~ w: max err / bound %.3e (bound 4 l eps sum|x~||w|)" % (n, m, par["xtr_max_err_over_bound"], par["xw_max_err_over_bound"]))

    if a.cpu_n > 0:
        nc = lc = a.cpu_n
        rows_c = packed_block(rng, lc, nc)
        Gc = unpack(rows_c, nc)
        miss = np.isnan(Gc)
        Xc = np.where(miss, 0.0, Gc - (np.where(miss, 0.0, Gc).sum(1) / (~miss).sum(1))[:, None])  # lc x nc
        U = np.linalg.qr(rng.standard_normal((nc, nc)))[0]
        b = rng.standard_normal(nc)
        t = time.perf_counter()
        UtX = U.T @ Xc.T          # CalcUtX(U, UtX), src/gemma.cpp:2951
        ref = UtX.T @ b           # the dgemv of BSLMM::RidgeR
        cpu_s = time.perf_counter() - t
        api.ridge_set_r(U @ b, 1.0)
        t = time.perf_counter()
        got = api.ridge_batch(rows_c, L.GENO_PLINK_2BIT)  # host block: upload + both kernels + download
        dev_s = time.perf_counter() - t
        api.ridge_finish()
        out["cpu_leg"] = {"n": nc, "snps": lc, "utx_bytes": int(UtX.nbytes), "cpu_utx_dgemv_s": cpu_s, "device_host_block_s": dev_s,
                          "max_abs_diff_over_max": float(np.max(np.abs(got - ref)) / np.max(np.abs(ref))),
                          "threads": os.cpu_count() if not os.environ.get("OMP_NUM_THREADS") else int(os.environ["OMP_NUM_THREADS"])}
    print(json.dumps(out))
    sys.exit(0 if out["ok"] else 1)


if __name__ == "__main__":
    main()

"""T univariate LMMs over one U^T x at size on one MI355X: ms per block of the multi-phenotype scan (LMM.batch_multi) for
T = 1, 8, 32 with the shared fixed-lambda table on and off (GEMMA_HIP_MULTI_TABLE), beside the single-phenotype block (LMM.batch).

    python scripts/multi_probe.py [--n 20000] [--snps 20000] [--T 1 8 32] [--blocks 5] [--warm 2] [--repeats 3]
    python scripts/multi_probe.py --single      # LMM.batch alone: only the interface that existed before the multi scan

n individuals, PLINK 2-bit blocks of --snps SNPs with 1 % missing calls, c = 1, -lmm 1; --blocks timed blocks after --warm
warm-up blocks, each block between two HIP events on the stream, everything device-resident (the _d entry points).  The
--single leg is repeated --repeats times (fresh setup each): its spread is the bar for "T = 1 costs what a single block costs".
Prints one JSON line per leg and a summary line with the per-phenotype increment (ms(T = 32) - ms(T = 1)) / 31."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import _lib as L  # noqa: E402
from gemma_amd import api  # noqa: E402


def packed_block(rng, l, n, miss=0.01):
    """random .bed rows: code 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing"""
    rows = np.zeros((l, (n + 3) // 4), dtype=np.uint8)
    for k in range(4):
        m = len(range(k, n, 4))
        g = rng.choice(np.array([3, 2, 0, 1], dtype=np.uint8), size=(l, m), p=[0.49 * (1 - miss), 0.42 * (1 - miss), 0.09 * (1 - miss), miss])
        rows[:, :m] |= g << (2 * k)
    return rows


def timed_blocks(fn, blocks, warm):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(blocks):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=20000)
    ap.add_argument("--T", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--single", action="store_true")
    a = ap.parse_args()
    api.init(0)
    import torch
    n, l, Tmax = a.n, a.snps, max(a.T)
    rng = np.random.default_rng(5)
    gen = torch.Generator(device="cuda").manual_seed(5)
    U = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, device="cuda", generator=gen))[0].contiguous()
    ev = torch.sort(torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 2.0)[0].contiguous()
    ev[0] = 0.0
    # traits of different heritability: y_t = sqrt(h_t) U sqrt(ev) z + sqrt(1 - h_t) e
    h = torch.linspace(0.05, 0.9, Tmax, dtype=torch.float64, device="cuda")
    z = torch.randn((n, Tmax), dtype=torch.float64, device="cuda", generator=gen)
    e = torch.randn((n, Tmax), dtype=torch.float64, device="cuda", generator=gen)
    UtY = (torch.sqrt(h) * torch.sqrt(ev)[:, None] * z + torch.sqrt(1 - h) * (U.T @ e)).contiguous()
    UtW = (U.T @ torch.ones((n, 1), dtype=torch.float64, device="cuda")).contiguous()
    dev = torch.from_numpy(packed_block(rng, l, n)).cuda()
    torch.cuda.synchronize()
    base = {"n": n, "snps": l, "blocks": a.blocks, "warm": a.warm}

    singles = []
    for rep in range(a.repeats):
        lmm = api.LMM(a_mode=1)
        lmm.setup(U, ev, UtW, UtY[:, 0].contiguous(), plink=True)
        out = torch.empty((l, 8), dtype=torch.float64, device="cuda")
        ts = timed_blocks(lambda: lmm.batch(dev, L.GENO_PLINK_2BIT, out=out), a.blocks, a.warm)
        lmm.finish()
        singles.append(float(np.median(ts)))
        print(json.dumps(dict(base, leg="single", rep=rep, ms_per_block=singles[-1], ms_min=float(np.min(ts)), ms_max=float(np.max(ts)))), flush=True)
    if a.single:
        return
    res = {}
    for table in ("1", "0"):
        os.environ["GEMMA_HIP_MULTI_TABLE"] = table
        api.reload_env()
        for T in a.T:
            lmm = api.LMM(a_mode=1)
            lmm.setup_multi(U, ev, UtW, UtY[:, :T].contiguous(), plink=True)
            out = torch.empty((T, l, 8), dtype=torch.float64, device="cuda")
            ts = timed_blocks(lambda: lmm.batch_multi(dev, L.GENO_PLINK_2BIT, out=out), a.blocks, a.warm)
            lmm.finish()
            res[(table, T)] = float(np.median(ts))
            print(json.dumps(dict(base, leg="multi", T=T, shared_table=int(table), ms_per_block=res[(table, T)], ms_min=float(np.min(ts)),
                                  ms_max=float(np.max(ts)), ms_per_phenotype=res[(table, T)] / T,
                                  baseline_T_singles_ms=T * float(np.median(singles)))), flush=True)
    os.environ.pop("GEMMA_HIP_MULTI_TABLE", None)
    api.reload_env()
    summ = dict(base, leg="summary", single_ms=float(np.median(singles)), single_spread_ms=float(np.max(singles) - np.min(singles)))
    lo, hi = min(a.T), max(a.T)
    if hi > lo:
        for table in ("1", "0"):
            summ["increment_ms_per_phenotype_table%s" % table] = (res[(table, hi)] - res[(table, lo)]) / (hi - lo)
    print(json.dumps(summ), flush=True)


if __name__ == "__main__":
    main()

"""The score panel at size on one MI355X: ms per block of LMM.batch_score_panel (ingest + U^T x + the product kernel) and of the
product kernel alone (LMM.assoc_score_panel on a resident U^T x) for T = 64, 1024, 4096 phenotypes, beside the multi-phenotype scan
in mode 3 (LMM.batch_multi: the per-SNP kernel once per phenotype) at T = 64.

    python scripts/score_panel_probe.py [--n 20000] [--snps 20000] [--T 64 1024 4096] [--multi-T 64] [--blocks 3] [--warm 1]

n individuals, PLINK 2-bit blocks of --snps SNPs with 1 % missing calls, c = 1, -lmm 3, null lambdas spread over 1e-5 ... 1e5;
--blocks timed blocks after --warm warm-ups, each between two HIP events on the stream, everything device-resident.  Prints one
JSON line per leg and a summary with the per-phenotype increment of the product between the smallest and the largest T, next to the
flop-count figure 2 l n (c + 2) / (fp64 MFMA peak) per phenotype.  A probe, not a test: no threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import _lib as L  # noqa: E402
from gemma_amd import api  # noqa: E402
from multi_probe import packed_block, timed_blocks  # noqa: E402

PEAK_F64_MFMA = 78.6e12  # flop/s, MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=20000)
    ap.add_argument("--T", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--multi-T", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    a = ap.parse_args()
    api.init(0)
    import torch
    n, l, Tmax = a.n, a.snps, max(a.T + [a.multi_T])
    rng = np.random.default_rng(5)
    gen = torch.Generator(device="cuda").manual_seed(5)
    U = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, device="cuda", generator=gen))[0].contiguous()
    ev = torch.sort(torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 2.0)[0].contiguous()
    ev[0] = 0.0
    h = torch.linspace(0.05, 0.9, Tmax, dtype=torch.float64, device="cuda")
    UtY = torch.empty((n, Tmax), dtype=torch.float64, device="cuda")
    for t0 in range(0, Tmax, 512):  # in slices: U^T e of 4096 traits at once is a 6 GB temporary too many
        t1 = min(Tmax, t0 + 512)
        z = torch.randn((n, t1 - t0), dtype=torch.float64, device="cuda", generator=gen)
        e = torch.randn((n, t1 - t0), dtype=torch.float64, device="cuda", generator=gen)
        UtY[:, t0:t1] = torch.sqrt(h[t0:t1]) * torch.sqrt(ev)[:, None] * z + torch.sqrt(1 - h[t0:t1]) * (U.T @ e)
    UtW = (U.T @ torch.ones((n, 1), dtype=torch.float64, device="cuda")).contiguous()
    lams = 10.0 ** rng.uniform(-5.0, 5.0, size=Tmax)
    dev = torch.from_numpy(packed_block(rng, l, n)).cuda()
    torch.cuda.synchronize()
    base = {"n": n, "snps": l, "c": 1, "blocks": a.blocks, "warm": a.warm}
    flop_ms = 2.0 * l * n * 3 / PEAK_F64_MFMA * 1e3  # per phenotype

    res = {}
    for T in a.T:
        lmm = api.LMM(a_mode=3)
        Yt = UtY[:, :T].contiguous()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lmm.setup_score_panel(U, ev, UtW, Yt, lams[:T])
        torch.cuda.synchronize()
        setup_ms = (time.perf_counter() - t0) * 1e3
        out = torch.empty((T, l, 3), dtype=torch.float64, device="cuda")
        ts = timed_blocks(lambda: lmm.batch_score_panel(dev, L.GENO_PLINK_2BIT, out=out), a.blocks, a.warm)
        finite = float(torch.isfinite(out).double().mean())
        UtX = torch.randn((l, n), dtype=torch.float64, device="cuda", generator=gen)
        tp = timed_blocks(lambda: lmm.assoc_score_panel(UtX, out=out), a.blocks, a.warm)
        lmm.finish()
        del out, UtX, Yt
        res[T] = (float(np.median(ts)), float(np.median(tp)))
        print(json.dumps(dict(base, leg="score_panel", T=T, setup_ms=setup_ms, ms_per_block=res[T][0], ms_min=float(np.min(ts)),
                              ms_max=float(np.max(ts)), product_ms=res[T][1], product_ms_min=float(np.min(tp)),
                              product_ms_per_phenotype=res[T][1] / T, flop_count_ms_per_phenotype=flop_ms,
                              product_tflops=2.0 * l * n * 3 * T / (res[T][1] * 1e-3) / 1e12, finite_fraction=finite)), flush=True)

    T = a.multi_T
    lmm = api.LMM(a_mode=3)
    lmm.setup_multi(U, ev, UtW, UtY[:, :T].contiguous(), lams[:T], np.zeros(T))
    out = torch.empty((T, l, 8), dtype=torch.float64, device="cuda")
    ts = timed_blocks(lambda: lmm.batch_multi(dev, L.GENO_PLINK_2BIT, out=out), a.blocks, a.warm)
    lmm.finish()
    one = api.LMM(a_mode=3, l_mle_null=float(lams[0]))
    one.setup(U, ev, UtW, UtY[:, 0].contiguous())
    out1 = torch.empty((l, 8), dtype=torch.float64, device="cuda")
    t1 = timed_blocks(lambda: one.batch(dev, L.GENO_PLINK_2BIT, out=out1), a.blocks, a.warm)
    one.finish()
    multi_ms, single_ms = float(np.median(ts)), float(np.median(t1))
    print(json.dumps(dict(base, leg="multi_mode3", T=T, ms_per_block=multi_ms, ms_min=float(np.min(ts)), ms_max=float(np.max(ts)),
                          single_mode3_ms=single_ms, increment_ms_per_phenotype=(multi_ms - single_ms) / (T - 1))), flush=True)
    lo, hi = min(a.T), max(a.T)
    summ = dict(base, leg="summary", flop_count_ms_per_phenotype=flop_ms, multi_mode3_increment_ms_per_phenotype=(multi_ms - single_ms) / (T - 1))
    if hi > lo:
        summ["block_increment_ms_per_phenotype"] = (res[hi][0] - res[lo][0]) / (hi - lo)
        summ["product_increment_ms_per_phenotype"] = (res[hi][1] - res[lo][1]) / (hi - lo)
    if a.multi_T in res:
        summ["score_panel_ms_per_phenotype_at_multi_T"] = (res[a.multi_T][0] - single_ms) / a.multi_T
    print(json.dumps(summ), flush=True)


if __name__ == "__main__":
    main()

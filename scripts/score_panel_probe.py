"""The score panel at size on one MI355X: ms per block of LMM.batch_score_panel (ingest + U^T x + the product kernel) and of the
product kernel alone (LMM.assoc_score_panel on a resident U^T x) for T = 64, 1024, 4096 phenotypes, beside the multi-phenotype scan
in mode 3 (LMM.batch_multi: the per-SNP kernel once per phenotype) at T = 64; and, per T and --p-max, the hits form of the same
block and product (gemma_hip_lmm_score_panel_hits_batch_d / _hits_assoc_d into a resident list, with `best`), its hit count, and
both forms once more with their result copied to the host (the records: T x l x 24 bytes; the hits: count, list and best).

    python scripts/score_panel_probe.py [--n 20000] [--snps 20000] [--T 64 1024 4096] [--p-max 1e-5 0.05] [--multi-T 64]
                                        [--blocks 3] [--warm 1]

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


def host_timed(fn, blocks, warm):
    """wall-clock ms of `blocks` calls after `warm` warm-ups, the device idle before and after each"""
    import torch
    out = []
    for k in range(warm + blocks):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def hits_leg(lmm, base, T, l, p_max, dev, UtX, a, rec_ms):
    """the hits form of the block and of the product alone at one p_max, then the block with its result copied to the host"""
    import ctypes as C
    import torch
    lib = L.lib()
    cap = int(2 * p_max * T * l) + 4096
    raw = torch.empty((cap, 4), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    best = torch.empty((T, 4), dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def block():
        L.check(lib.gemma_hip_lmm_score_panel_hits_batch_d(L.GENO_PLINK_2BIT, ptr(dev), l, dev.stride(0), p_max, ptr(raw), cap, ptr(cnt),
                                                           ptr(best), st), "hits_batch_d")

    def product():
        L.check(lib.gemma_hip_lmm_score_panel_hits_assoc_d(ptr(UtX), l, UtX.stride(0), p_max, ptr(raw), cap, ptr(cnt), ptr(best), st),
                "hits_assoc_d")

    def to_host():
        block()
        k = min(int(cnt.item()), cap)
        return raw[:k].cpu(), best.cpu()
    ts = timed_blocks(block, a.blocks, a.warm)
    n_block = int(cnt.item())
    tp = timed_blocks(product, a.blocks, a.warm)
    n_prod = int(cnt.item())
    th = host_timed(to_host, a.blocks, a.warm)
    print(json.dumps(dict(base, leg="score_panel_hits", T=T, p_max=p_max, cap=cap, ms_per_block=float(np.median(ts)),
                          ms_min=float(np.min(ts)), ms_max=float(np.max(ts)), product_ms=float(np.median(tp)),
                          product_ms_min=float(np.min(tp)), product_ms_max=float(np.max(tp)), records_ms_per_block=rec_ms[0],
                          records_product_ms=rec_ms[1], hits_per_block=n_block, hits_product=n_prod,
                          to_host_ms_per_block=float(np.median(th)), d2h_bytes=8 + 32 * min(n_block, cap) + 32 * T)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=20000)
    ap.add_argument("--T", type=int, nargs="+", default=[64, 1024, 4096])
    ap.add_argument("--p-max", type=float, nargs="*", default=[1e-5, 0.05])
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
        res[T] = (float(np.median(ts)), float(np.median(tp)))
        lmm.finish()
        del out
        if a.p_max:
            # The hits legs need calibrated statistics: under nulls spread over ten decades most pairs of a trait whose lambda is
            # far off have a p_score of 0 and every p_max keeps a fifth of the block.  The traits were drawn with variance
            # (1 - h)(lambda delta + 1), lambda = h / (1 - h): with those nulls p_score is uniform on a random U^T x.  The records
            # form is timed again under the same setup, beside the hits form and with its copy to the host (wall clock).
            lmm.setup_score_panel(U, ev, UtW, Yt, (h[:T] / (1 - h[:T])).cpu().numpy())
            out = torch.empty((T, l, 3), dtype=torch.float64, device="cuda")
            rs = timed_blocks(lambda: lmm.batch_score_panel(dev, L.GENO_PLINK_2BIT, out=out), a.blocks, a.warm)
            rp = timed_blocks(lambda: lmm.assoc_score_panel(UtX, out=out), a.blocks, a.warm)
            th = host_timed(lambda: lmm.batch_score_panel(dev, L.GENO_PLINK_2BIT, out=out).cpu(), a.blocks, a.warm)
            rec = (float(np.median(rs)), float(np.median(rp)))
            print(json.dumps(dict(base, leg="score_panel_true_nulls", T=T, ms_per_block=rec[0], ms_min=float(np.min(rs)),
                                  ms_max=float(np.max(rs)), product_ms=rec[1], product_ms_min=float(np.min(rp)),
                                  product_ms_max=float(np.max(rp)), to_host_ms_per_block=float(np.median(th)),
                                  d2h_bytes=T * l * 24)), flush=True)
            del out
            for p_max in a.p_max:
                hits_leg(lmm, base, T, l, p_max, dev, UtX, a, rec)
            lmm.finish()
        del UtX, Yt
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

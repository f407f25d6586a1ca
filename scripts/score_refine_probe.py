"""The refinement of the score panel's hits at size on one MI355X: Wald and LRT of the pairs a block's screen returns, as one
launch over the list (gemma_hip_lmm_score_panel_refine_last_d) against what the library offered before -- one single-phenotype
setup per distinct phenotype among the hits.

    python scripts/score_refine_probe.py [--n 20000] [--snps 20000] [--T 1024 4096] [--p-max 1e-5] [--runs 5] [--warm 1]

The panel of scripts/score_panel_probe.py: n individuals, one PLINK 2-bit block of --snps SNPs with 1 % missing calls, c = 1, traits
of heritability 0.05 ... 0.9 with their true null lambdas h / (1 - h) in the score-panel setup (calibrated p_score: the hits are
p_max T l of the pairs); logl_mle_H0 of the refinement from gemma_hip_lmm_null_panel_d.  Per T, wall clock around each leg with
the device idle before and after, the median and range of --runs runs after --warm warm-ups, one process:
    (a) hits_batch_d alone (the block: ingest, U^T x, the product with the hits epilogue),
    (b) hits_batch_d followed by refine_last_d on its list,
    (c) for each distinct phenotype among the hits: gemma_hip_lmm_setup_d (a_mode 4) + gemma_hip_lmm_assoc_d on the gathered hit
        rows of that phenotype + gemma_hip_lmm_finish -- the parent commit's way to the same records,
and beside them the product alone (hits_assoc_d on the block's U^T x: the score_panel_kernel time of DESIGN.md section 17) and the
refinement alone (refine_assoc_d on the same U^T x, between two events).  The records of (b) and (c) are compared: legs (c) run
with the tables on, so they agree to the tables' accuracy, not in bits.  Prints two JSON lines per T (legs a, b and the kernels
alone; then leg c).  A probe, not a test: no threshold."""
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
from multi_probe import packed_block, timed_blocks  # noqa: E402
from score_panel_probe import host_timed  # noqa: E402


def stats(ts):
    return dict(median=float(np.median(ts)), min=float(np.min(ts)), max=float(np.max(ts)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--snps", type=int, default=20000)
    ap.add_argument("--T", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--p-max", type=float, default=1e-5)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    a = ap.parse_args()
    api.init(0)
    import torch
    lib = L.lib()
    n, l, Tmax, p_max = a.n, a.snps, max(a.T), a.p_max
    rng = np.random.default_rng(5)
    gen = torch.Generator(device="cuda").manual_seed(5)
    U = torch.linalg.qr(torch.randn((n, n), dtype=torch.float64, device="cuda", generator=gen))[0].contiguous()
    ev = torch.sort(torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 2.0)[0].contiguous()
    ev[0] = 0.0
    h = torch.linspace(0.05, 0.9, Tmax, dtype=torch.float64, device="cuda")
    UtY = torch.empty((n, Tmax), dtype=torch.float64, device="cuda")
    for t0 in range(0, Tmax, 512):
        t1 = min(Tmax, t0 + 512)
        z = torch.randn((n, t1 - t0), dtype=torch.float64, device="cuda", generator=gen)
        e = torch.randn((n, t1 - t0), dtype=torch.float64, device="cuda", generator=gen)
        UtY[:, t0:t1] = torch.sqrt(h[t0:t1]) * torch.sqrt(ev)[:, None] * z + torch.sqrt(1 - h[t0:t1]) * (U.T @ e)
    UtW = (U.T @ torch.ones((n, 1), dtype=torch.float64, device="cuda")).contiguous()
    host_block = packed_block(rng, l, n)
    dev = torch.from_numpy(host_block).cuda()
    torch.cuda.synchronize()
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    for T in a.T:
        Yt = UtY[:, :T].contiguous()
        lam = (h[:T] / (1 - h[:T])).cpu().numpy()
        fit = api.CalcLambdaNullPanel(ev, UtW, Yt)  # (T, 8) device tensor: l_mle_null, logl_mle_H0, ...
        logl = fit[:, 1].cpu().numpy()
        lmm = api.LMM(a_mode=3)
        lmm.setup_score_panel(U, ev, UtW, Yt, lam)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lmm.setup_score_refine(Yt, logl)
        refine_setup_ms = (time.perf_counter() - t0) * 1e3
        cap = int(2 * p_max * T * l) + 4096
        raw = torch.zeros((cap, 4), dtype=torch.int64, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        best = torch.empty((T, 4), dtype=torch.int64, device="cuda")
        out = torch.empty((cap, 8), dtype=torch.float64, device="cuda")

        def block():
            L.check(lib.gemma_hip_lmm_score_panel_hits_batch_d(L.GENO_PLINK_2BIT, ptr(dev), l, dev.stride(0), p_max, ptr(raw), cap, ptr(cnt),
                                                               ptr(best), st), "hits_batch_d")

        def block_refine():
            block()
            m = min(int(cnt.item()), cap)  # the list's length has to reach the host: one 8-byte copy
            L.check(lib.gemma_hip_lmm_score_panel_refine_last_d(ptr(raw), m, ptr(out), st), "refine_last_d")

        leg_a = host_timed(block, a.runs, a.warm)
        leg_b = host_timed(block_refine, a.runs, a.warm)
        m = min(int(cnt.item()), cap)
        key = raw[:m, 0]
        order = torch.argsort(key)  # by (pheno, snp): pheno sits in the high half
        pairs = raw[:m][order].contiguous()
        snp, pheno = (pairs[:, 0] & 0xffffffff), (pairs[:, 0] >> 32) & 0xffffffff
        # the block's own U^T x, for the product alone, the refinement alone and leg (c)
        UtX = torch.from_numpy(lmm.dbg_utx(host_block, L.GENO_PLINK_2BIT, 1)).cuda()
        product = timed_blocks(lambda: L.check(lib.gemma_hip_lmm_score_panel_hits_assoc_d(
            ptr(UtX), l, UtX.stride(0), p_max, ptr(raw), cap, ptr(cnt), ptr(best), st), "hits_assoc_d"), a.runs, a.warm)
        refined = torch.empty((m, 8), dtype=torch.float64, device="cuda")
        alone = timed_blocks(lambda: L.check(lib.gemma_hip_lmm_score_panel_refine_assoc_d(
            ptr(UtX), l, UtX.stride(0), ptr(pairs), m, ptr(refined), st), "refine_assoc_d"), a.runs, a.warm)
        torch.cuda.synchronize()
        lmm.finish()
        a_med, b_med = float(np.median(leg_a)), float(np.median(leg_b))
        base = dict(n=n, snps=l, c=1, T=T, p_max=p_max, runs=a.runs, warm=a.warm, hits=m)
        print(json.dumps(dict(base, leg="panel", refine_setup_ms=refine_setup_ms, a_hits_batch_ms=stats(leg_a),
                              b_hits_batch_refine_last_ms=stats(leg_b), refinement_b_minus_a_ms=b_med - a_med, refine_alone_ms=stats(alone),
                              product_alone_ms=stats(product))), flush=True)

        phs, starts = torch.unique_consecutive(pheno, return_counts=True)
        phs, counts = phs.cpu().numpy(), starts.cpu().numpy()
        offs = np.concatenate([[0], np.cumsum(counts)])
        loop_out = torch.empty((m, 8), dtype=torch.float64, device="cuda")

        def loop():
            for k, t in enumerate(phs):
                rows = UtX[snp[offs[k]:offs[k + 1]]].contiguous()
                one = api.LMM(a_mode=4, l_mle_null=float(lam[t]), logl_mle_H0=float(logl[t]))
                one.setup(U, ev, UtW, Yt[:, t].contiguous())
                one.assoc(rows, out=loop_out[offs[k]:offs[k + 1]])
                torch.cuda.synchronize()
                one.finish()

        leg_c = host_timed(loop, a.runs, a.warm) if m else [0.0]
        with np.errstate(invalid="ignore", divide="ignore"):
            r, q = refined.cpu().numpy(), loop_out.cpu().numpy()
            rel = np.abs(r - q) / np.abs(q)
        worst = {k: float(np.nanmax(rel[:, j])) if m else 0.0 for j, k in
                 enumerate(("beta", "se", "lambda_remle", "lambda_mle", "p_wald", "p_lrt", "p_score", "logl_H1"))}
        print(json.dumps(dict(base, leg="setup_loop", distinct_phenotypes=int(len(phs)), c_setup_loop_ms=stats(leg_c),
                              refinement_b_minus_a_ms=b_med - a_med, refinement_below_min_of_c=bool(b_med - a_med < float(np.min(leg_c))),
                              nan_records=int(np.isnan(r).any(axis=1).sum()) if m else 0, worst_rel_b_vs_c=worst)), flush=True)
        del UtX, Yt, raw, out, refined, loop_out


if __name__ == "__main__":
    main()

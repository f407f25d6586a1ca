"""Times one block of the windowed SNP correlation (-calccor) on one GPU -- not part of any test:

    python scripts/cor_probe.py [--n 20000] [--l 20000] [--windowns 500] [--reps 3]

One gemma_hip_cor_block_d of `l` output SNPs with `windowns` neighbours each (l + windowns rows with the halo) over n individuals,
on three inputs made on the device:
* hard calls (2-bit rows) with 1 % missing calls: every tile pair runs the four int8 products;
* the same hard calls without a missing call: every tile pair runs P1 alone;
* the second input as fp64 rows: the fp64 MFMA panels and the scatter kernel.
Prints one JSON line: ms per block (best of `reps` after one warm-up), int8 TOP/s over the tile pairs the band kernel ran
(products x 2 x 64 x 64 x n per pair, ingest included in the time), and the ratio of the fp64 time to each integer time
(DESIGN.md section 14 carries the numbers of the default sizes)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--l", type=int, default=20000)
    ap.add_argument("--windowns", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    import torch
    from gemma_amd import api, _lib as L
    api.init(0)
    lib = L.lib()
    n, l, w = a.n, a.l, a.windowns
    l_in = l + w
    ld = (n + 3) // 4
    gen = torch.Generator(device="cuda").manual_seed(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # genotypes 0 / 1 / 2 by allele frequency; 2-bit codes: 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing
    f = torch.rand(l_in, 1, device="cuda", generator=gen) * 0.4 + 0.1
    g = (torch.rand(l_in, 4 * ld, device="cuda", generator=gen) < f).to(torch.uint8)
    g += (torch.rand(l_in, 4 * ld, device="cuda", generator=gen) < f).to(torch.uint8)
    code = torch.where(g == 2, 0, torch.where(g == 1, 2, 3)).to(torch.uint8)

    def pack(c):
        c = c.view(l_in, ld, 4)
        return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).contiguous()

    rows_full = pack(code)
    code_m = code.clone()
    code_m[torch.rand(l_in, 4 * ld, device="cuda", generator=gen) < 0.01] = 1
    rows_miss = pack(code_m)
    del code, code_m, f
    ind = np.ones(n, dtype=np.int32)
    L.check(lib.gemma_hip_cor_begin(n, C.c_void_p(ind.ctypes.data)), "begin")
    nb = torch.full((l,), w, dtype=torch.int32, device="cuda")
    var = torch.empty(l, dtype=torch.float64, device="cuda")
    cor = torch.empty(l * w, dtype=torch.float64, device="cuda")

    def timed(kind, rows, ldr):
        best = None
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.check(lib.gemma_hip_cor_block_d(kind, C.c_void_p(rows.data_ptr()), l_in, ldr, l, C.c_void_p(nb.data_ptr()),
                                              C.c_void_p(var.data_ptr()), C.c_void_p(cor.data_ptr()), stream), "block")
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if r > 0:
                best = dt if best is None else min(best, dt)
        return best * 1e3, float(cor[:: max(1, cor.numel() // 1000)].nan_to_num().abs().sum())

    ms_miss, chk_miss = timed(L.GENO_PLINK_2BIT, rows_miss, ld)
    ms_full, chk_full = timed(L.GENO_PLINK_2BIT, rows_full, ld)
    del rows_miss, rows_full
    X = g[:, :n].to(torch.float64).contiguous()
    del g
    ms_f64, chk_f64 = timed(L.GENO_F64_SNP_MAJOR, X, n)
    api.VARCOV.Release()
    pairs = sum(min((ti * 64 + 63 + w), l_in - 1) // 64 - ti + 1 for ti in range((l + 63) // 64))
    ops = 2.0 * 64 * 64 * n * pairs
    print(json.dumps(dict(n=n, l_out=l, window_ns=w, tile_pairs=pairs, ms_hard_1pct_missing=round(ms_miss, 2),
                          ms_hard_complete=round(ms_full, 2), ms_fp64=round(ms_f64, 2),
                          int8_tops_1pct_missing=round(4 * ops / ms_miss / 1e9, 1), int8_tops_complete=round(ops / ms_full / 1e9, 1),
                          fp64_over_int8_1pct_missing=round(ms_f64 / ms_miss, 2), fp64_over_int8_complete=round(ms_f64 / ms_full, 2),
                          complete_over_1pct=round(ms_full / ms_miss, 2), checksum=[chk_miss, chk_full, chk_f64])))


if __name__ == "__main__":
    main()

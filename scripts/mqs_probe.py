"""Times the two stages of the MQS path (-gs / -vc 1 -beta) on one GPU -- not part of any test:

    python scripts/mqs_probe.py [--n 20000] [--p 100000] [--nvc 4] [--batch 20000]

* kinship pass: gemma_hip_mqs_add_d over p random hard-call SNPs (2-bit rows made on the device, 1 % missing) in blocks of
  `batch`: ingest + residual + compaction + one fp64 SYRK per category and block;
* S stage: gemma_hip_mqs_end: mirror + centre + scale of the n_vc matrices, the row pass, the n_vc (n_vc + 1) / 2 pair passes
  and the host finishing step of the jackknife.
Prints one JSON line (DESIGN.md section 13 carries the numbers of the default sizes)."""
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
    ap.add_argument("--p", type=int, default=100000)
    ap.add_argument("--nvc", type=int, default=4)
    ap.add_argument("--batch", type=int, default=20000)
    a = ap.parse_args()
    import torch
    from gemma_amd import api, _lib as L
    api.init(0)
    lib = L.lib()
    n, p, nvc = a.n, a.p, a.nvc
    ind = np.ones(n, dtype=np.int32)
    W = np.ones((n, 1))
    gen = torch.Generator(device="cuda").manual_seed(1)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ld = (n + 3) // 4
    L.check(lib.gemma_hip_mqs_begin(n, C.c_void_p(ind.ctypes.data), nvc, C.c_void_p(W.ctypes.data), 1, 0), "begin")
    t_kin = 0.0
    for s0 in range(0, p, a.batch):
        l = min(a.batch, p - s0)
        # 2-bit codes: 0 -> 2, 2 -> 1, 3 -> 0, 1 -> missing
        f = torch.rand(l, 1, device="cuda", generator=gen) * 0.4 + 0.1
        u = torch.rand(l, 4 * ld, device="cuda", generator=gen)
        g = (u < f).to(torch.uint8) + (torch.rand(l, 4 * ld, device="cuda", generator=gen) < f).to(torch.uint8)
        code = torch.where(g == 2, 0, torch.where(g == 1, 2, 3)).to(torch.uint8)
        code[torch.rand(l, 4 * ld, device="cuda", generator=gen) < 0.01] = 1
        code = code.view(l, ld, 4)
        rows = (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).contiguous()
        cat = torch.randint(0, nvc, (l,), device="cuda", generator=gen, dtype=torch.int32)
        del f, u, g, code
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        L.check(lib.gemma_hip_mqs_add_d(L.GENO_PLINK_2BIT, C.c_void_p(rows.data_ptr()), l, ld, C.c_void_p(cat.data_ptr()), None, stream),
                "add")
        torch.cuda.synchronize()
        t_kin += time.perf_counter() - t0
        del rows, cat
    S = np.zeros((2 * nvc, nvc))
    ns = np.zeros(nvc)
    t0 = time.perf_counter()
    L.check(lib.gemma_hip_mqs_end(C.c_void_p(S.ctypes.data), C.c_void_p(ns.ctypes.data)), "end")
    t_S = time.perf_counter() - t0
    api.MQS.Release()
    flops = 2.0 * n * n / 2 * ns.sum()  # the upper triangle of the SYRKs
    print(json.dumps(dict(n=n, p=p, n_vc=nvc, batch=a.batch, kinship_s=round(t_kin, 3), S_stage_s=round(t_S, 3),
                          syrk_tflops=round(flops / t_kin / 1e12, 2), ns=ns.tolist(), S00=S[0, 0], Svar00=S[nvc, 0])))


if __name__ == "__main__":
    main()

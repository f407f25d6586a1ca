"""-vc 1 / -vc 2 at size on one MI355X: the HE time, the REML time per evaluation split into assembly, SPD inverse, P correction,
mat-vecs and traces, the evaluation count, and the SPD inverse's rate (n^3 flop / time) against the 78.6 TFLOP/s fp64 peak.

    python scripts/vc_probe.py [--n 20000] [--nvc 3] [--spd 8192,20000]

Kinships come from disjoint random SNP sets (api.CalcKin + api.CenterMatrix); the phenotype has pve 0.5 spread over them."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import api  # noqa: E402

PEAK = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--nvc", type=int, default=3)
    ap.add_argument("--snps", type=int, default=2000)
    ap.add_argument("--spd", default="8192,20000,50000")
    a = ap.parse_args()
    api.init(0)
    import torch
    out = {"spd": []}
    for n in [int(v) for v in a.spd.split(",") if v]:
        g = torch.Generator(device="cuda").manual_seed(n)
        X = torch.randn(n, 512, device="cuda", dtype=torch.float64, generator=g)
        A = X @ X.T / 512 + torch.eye(n, device="cuda", dtype=torch.float64)
        B = A.clone()
        api.spd_inverse(B)  # warm-up (workspace, code objects)
        torch.cuda.synchronize()
        B.copy_(A)
        torch.cuda.synchronize()
        t = time.perf_counter()
        api.spd_inverse(B)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t
        out["spd"].append({"n": n, "s": dt, "tflops_n3": n ** 3 / dt / 1e12, "of_peak": n ** 3 / dt / PEAK})
        del A, B, X
        torch.cuda.empty_cache()
    n, rng = a.n, np.random.default_rng(1)
    Ks, y = [], np.zeros(n)
    for l in range(a.nvc):
        G = rng.integers(0, 3, size=(a.snps, n)).astype(np.float64)
        K = api.CalcKin(G, 0, n, 1)
        Ks.append(api.CenterMatrix(K))
        y += (G - G.mean(1, keepdims=True)).T @ rng.standard_normal(a.snps) * np.sqrt(0.5 / a.nvc / a.snps)
    y += rng.standard_normal(n) * np.sqrt(0.5)
    W = np.ones((n, 1))
    Kd = [torch.from_numpy(K).cuda() for K in Ks]
    t = time.perf_counter()
    h = api.VC().CalcVChe(Kd, W, y)
    out["he_s"] = time.perf_counter() - t
    t = time.perf_counter()
    r = api.VC().CalcVCreml(Kd, W, y)
    out["reml_s"] = time.perf_counter() - t
    out.update(n=n, nvc=a.nvc, he_sigma2=list(h.v_sigma2), reml_sigma2=list(r.v_sigma2), iterations=r.iterations, status=r.status,
               evaluations=r.evaluations, inverses=r.inverses,
               per_eval_s={k: v / max(r.evaluations, 1) for k, v in r.timing.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()

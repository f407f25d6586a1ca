"""The trait-pair panel at size on one MI355X: ms per pair of gemma_hip_mvlmm_null_pairs (device form, inputs resident; host form,
uploads included) for T = 32 (496 pairs) and T = 128 (8128 pairs), with one and with four wavefronts (= pairs) per workgroup
(GEMMA_HIP_MVPAIR_WAVES), beside the loop of gemma_hip_mvlmm_null(d = 2) over the same pairs in the same process -- the way
available before the panel: per pair two univariate fits, uploads, one launch of one wavefront and a synchronisation.

    python scripts/pair_panel_probe.py [--n 20000] [--T 32 128] [--loop-pairs 496] [--reps 2] [--warm 1] [--em-iter 500]
                                       [--out profiles/pair_panel_probe_mi355x.jsonl]

n individuals, c = 1 (the intercept), synthetic eigenvalues; the traits share one genetic and one residual factor with loadings
spread over -0.8 ... 0.8 and heritabilities over 0.1 ... 0.8, so the pairs differ in their correlations and in their EM trip counts.
--em-iter caps MphEM (PARAM's default is 10000) for both sides alike so that a slowly converging pair cannot stretch the loop over
the probe's time.  Every timing is wall clock around the call with the device idle before and after.  Appends ONE JSON line to
--out and prints it.  A probe, not a test: the only condition is the one a defect would break -- the panel is not slower than the
loop on the same pairs -- and the fields both report are compared as bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import _lib as L  # noqa: E402
from gemma_amd import api  # noqa: E402


def timed(fn, reps, warm):
    import torch
    out = []
    for k in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--T", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--loop-pairs", type=int, default=496, help="pairs of the smallest T the loop of single fits runs over")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--em-iter", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    api.init(0)
    import torch
    n, Tmax = a.n, max(a.T)
    gen = torch.Generator(device="cuda").manual_seed(11)
    ev = torch.sort(torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 2.0)[0].contiguous()
    ev[0] = 0.0
    w = torch.randn((n, 1), dtype=torch.float64, device="cuda", generator=gen)
    UtW = (w * (n ** 0.5 / torch.linalg.norm(w))).contiguous()  # U^T 1: a vector of norm sqrt(n)
    perm = torch.randperm(Tmax, device="cuda", generator=gen)
    h = torch.linspace(0.1, 0.8, Tmax, dtype=torch.float64, device="cuda")[perm]
    lg = torch.linspace(-0.8, 0.8, Tmax, dtype=torch.float64, device="cuda")[torch.randperm(Tmax, device="cuda", generator=gen)]
    le = torch.linspace(-0.8, 0.8, Tmax, dtype=torch.float64, device="cuda")[torch.randperm(Tmax, device="cuda", generator=gen)]
    fg, fe = (torch.randn((n, 1), dtype=torch.float64, device="cuda", generator=gen) for _ in range(2))
    zg = lg * fg + torch.sqrt(1 - lg * lg) * torch.randn((n, Tmax), dtype=torch.float64, device="cuda", generator=gen)
    ze = le * fe + torch.sqrt(1 - le * le) * torch.randn((n, Tmax), dtype=torch.float64, device="cuda", generator=gen)
    UtY = (torch.sqrt(h * ev[:, None]) * zg + torch.sqrt(1.0 - h) * ze + 0.3 * UtW).contiguous()
    torch.cuda.synchronize()
    opt = L.MvOpt(a.em_iter, 100, 1e-4, 1e-4, 1e-3, 0, 0)
    res = {"probe": "pair_panel", "n": n, "c": 1, "em_iter": a.em_iter, "reps": a.reps, "warm": a.warm, "device": api.device_info()[0],
           "cus": api.device_info()[1]}
    ev_h, UtW_h = ev.cpu().numpy(), UtW.cpu().numpy()
    for T in a.T:
        Yd = UtY[:, :T].contiguous()
        m = T * (T - 1) // 2
        leg = {"pairs": m}
        for waves in (4, 1):
            os.environ["GEMMA_HIP_MVPAIR_WAVES"] = str(waves)  # read at the call
            td = timed(lambda: api.CalcMvNullPairs(ev, UtW, Yd, opt=opt), a.reps, a.warm)
            leg["panel_d_ms_waves%d" % waves] = float(np.median(td))
            leg["panel_d_ms_waves%d_min" % waves] = float(np.min(td))
            leg["panel_d_ms_per_pair_waves%d" % waves] = float(np.median(td)) / m
        os.environ.pop("GEMMA_HIP_MVPAIR_WAVES")
        fit = api.CalcMvNullPairs(ev, UtW, Yd, opt=opt).cpu().numpy().view(api.MVPAIR_DTYPE).reshape(-1)
        leg["status_ok"] = float((fit["status"] == 0).mean())
        leg["rg_min_max"] = [float(np.nanmin(fit["remle"]["rg"])), float(np.nanmax(fit["remle"]["rg"]))]
        res["T%d" % T] = leg
    T = min(a.T)
    Yh = UtY[:, :T].cpu().numpy()
    pairs = [(i, j) for i in range(T) for j in range(i + 1, T)][:a.loop_pairs]
    lst = np.array(pairs, dtype=np.int32)
    th = timed(lambda: api.CalcMvNullPairs(ev_h, UtW_h, Yh, pairs=lst, opt=opt), a.reps, a.warm)
    panel = api.CalcMvNullPairs(ev_h, UtW_h, Yh, pairs=lst, opt=opt)
    cols = [np.ascontiguousarray(Yh[:, [i, j]]) for i, j in pairs]
    mv = api.MVLMM(em_iter=a.em_iter)

    def loop():
        return [dict(mv.fit_null(ev_h, UtW_h, y)) for y in cols]
    tl = timed(loop, 1, 0)  # the loop is the slow side: one pass
    single = loop()
    iu = np.triu_indices(2)
    same = all(np.array_equal(panel[q][tag][k], single[q][k + "_" + tag][iu]) for q in range(len(pairs)) for tag in ("remle", "mle")
               for k in ("Vg", "Ve")) and all(panel[q][tag]["logl"] == single[q]["logl_" + tag] for q in range(len(pairs))
                                              for tag in ("remle", "mle"))
    res["loop"] = {"T": T, "pairs": len(pairs), "loop_ms": float(np.median(tl)), "loop_ms_per_pair": float(np.median(tl)) / len(pairs),
                   "panel_host_ms": float(np.median(th)), "panel_host_ms_per_pair": float(np.median(th)) / len(pairs),
                   "bits_equal_panel": bool(same)}
    res["panel_not_slower_than_loop"] = bool(np.median(th) <= np.median(tl))
    res["ratio_loop_over_panel_host"] = float(np.median(tl) / np.median(th))
    line = json.dumps(res)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()

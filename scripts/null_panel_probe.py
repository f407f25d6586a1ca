"""The whole-panel null fit at size on one MI355X: ms of gemma_hip_lmm_null_panel for T = 64, 1024, 16384 phenotypes, device form
(inputs resident) and host form (uploads and chunks included), beside the loop of T = 64 single fits (gemma_hip_lmm_null, one call
per column: five allocations, three uploads, one 64-lane workgroup and a synchronisation each) on the same columns in the same
process.

    python scripts/null_panel_probe.py [--n 20000] [--T 64 1024 16384] [--loop-T 64] [--reps 3] [--warm 1] [--beta] [--beta-c 16]
                                       [--parent-lib path/to/the/parent/commit's/libgemma_hip.so]

--parent-lib: the same loop once more on a library built from the parent commit (the single fit's kernels take the phenotype as an
argument since the panel exists), in a fresh process per library -- parent, this build, parent, this build -- through the C ABI
alone; reports both loop times and whether the parent's fits are the bytes of this build's.

n individuals, c = 1 (the intercept), synthetic eigenvalues and U^T Y with heritabilities spread over 0.02 ... 0.95, so that the fits
end at l_min, inside and near l_max and polish one to three brackets.  Every timing is wall clock around the call with the device
idle before and after.  Prints ONE JSON line.  A probe, not a test: the only condition is the one a defect would break -- at
T = loop-T the panel is not slower than the loop -- and the fits of the two are compared as bytes."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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


def loop_child(lib_path, in_path, out_path, reps, warm):
    """the loop of single fits through the C ABI of the library at lib_path: times (ms) and the fits -> out_path"""
    import torch  # noqa: F401  (one HIP runtime per process)
    lib = C.CDLL(lib_path)
    sz, dp, cd = C.c_size_t, C.c_void_p, C.c_double
    lib.gemma_hip_init.argtypes = [C.c_int, C.c_int]
    lib.gemma_hip_lmm_null.argtypes = [sz, sz, dp, dp, dp, cd, cd, sz, cd, dp]
    assert lib.gemma_hip_init(0, 0) == 0
    z = np.load(in_path)
    ev, W, Y, tr = z["ev"], np.ascontiguousarray(z["UtW"]), z["UtY"], float(z["tr"])
    cols = [np.ascontiguousarray(Y[:, t]) for t in range(Y.shape[1])]
    out = np.zeros((len(cols), 8))
    ms = []
    for k in range(warm + reps):
        t0 = time.perf_counter()
        for t, y in enumerate(cols):  # the call synchronises: its result is on the host when it returns
            rc = lib.gemma_hip_lmm_null(len(ev), W.shape[1], ev.ctypes.data, W.ctypes.data, y.ctypes.data, 1e-5, 1e5, 10, tr,
                                        out[t].ctypes.data)
            assert rc == 0, rc
        if k >= warm:
            ms.append((time.perf_counter() - t0) * 1e3)
    np.savez(out_path, ms=np.array(ms), fit=out)


def parent_leg(parent_lib, ev_h, UtW_h, Yh, tr, reps, warm):
    from gemma_amd import _lib as L
    res = {}
    with tempfile.TemporaryDirectory() as td:
        np.savez(os.path.join(td, "in.npz"), ev=ev_h, UtW=UtW_h, UtY=Yh, tr=tr)
        runs = {"parent": [], "this": []}
        fits = {}
        for rnd in range(2):
            for who, path in (("parent", parent_lib), ("this", L.LIB_PATH)):
                out = os.path.join(td, "%s%d.npz" % (who, rnd))
                subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-child", path, os.path.join(td, "in.npz"), out,
                                str(reps), str(warm)], check=True, timeout=600)
                z = np.load(out)
                runs[who] += z["ms"].tolist()
                fits[who] = z["fit"]
        for who in runs:
            res["loop_ms_" + who] = float(np.median(runs[who]))
            res["loop_ms_%s_min" % who] = float(np.min(runs[who]))
            res["loop_ms_%s_max" % who] = float(np.max(runs[who]))
        res["single_fit_bits_equal_parent"] = bool(fits["parent"].tobytes() == fits["this"].tobytes())
    return res


def main():
    if len(sys.argv) == 7 and sys.argv[1] == "--loop-child":
        return loop_child(sys.argv[2], sys.argv[3], sys.argv[4], int(sys.argv[5]), int(sys.argv[6]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--T", type=int, nargs="+", default=[64, 1024, 16384])
    ap.add_argument("--loop-T", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--beta", action="store_true", help="also time the panel with the covariate effects")
    ap.add_argument("--beta-c", type=int, default=0, help="also time fits and covariate effects with this many covariates at T = 1024")
    ap.add_argument("--parent-lib", default=None, help="libgemma_hip.so of the parent commit: the loop on it, in processes of their own")
    a = ap.parse_args()
    api.init(0)
    import torch
    n, Tmax = a.n, max(a.T + [a.loop_T])
    gen = torch.Generator(device="cuda").manual_seed(9)
    ev = torch.sort(torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) * 2.0)[0].contiguous()
    ev[0] = 0.0
    w = torch.randn((n, 1), dtype=torch.float64, device="cuda", generator=gen)
    UtW = (w * (n ** 0.5 / torch.linalg.norm(w))).contiguous()  # U^T 1: a vector of norm sqrt(n)
    h = torch.linspace(0.02, 0.95, Tmax, dtype=torch.float64, device="cuda")[torch.randperm(Tmax, device="cuda", generator=gen)]
    UtY = torch.empty((n, Tmax), dtype=torch.float64, device="cuda")
    for t0 in range(0, Tmax, 2048):
        t1 = min(Tmax, t0 + 2048)
        z = torch.randn((n, t1 - t0), dtype=torch.float64, device="cuda", generator=gen)
        UtY[:, t0:t1] = torch.sqrt(h[t0:t1] * ev[:, None] + (1.0 - h[t0:t1])) * z + 0.3 * UtW
    torch.cuda.synchronize()
    tr = float(ev.mean())
    res = {"probe": "null_panel", "n": n, "c": 1, "reps": a.reps, "warm": a.warm, "device": api.device_info()[0], "cus": api.device_info()[1]}
    ev_h, UtW_h = ev.cpu().numpy(), UtW.cpu().numpy()
    for T in a.T:
        Yd = UtY[:, :T].contiguous()
        td = timed(lambda: api.CalcLambdaNullPanel(ev, UtW, Yd, trace_G=tr), a.reps, a.warm)
        fit = api.CalcLambdaNullPanel(ev, UtW, Yd, trace_G=tr)
        lam = fit[:, 0]
        leg = {"panel_d_ms": float(np.median(td)), "panel_d_ms_min": float(np.min(td)), "panel_d_ms_max": float(np.max(td)),
               "panel_d_us_per_phenotype": float(np.median(td)) * 1e3 / T,
               "ml_at_l_min": int((lam <= 1e-5).sum()), "ml_at_l_max": int((lam >= 1e5).sum()), "finite": float(torch.isfinite(fit).double().mean())}
        if a.beta:
            tb = timed(lambda: api.CalcLambdaNullPanel(ev, UtW, Yd, trace_G=tr, want_beta=True), a.reps, a.warm)
            leg["panel_d_beta_ms"] = float(np.median(tb))
        if T <= 1024:  # the host form moves U^T Y across PCIe: 2.6 GB at T = 16384 would time the link
            Yh = Yd.cpu().numpy()
            th = timed(lambda: api.CalcLambdaNullPanel(ev_h, UtW_h, Yh, trace_G=tr), a.reps, a.warm)
            leg["panel_host_ms"] = float(np.median(th))
            leg["panel_host_ms_min"] = float(np.min(th))
        res["T%d" % T] = leg
        del Yd
    T = a.loop_T
    Yh = UtY[:, :T].cpu().numpy()
    cols = [np.ascontiguousarray(Yh[:, t]) for t in range(T)]

    def loop():
        return [api.CalcLambdaNull(ev_h, UtW_h, cols[t], trace_G=tr) for t in range(T)]
    tl = timed(loop, a.reps, a.warm)
    single = np.array([[f[k] for k in api.NULL_DTYPE.names] for f in loop()])
    panel = api.CalcLambdaNullPanel(ev_h, UtW_h, Yh, trace_G=tr)
    same = single.tobytes() == np.ascontiguousarray(panel).tobytes()
    res["loop"] = {"T": T, "loop_ms": float(np.median(tl)), "loop_ms_min": float(np.min(tl)), "loop_ms_max": float(np.max(tl)),
                   "loop_us_per_phenotype": float(np.median(tl)) * 1e3 / T, "bits_equal_panel": bool(same)}
    if a.beta_c:
        c, Tb = a.beta_c, min(1024, Tmax)
        Wc = torch.randn((n, c), dtype=torch.float64, device="cuda", generator=gen)
        Wc[:, c - 1] = UtW[:, 0]
        Yb = UtY[:, :Tb].contiguous()
        t_fit = timed(lambda: api.CalcLambdaNullPanel(ev, Wc, Yb, trace_G=tr), a.reps, a.warm)
        t_beta = timed(lambda: api.CalcLambdaNullPanel(ev, Wc, Yb, trace_G=tr, want_beta=True), a.reps, a.warm)
        res["beta_c%d_T%d" % (c, Tb)] = {"panel_d_ms": float(np.median(t_fit)), "panel_d_beta_ms": float(np.median(t_beta)),
                                       "beta_ms": float(np.median(t_beta) - np.median(t_fit))}
    if a.parent_lib:
        res["parent"] = parent_leg(a.parent_lib, ev_h, UtW_h, Yh, tr, a.reps, a.warm)
    key = "T%d" % T
    if key in res:
        res["panel_not_slower_than_loop"] = bool(res[key].get("panel_host_ms", res[key]["panel_d_ms"]) <= res["loop"]["loop_ms"])
    big = "T%d" % max(a.T)
    res["rate_ratio_loop_over_largest_panel"] = res["loop"]["loop_us_per_phenotype"] / res[big]["panel_d_us_per_phenotype"]
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

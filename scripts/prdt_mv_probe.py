"""The solve of the Kronecker system of the multi-phenotype kinship-only prediction at size on one MI355X: Cholesky factor + two
triangular solves (what gemma_hip_prdt_kin_mv_apply runs on H_oo) beside the yardstick it replaces, gemma_hip_spd_inverse_d of the
same matrix followed by a matrix-vector product.  The matrix is symmetric and diagonally dominant, made on the device.

    python scripts/prdt_mv_probe.py [--n 8192] [--reps 3]

Prints one JSON line: seconds of both paths (HIP events, median of --reps after one warm-up), their ratio, the flop ratio
(n^3 / 3) / (4 n^3 / 3) = 0.25 it is held against, and the largest difference of the two solutions over max |z|."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemma_amd import _lib as L  # noqa: E402
from gemma_amd import api  # noqa: E402


def timed(fn, prepare, reps):
    import torch
    ts = []
    for k in range(reps + 1):
        prepare()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if k:
            ts.append(a.elapsed_time(b) / 1e3)
    return float(np.median(ts))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    api.init(0)
    lib = L.lib()
    lib.gemma_hip_dbg_spd_solve_d.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_long), C.c_void_p]
    n = a.n
    g = torch.Generator(device="cuda").manual_seed(5)
    A0 = torch.rand((n, n), dtype=torch.float64, device="cuda", generator=g)
    A0 = torch.triu(A0) + torch.triu(A0, 1).T
    A0 += n * torch.eye(n, dtype=torch.float64, device="cuda")
    r = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    A, x = torch.empty_like(A0), torch.empty_like(r)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = C.c_long(-1)

    def prepare():
        A.copy_(A0)
        x.copy_(r)

    def solve():
        L.check(lib.gemma_hip_dbg_spd_solve_d(C.c_void_p(A.data_ptr()), n, n, C.c_void_p(x.data_ptr()), C.byref(bad), stream), "solve")

    zi = [None]

    def inverse():
        api.spd_inverse(A)
        zi[0] = torch.mv(A, r)

    t_solve = timed(solve, prepare, a.reps)
    z = x.clone()
    t_inv = timed(inverse, prepare, a.reps)
    diff = float((z - zi[0]).abs().max() / z.abs().max())
    print(json.dumps(dict(n=n, factor_solve_s=t_solve, inverse_matvec_s=t_inv, ratio=t_solve / t_inv, flop_ratio=0.25, max_rel_diff=diff)))


if __name__ == "__main__":
    main()

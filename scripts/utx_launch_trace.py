#!/usr/bin/env python3
"""Which kernels the int8 U^T x launches, form by form: the check of a change to its launch site (i8_plan.h, abi_utx.inc.h) that
must leave every launch as it was.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o t -- python scripts/utx_launch_trace.py
    python scripts/utx_launch_trace.py --compare OLD_kernel_trace.csv NEW_kernel_trace.csv

The run: for every form of DESIGN 3.7's table that a small n reaches, LMM.setup and LMM.batch on a PLINK block of l = 257 SNPs
and n = 130 individuals (two ragged tile rows, two ragged column tiles, a ragged K), once with about 1 % missing calls and once
with none; the forms are switched through the environment, reload_env() and a new setup.  The two-block pipe and a block in row
chunks (l = 1100) go last.  A one-element fill on the device separates the cases in the trace.

--compare: the ordered (kernel name, grid, workgroup, LDS bytes) of the two traces, case by case; exit status 1 if any differs.
"""
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, L_SNPS, L_CHUNKED = 130, 257, 1100
SWITCHES = ("GEMMA_HIP_I8_DIGITS", "GEMMA_HIP_I8_FORM", "GEMMA_HIP_I8_COMPLETE", "GEMMA_HIP_I8_EPILOGUE", "GEMMA_HIP_I8_FUSE",
            "GEMMA_HIP_I8_ROWS", "GEMMA_HIP_I8_SPARSE", "GEMMA_HIP_I8_DIRECT", "GEMMA_HIP_OVERLAP")
FORMS = [  # n = 130 takes seven digits: four fused planes; GEMMA_HIP_I8_DIGITS=6 gives the three of n >= 16384
    ("default", {}),
    ("digits6", {"GEMMA_HIP_I8_DIGITS": "6"}),
    ("complete0", {"GEMMA_HIP_I8_COMPLETE": "0"}),
    ("7g6m", {"GEMMA_HIP_I8_FORM": "7g6m"}),
    ("7g6m complete0", {"GEMMA_HIP_I8_FORM": "7g6m", "GEMMA_HIP_I8_COMPLETE": "0"}),
    ("epilogue0", {"GEMMA_HIP_I8_EPILOGUE": "0"}),
    ("epilogue0 digits6", {"GEMMA_HIP_I8_EPILOGUE": "0", "GEMMA_HIP_I8_DIGITS": "6"}),
    ("epilogue0 complete0", {"GEMMA_HIP_I8_EPILOGUE": "0", "GEMMA_HIP_I8_COMPLETE": "0"}),
    ("epilogue0 7g6m", {"GEMMA_HIP_I8_EPILOGUE": "0", "GEMMA_HIP_I8_FORM": "7g6m"}),
    ("epilogue0 7g6m complete0", {"GEMMA_HIP_I8_EPILOGUE": "0", "GEMMA_HIP_I8_FORM": "7g6m", "GEMMA_HIP_I8_COMPLETE": "0"}),
    ("fuse0", {"GEMMA_HIP_I8_FUSE": "0"}),  # the unfused rows (n > 32640)
    ("fuse0 digits6", {"GEMMA_HIP_I8_FUSE": "0", "GEMMA_HIP_I8_DIGITS": "6"}),
    ("fuse0 7g6m", {"GEMMA_HIP_I8_FUSE": "0", "GEMMA_HIP_I8_FORM": "7g6m"}),
    ("rows32", {"GEMMA_HIP_I8_ROWS": "32"}),
    ("sparse1", {"GEMMA_HIP_I8_SPARSE": "1"}),
    ("sparse0", {"GEMMA_HIP_I8_SPARSE": "0"}),
    ("direct0", {"GEMMA_HIP_I8_DIRECT": "0"}),
    ("pipe", {}),
    ("chunked", {"GEMMA_HIP_OVERLAP": "1"}),
]
CASES = [(f"{name} / {'1 % missing' if miss else 'no missing call'}", name, env, miss) for name, env in FORMS for miss in (0.01, 0.0)]


def run():
    import numpy as np
    import torch
    from gemma_amd import api
    from gemma_amd import _lib as L

    api.init(0, verbose=0)
    rng = np.random.default_rng(5)
    U = np.linalg.qr(rng.standard_normal((N, N)))[0]
    ev = np.sort(rng.random(N) * 2.0 + 0.05)
    UtW, Uty = U.T @ np.ones((N, 1)), U.T @ rng.standard_normal(N)
    mark = torch.empty(1, device="cuda")  # no kernel: the first fill is the first separator

    def block(l, miss):  # PLINK 2-bit codes (01 = missing call), l SNPs x N individuals, four calls a byte
        codes = rng.choice([0, 1, 2, 3], size=(l, (N + 3) // 4 * 4), p=[0.25, miss, 0.45 - miss, 0.3]).astype(np.uint8)
        codes[:, N:] = 0
        return (codes[:, 0::4] | (codes[:, 1::4] << 2) | (codes[:, 2::4] << 4) | (codes[:, 3::4] << 6)).astype(np.uint8)

    for label, name, env, miss in CASES:
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)
        api.reload_env()
        raw = block(L_CHUNKED if name == "chunked" else L_SNPS, miss)
        lmm = api.LMM(a_mode=1)
        lmm.setup(U, ev, UtW, Uty, plink=True)
        torch.cuda.synchronize()
        mark.fill_(1.0)  # the separator: everything up to the next one is this case's batch
        if name == "pipe":
            g = torch.from_numpy(raw).cuda()
            out = torch.empty((raw.shape[0], 8), dtype=torch.float64, device="cuda")
            for _ in range(2):  # two blocks in flight
                lmm.batch_pipe(g, L.GENO_PLINK_2BIT, out)
            lmm.pipe_flush()
            torch.cuda.synchronize()
            res = out.cpu().numpy()
        else:
            res = lmm.batch(raw, L.GENO_PLINK_2BIT)
        lmm.finish()
        print(f"{label}: {raw.shape[0]} SNPs, {np.isfinite(np.asarray(res).view(np.float64)).mean():.3f} of the output finite", flush=True)
    mark.fill_(1.0)
    torch.cuda.synchronize()


def read_trace(path):
    """The trace as one list of launches per case: (kernel name, grid, workgroup, LDS bytes) in dispatch order."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, what: tuple(int(r[k]) for k in sorted(r) if k.startswith(what))
    cases, cur = [], None
    for r in rows:
        if "FillFunctor" in r["Kernel_Name"]:  # the separator
            cur = []
            cases.append(cur)
        elif cur is not None:  # what runs before the first separator is torch's and the first setup's
            cur.append((r["Kernel_Name"].split("(")[0], dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), int(r["LDS_Block_Size"])))
    return cases


def compare(old_path, new_path):
    old, new = read_trace(old_path), read_trace(new_path)
    # a case is the batch behind its separator and, behind that, the next case's setup; the last separator has nothing behind it
    if len(old) != len(CASES) + 1 or len(new) != len(CASES) + 1:
        print(f"expected {len(CASES) + 1} separators, found {len(old)} before and {len(new)} after")
        return 1
    bad = 0
    for (label, *_), a, b in zip(CASES, old, new):
        same = a == b
        bad += not same
        print(f"{'same' if same else 'DIFFERENT'}  {label}: {len(a)} launches before, {len(b)} after")
        i8 = [x for x in (b if same else a) if "i8gemm" in x[0]]
        for name, grid, wg, lds in i8:
            print(f"        {name}  grid {grid}  workgroup {wg}  LDS {lds}")
        if not same:
            for i, (x, y) in enumerate(zip(a, b)):
                if x != y:
                    print(f"    first difference at launch {i}: {x} -> {y}")
                    break
    print(f"{len(CASES) - bad} of {len(CASES)} cases launch the same kernels with the same grid, workgroup and LDS, in the same order")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()

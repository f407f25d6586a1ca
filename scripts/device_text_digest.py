#!/usr/bin/env python3
"""One sha256 per translation unit over its gfx950 device code: the .text bytes and the sorted kernel symbols.

A refactor that must not touch kernel arithmetic runs this before and after and compares the two columns.
Whole-file hashes differ even for a pure rename (the code object carries a unit id); .text does not.

    python scripts/device_text_digest.py [--csrc DIR] [--jobs N] [UNIT ...]
"""
import argparse
import concurrent.futures
import hashlib
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gemma_amd import build as recipe  # noqa: E402  (the unit list and the compiler are the build's own)


def digest(csrc, unit, tmp):
    cc = recipe.hipcc()
    llvm = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(cc))), "llvm", "bin")
    elf, text = os.path.join(tmp, unit + ".elf"), os.path.join(tmp, unit + ".text")
    subprocess.check_call([cc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "--offload-device-only",
                           "--no-gpu-bundle-output", "-c", os.path.join(csrc, unit), "-o", elf], cwd=csrc)
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "-O", "binary", "--only-section=.text", elf, text])
    syms = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--symbols", "--wide", elf], text=True)
    rows = [ln.split() for ln in syms.splitlines()]  # Num: Value Size Type Bind Vis Ndx Name
    kernels = sorted(r[7] for r in rows if len(r) == 8 and r[3] == "FUNC" and r[4] == "GLOBAL")
    h = hashlib.sha256(open(text, "rb").read())
    h.update("\n".join(kernels).encode())
    return h.hexdigest(), len(kernels)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", default=recipe.CSRC, help="the csrc directory to compile (default: this tree's)")
    ap.add_argument("--jobs", type=int, default=min(len(recipe.SOURCES), os.cpu_count() or 1))
    ap.add_argument("units", nargs="*", default=recipe.SOURCES)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        for unit, (sha, nk) in zip(a.units, pool.map(lambda u: digest(os.path.abspath(a.csrc), u, tmp), a.units)):
            print(f"{sha}  {unit}  ({nk} kernels)", flush=True)


if __name__ == "__main__":
    main()

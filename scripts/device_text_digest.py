#!/usr/bin/env python3
"""One sha256 per translation unit over its gfx950 device code: the .text bytes and the sorted kernel symbols.

A refactor that must not touch kernel arithmetic runs this before and after and compares the two columns.
Whole-file hashes differ even for a pure rename (the code object carries a unit id); .text does not.

    python scripts/device_text_digest.py [--csrc DIR] [--jobs N] [UNIT ...]

A refactor that MOVES kernels between units compares kernel by kernel instead:

    python scripts/device_text_digest.py --per-kernel --keep DIR [--csrc DIR] [UNIT ...] > TABLE
    python scripts/device_text_digest.py --compare OLD_TABLE NEW_TABLE

The table has one line per unit and kernel symbol: the size, a sha256 of the kernel's own bytes of .text, and the
code object's metadata of it (registers, spills, scratch, LDS).  --compare sorts every kernel into identical / same
size and metadata but other bytes / different, and prints the disassembly lines that differ for the middle class
(from the code objects --keep left in DIR, which the table names).
"""
import argparse
import concurrent.futures
import difflib
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gemma_amd import build as recipe  # noqa: E402  (the unit list and the compiler are the build's own)

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def llvm(tool):
    cc = recipe.hipcc()
    return os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(cc))), "llvm", "bin", tool)


def compile_device(csrc, unit, tmp):
    elf = os.path.join(tmp, unit + ".elf")
    subprocess.check_call([recipe.hipcc(), *recipe.FLAGS, "--offload-device-only", "--no-gpu-bundle-output", "-c",
                           os.path.join(csrc, unit), "-o", elf], cwd=csrc)
    return elf


def kernel_symbols(elf):
    """(name, value, size) of every global function symbol of a code object."""
    syms = subprocess.check_output([llvm("llvm-readelf"), "--symbols", "--wide", elf], text=True)
    rows = [ln.split() for ln in syms.splitlines()]  # Num: Value Size Type Bind Vis Ndx Name
    return sorted({(r[7], int(r[1], 16), int(r[2])) for r in rows if len(r) == 8 and r[3] == "FUNC" and r[4] == "GLOBAL"})  # .dynsym and .symtab


def digest(csrc, unit, tmp):
    elf, text = compile_device(csrc, unit, tmp), os.path.join(tmp, unit + ".text")
    subprocess.check_call([llvm("llvm-objcopy"), "-O", "binary", "--only-section=.text", elf, text])
    kernels = [k[0] for k in kernel_symbols(elf)]
    h = hashlib.sha256(open(text, "rb").read())
    h.update("\n".join(kernels).encode())
    return h.hexdigest(), len(kernels)


def per_kernel(csrc, unit, tmp):
    """One table row per kernel of the unit: name, size, sha256 of its bytes, the metadata fields of META."""
    elf, text = compile_device(csrc, unit, tmp), os.path.join(tmp, unit + ".text")
    subprocess.check_call([llvm("llvm-objcopy"), "-O", "binary", "--only-section=.text", elf, text])
    blob = open(text, "rb").read()
    secs = subprocess.check_output([llvm("llvm-readelf"), "--sections", "--wide", elf], text=True)
    base = next(int(ln.split("]")[1].split()[2], 16) for ln in secs.splitlines() if " .text " in ln)
    notes = subprocess.check_output([llvm("llvm-readelf"), "--notes", elf], text=True)
    meta, cur = {}, None
    for ln in notes.splitlines():  # the amdhsa.kernels list: one "- .key: value" map per kernel
        m = re.match(r"  (- |  )\.(\w+):\s*(.*)$", ln)  # a kernel's own keys, not those of its argument list
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        cur[m.group(2)] = m.group(3).strip("'")
        if m.group(2) == "name":
            meta[cur["name"]] = cur
    rows = []
    for name, value, size in kernel_symbols(elf):
        sha = hashlib.sha256(blob[value - base:value - base + size]).hexdigest()
        md = meta.get(name, {})
        rows.append("\t".join([unit, name, str(size), sha] + [f"{k}={md.get(k, '?')}" for k in META]))
    return rows


def read_table(path):
    """{kernel symbol: [(unit, size, sha, metadata)]} and the directory of the code objects, if the table names one."""
    table, elfdir = {}, None
    for ln in open(path):
        if ln.startswith("# elfdir "):
            elfdir = ln.split(None, 2)[2].strip()
        if ln.startswith("#") or not ln.strip():
            continue
        unit, name, size, sha, *md = ln.rstrip("\n").split("\t")
        table.setdefault(name, []).append((unit, int(size), sha, tuple(md)))
    return table, elfdir


def disassembly(elfdir, unit, name):
    out = subprocess.check_output([llvm("llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                   f"--disassemble-symbols={name}", os.path.join(elfdir, unit + ".elf")], text=True)
    return [ln.split("//")[0].rstrip() for ln in out.splitlines()]


def compare(old_path, new_path):
    (old, old_dir), (new, new_dir) = read_table(old_path), read_table(new_path)
    print(f"kernel symbols: {len(old)} before, {len(new)} after")
    for side, table, other in (("before", old, new), ("after", new, old)):  # a renamed kernel: the same size and bytes under another name
        for name in sorted(set(table) - set(other)):
            for unit, size, sha, _ in table[name]:
                print(f"only {side}: {unit}\t{name}\t{size}\t{sha}")
    same, moved, different = [], [], []
    for name in sorted(set(old) & set(new)):
        if len({c[1:] for c in old[name]}) != 1 or len({c[1:] for c in new[name]}) != 1:
            different.append(name)  # the copies of one side do not even agree with each other
            continue
        if len(old[name]) != len(new[name]):
            print(f"multiplicity {len(old[name])} -> {len(new[name])}: {name}  "
                  f"({', '.join(c[0] for c in old[name])} -> {', '.join(c[0] for c in new[name])})")
        o, n = old[name][0], new[name][0]
        (same if o[1:] == n[1:] else moved if (o[1], o[3]) == (n[1], n[3]) else different).append(name)
    print(f"identical: {len(same)}; same size and metadata, other bytes: {len(moved)}; different: {len(different)}")
    for name in moved:
        print(f"--- same size and metadata, other bytes: {name}")
        if old_dir and new_dir:
            a, b = disassembly(old_dir, old[name][0][0], name), disassembly(new_dir, new[name][0][0], name)
            for ln in difflib.unified_diff(a, b, "before", "after", n=0, lineterm=""):
                print("    " + ln)
    for name in different:
        print(f"--- DIFFERENT: {name}: {old[name]} -> {new[name]}")
    return 1 if different or set(old) != set(new) else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--csrc", default=recipe.CSRC, help="the csrc directory to compile (default: this tree's)")
    ap.add_argument("--jobs", type=int, default=min(len(recipe.SOURCES), os.cpu_count() or 1))
    ap.add_argument("--per-kernel", action="store_true", help="one line per unit and kernel instead of one per unit")
    ap.add_argument("--keep", metavar="DIR", help="with --per-kernel: leave the code objects there (for --compare's disassembly)")
    ap.add_argument("--compare", nargs=2, metavar=("OLD", "NEW"), help="compare two --per-kernel tables")
    ap.add_argument("units", nargs="*", default=None)
    a = ap.parse_args()
    if a.compare:
        sys.exit(compare(*a.compare))
    units = a.units or (recipe.SOURCES if a.csrc == recipe.CSRC else sorted(f for f in os.listdir(a.csrc) if f.endswith(".hip")))
    csrc = os.path.abspath(a.csrc)
    with tempfile.TemporaryDirectory() as tmpdir, concurrent.futures.ThreadPoolExecutor(a.jobs) as pool:
        tmp = a.keep or tmpdir
        os.makedirs(tmp, exist_ok=True)
        if a.per_kernel:
            if a.keep:
                print(f"# elfdir {os.path.abspath(a.keep)}")
            for rows in pool.map(lambda u: per_kernel(csrc, u, tmp), units):
                for row in rows:
                    print(row, flush=True)
            return
        for unit, (sha, nk) in zip(units, pool.map(lambda u: digest(csrc, u, tmp), units)):
            print(f"{sha}  {unit}  ({nk} kernels)", flush=True)


if __name__ == "__main__":
    main()

"""CPU: the kernels live in units of their own.  The C ABI unit (gemma_hip.hip: g_ctx and the abi_*.inc.h parts) and any other
source of the build that is neither a kernel unit (*_kernels*.hip) nor a feature unit (*_tu.hip, dgemm_tu.hip among them) must
compile to a gfx950 code object without a single function symbol -- an edit of the host plumbing then never regenerates a kernel.
Symbol tables only: one device-side compile per such source with the build's own flags (well under a second for gemma_hip.hip)."""
import fnmatch
import os
import subprocess

from gemma_amd import build

READELF = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "llvm", "bin", "llvm-readelf")


def _holds_kernels(src):
    return fnmatch.fnmatch(src, "*_kernels*.hip") or fnmatch.fnmatch(src, "*_tu.hip")


def _device_functions(src, tmp_path):
    elf = str(tmp_path / (src + ".elf"))
    subprocess.run([build.hipcc(), *build.FLAGS, "--offload-device-only", "--no-gpu-bundle-output", "-c", os.path.join(build.CSRC, src),
                    "-o", elf], cwd=build.CSRC, check=True, capture_output=True)
    syms = subprocess.run([READELF, "--symbols", "--wide", elf], check=True, capture_output=True, text=True).stdout
    rows = [ln.split() for ln in syms.splitlines()]  # Num: Value Size Type Bind Vis Ndx Name
    return sorted({r[7] for r in rows if len(r) == 8 and r[3] == "FUNC" and r[4] in ("GLOBAL", "WEAK")})


def test_the_sources_are_the_files_on_disk():
    on_disk = sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip"))
    assert sorted(build.SOURCES) == on_disk


def test_only_kernel_and_feature_units_define_kernels(tmp_path):
    others = [s for s in build.SOURCES if not _holds_kernels(s)]
    assert others == ["gemma_hip.hip"], others  # a new source is a kernel unit, a feature unit, or is named here and holds no kernel
    for src in others:
        assert _device_functions(src, tmp_path) == [], src

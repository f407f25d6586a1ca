"""The multi-phenotype LMM interface without a GPU: the entry points include/gemma_hip.h declares are exported by the built library
with the prototypes gemma_amd/_lib.py binds, and the file driver of the C++ mirror compiles against the headers."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gemma_hip_lmm_multi_setup", "gemma_hip_lmm_multi_setup_d", "gemma_hip_lmm_multi_setup_kept",
         "gemma_hip_lmm_multi_batch", "gemma_hip_lmm_multi_batch_d")


def _ctype_of(decl):
    """ctypes class of one C parameter declaration of include/gemma_hip.h"""
    decl = decl.strip()
    if "*" in decl:
        return "pointer"
    return {"size_t": C.c_size_t, "int": C.c_int, "double": C.c_double}[decl.split()[-2]]


def test_multi_symbols_and_prototypes():
    from gemma_amd import _lib, build
    so = build.build()
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    assert re.search(r"#define\s+GEMMA_LMM_MULTI_MAX\s+64\b", hdr) and _lib.LMM_MULTI_MAX == 64
    lib = _lib.lib()  # first: it settles which HIP runtime the process uses
    raw = C.CDLL(so)
    for name in NAMES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S)
        assert m, name + " is not declared in include/gemma_hip.h"
        assert hasattr(raw, name), name + " is not exported by the library"
        assert name in _lib.SYMBOLS
        params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
        bound = getattr(lib, name).argtypes
        assert bound is not None and len(bound) == len(params), (name, len(params))
        for decl, ct in zip(params, bound):
            want = _ctype_of(decl)
            if want == "pointer":
                assert ct is C.c_void_p or issubclass(ct, C._Pointer), (name, decl, ct)
            else:
                assert ct is want, (name, decl, ct)


def test_multi_file_driver_compiles(tmp_path):
    r = subprocess.run(["g++", "-std=c++11", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c",
                        os.path.join(ROOT, "tests", "cpp", "multi_file_driver.cpp"), "-o", str(tmp_path / "multi_file_driver.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]

"""Build recipe for the gfx950 shared library (explicit hipcc, in-tree output)."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libgemma_hip.so")
OBJDIR = os.path.join(HERE, "_obj")
# One object per source, compiled concurrently.  What each one depends on is the compiler's own list (-MD: <obj>.d), not one kept here.
SOURCES = [
    "gemma_hip.hip",          # the C ABI around g_ctx: host code only, its device side holds no kernel
    "dgemm_tu.hip",           # the fp64 MFMA GEMM, its side stream and switches: once for every unit below
    "utx_i8_kernels.hip",     # the int8 U^T x: digit planes, dense and sparse products, the records kernels
    "firstpass_kernels.hip",  # ingest, QC, the exact-integer kinship
    "lmm_kernels.hip",        # the per-SNP stage: -lm, -lmm 1/2/3/4, gene / GXE forms, tables, score and null panels
    "eigh_tu.hip",            # the eigensolver
    "vc_tu.hip",              # -vc 1 / -vc 2
    "prdt_tu.hip",            # -bslmm 2 / -predict: genotype matrix-vector passes; the Kronecker system of -predict with a kinship alone
    "mqs_tu.hip",             # -gs / -vc 1 -beta: MQS kinships, S and its jackknife; -ci: the two genotype passes
    "cor_tu.hip",             # -calccor: banded SNP correlation, int8 band kernel and fp64 panels
    "mvlmm_kernels.hip",
    "mvlmm_kernels_wide.hip",
    "mvlmm_kernels_rt.hip",   # the run-time (d, c) instance
    "mvlmm_kernels_d6.hip",   # six phenotypes, fixed form (two wavefronts per workgroup)
    "mvlmm_kernels_d7.hip",   # seven phenotypes (one wavefront per workgroup)
    "mvlmm_kernels_d8.hip",   # eight phenotypes, one covariate
    "mvlmm_kernels_pair.hip",     # two-trait null fits of a whole panel: one wavefront per pair of traits
    "mvlmm_kernels_null_se.hip",  # the fixed null fits with the variance epilogue (VVg, VVe, VB)
]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: the gfx950 library cannot be built")


def obj_of(src):
    return os.path.join(OBJDIR, src.replace(".hip", ".o"))


def obj_stale(src):
    """The object is missing, has no dependency file, or is older than a file that file names."""
    obj = obj_of(src)
    if not os.path.exists(obj) or not os.path.exists(obj + ".d"):
        return True
    deps = open(obj + ".d").read().replace("\\\n", " ").split(":", 1)[1].split()
    t = os.path.getmtime(obj)
    deps = [os.path.join(CSRC, d) for d in deps]  # the compiler runs in CSRC
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in deps)


def stale():
    return not os.path.exists(LIB) or any(obj_stale(s) or os.path.getmtime(obj_of(s)) > os.path.getmtime(LIB) for s in SOURCES)


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 -> gemma_amd/libgemma_hip.so (cross-compiles without a GPU)."""
    if not force and not stale():
        return LIB
    cc = hipcc()
    os.makedirs(OBJDIR, exist_ok=True)
    procs = []
    for src in SOURCES:
        if not force and not obj_stale(src):
            continue
        obj = obj_of(src)
        cmd = [cc, *FLAGS, "-MD", "-MF", obj + ".d", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd, cwd=CSRC)))
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    cmd = [cc, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", LIB] + [obj_of(s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB


if __name__ == "__main__":
    print(build(force=True, verbose=True))

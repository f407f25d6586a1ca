"""What the reference binary (oracle/_ref/gemma, see oracle/Makefile) prints for `-lmm 4 -n t`, t = 1, 2, 3, on the small PLINK set
of tests/multicases.py::plink_set -- the pin of tests/test_gpu_lmm_multi.py::test_multi_file_driver_writes_the_single_runs_files.
Run in the build container only:

    python tests/golden/make_multi_fixtures.py

Writes tests/golden/ref_multi.npz: the set itself (codes, pheno: the test checks that it generates the same one) and the three
.assoc.txt files as bytes.  Data only; deterministic."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import multicases as mc  # noqa: E402

GEMMA = os.path.join(ROOT, "oracle", "_ref", "gemma")


def gemma(tmp, *args):
    r = subprocess.run([GEMMA] + [str(a) for a in args], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        raise RuntimeError(r.stdout.decode()[-2000:])


def main():
    codes, pheno = mc.plink_set()
    out = {"codes": codes, "pheno": pheno}
    with tempfile.TemporaryDirectory() as tmp:
        mc.write_plink(os.path.join(tmp, "M"), codes, pheno)
        gemma(tmp, "-bfile", "M", "-gk", 1, "-o", "M")
        for t in (1, 2, 3):
            gemma(tmp, "-bfile", "M", "-k", "output/M.cXX.txt", "-lmm", 4, "-n", t, "-o", "r%d" % t)
            out["assoc%d" % t] = np.frombuffer(open(os.path.join(tmp, "output", "r%d.assoc.txt" % t), "rb").read(), dtype=np.uint8)
    np.savez_compressed(mc.REF_NPZ, **out)
    print("wrote %s (%d bytes)" % (mc.REF_NPZ, os.path.getsize(mc.REF_NPZ)))


if __name__ == "__main__":
    main()

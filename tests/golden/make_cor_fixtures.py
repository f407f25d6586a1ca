"""Files of the reference binary's `-calccor` runs (a_mode 71: prefix.cor.txt, VARCOV::WriteCov) for tests/test_cor_host.py and
tests/test_gpu_cor.py.  Run in the build container only (oracle/_ref/gemma, see oracle/Makefile):

    python tests/golden/make_cor_fixtures.py

Outputs, gzipped under tests/golden/text/ (nothing else of the reference is kept: the tests rebuild the PLINK set from
tests/golden/ref_issue188.npz and take rs / ps / alleles of its analysed SNPs from these files):
* C188ns.cor.txt.gz  issue188 (test/data/issue188/2000: 1 008 individuals, 876 analysed, 1 850 of 2 000 SNPs, one chromosome),
                     `-windowns 12`;
* C188bp.cor.txt.gz  the same set, `-windowbp 300` (windows of 0 .. 14);
* CBXD.cor.txt.gz    BXD mean genotypes with `-a` (20 chromosomes), `-windowbp 35000` (windows of 0 .. 5).

The BXD window: positions descend at four places of the annotation (chromosome 3 at 58 477 550 and 116 991 680, 16 at 92 411 606,
18 at 11 212 105).  Where the window of a SNP ends before the window of the SNP in front of it, the reference's sliding buffer
keeps the surplus row (src/varcov.cpp:289-293: the rows to read are counted from the previous n_nb, not from the buffer), from
there to the end of the file and across chromosomes: with `-windowbp 40000` and above every record after SNP 6 579 has one
neighbour more than CalcNB gave it (741 records; 1 065 from 88 273 on, 5 811 at 2 Mb).  The library computes CalcNB's windows
(INTEGRATION.md), so the fixture uses the largest round window below the first such place: up to 38 611 bp the reference's file
holds exactly CalcNB's windows on this input."""
import gzip
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GEMMA = os.path.join(ROOT, "oracle", "_ref", "gemma")
TXT = os.path.join(ROOT, "tests", "golden", "text")
REF = "/root/reference"
LIMIT = 400 * 1024


def calccor(tmp, tag, args):
    cmd = [GEMMA] + [str(a) for a in args] + ["-calccor", "-o", tag]
    r = subprocess.run(cmd, cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    src = os.path.join(tmp, "output", tag + ".cor.txt")
    if r.returncode != 0 or not os.path.exists(src):
        raise RuntimeError("%s: exit %d\n%s" % (tag, r.returncode, r.stdout[-2000:]))
    dst = os.path.join(TXT, tag + ".cor.txt.gz")
    with open(src, "rb") as f, open(dst, "wb") as g, gzip.GzipFile(fileobj=g, mode="wb", mtime=0) as z:
        z.write(f.read())
    if os.path.getsize(dst) > LIMIT:
        raise RuntimeError("%s: %d bytes gzipped" % (dst, os.path.getsize(dst)))
    print(tag, os.path.getsize(src), "->", os.path.getsize(dst))


def main():
    tmp = tempfile.mkdtemp()
    try:
        for ext in (".bed", ".bim", ".fam"):
            shutil.copy(os.path.join(REF, "test", "data", "issue188", "2000" + ext), os.path.join(tmp, "i188" + ext))
        calccor(tmp, "C188ns", ["-bfile", "i188", "-windowns", 12])
        calccor(tmp, "C188bp", ["-bfile", "i188", "-windowbp", 300])
        for src, dst in (("bxd_mean_genotypes.txt.gz", "bxd_geno.txt"), ("bxd_trait.txt.gz", "bxd_pheno.txt"),
                         ("bxd_anno.txt.gz", "bxd_anno.txt")):
            with gzip.open(os.path.join(TXT, src), "rt") as f, open(os.path.join(tmp, dst), "w") as g:
                g.write(f.read())
        calccor(tmp, "CBXD", ["-g", "bxd_geno.txt", "-p", "bxd_pheno.txt", "-a", "bxd_anno.txt", "-windowbp", 35000])
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

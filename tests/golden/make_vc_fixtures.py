"""Printed numbers of the reference binary's -vc 1 (Haseman-Elston, VC::CalcVChe) and -vc 2 (REML, VC::CalcVCreml) on the
committed PLINK set P and on BXD, for tests/test_vc_cpu.py and tests/test_gpu_vc.py -- run in the build container only (oracle/_ref/gemma, see oracle/Makefile):

    python tests/golden/make_vc_fixtures.py

P: the phenotype is P.fam's column 6 with -9 written as NA (154 of 240 analysed); the kinships are the reference's own -gk 1
of P, of all SNPs or of SNP subsets (-snps).  BXD: the reference's example (committed as bxd_*.gz), trait column 1.
Writes tests/golden/text/V*.log.json: the sigma2 / se(sigma2) / pve / se(pve) (/ total) lines and the counts of the log, as
printed:
* V1 (-k), V1c (-k, -c P.cov.txt);
* V2c (-mk of SNPs 1-400 and 401-800, -c P.cov.txt), V3 (-mk of SNPs 1-250 / 251-500 / 501-800);
* VB1 (BXD -k), VB2 (BXD -mk of the first and second half of its SNPs).
The same six runs with -vc 2 write tests/golden/text/V*r.log.json, and V1 with -vc 2 -noconstrain V1nr.log.json: the
"sigma2 = " line printed after each "iteration k" line (list "iterations", row k = iteration k) and the final estimates of the
log (the "pve estimates" / "se(pve)" / "sigma2 estimates" / "se(sigma2)" lines); a run that dies keeps the iterations it
printed and its "GSL ERROR" line ("error").  The multiroot solver of -vc 2 comes from
oracle/gslshim (an adaptor over include/gemma_vc_hybrid.hpp), the rest of the run is the reference's own code."""
import gzip
import json
import os
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GEMMA = os.path.join(ROOT, "oracle", "_ref", "gemma")
TXT = os.path.join(ROOT, "tests", "golden", "text")


def run(tmp, *args, may_fail=False):
    r = subprocess.run([GEMMA] + [str(a) for a in args], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0 and not may_fail:
        raise RuntimeError(r.stdout[-2000:])
    return r.stdout if not may_fail else (r.returncode, r.stdout)


def printed(out, log):
    meta = {}
    for line in out.splitlines():
        for key in ("sigma2", "se(sigma2)", "pve", "se(pve)", "total pve", "se(total pve)"):
            if line.startswith(key + " = "):
                meta[key] = line.split("=", 1)[1].split()
    for line in open(log):
        if line.startswith("## number of") and "SNPs" not in line:  # -vc reads no genotypes: the SNP counts are uninitialised
            k, v = line[2:].split("=", 1)
            meta[k.strip()] = v.strip()
    return meta


def printed_reml(out, log):
    meta, iters, want = {}, [], False
    for line in out.splitlines():
        if line.startswith("iteration "):
            assert int(line.split()[1]) == len(iters), line
            want = True
        elif want and line.startswith("sigma2 = "):
            iters.append(line.split("=", 1)[1].split())
            want = False
    meta["iterations"] = iters
    for line in open(log):
        if line.startswith("## number of") and "SNPs" not in line:
            k, v = line[2:].split("=", 1)
            meta[k.strip()] = v.strip()
        for key in ("pve estimates", "se(pve)", "sigma2 estimates", "se(sigma2)", "total pve", "se(total pve)"):
            if line.startswith("## " + key + " ="):
                meta[key] = line.split("=", 1)[1].split()
    return meta


def both(tmp, tag, extra, noconstrain_too=False):
    """-vc 1 -> <tag>.log.json, -vc 2 -> <tag>r.log.json (and -vc 2 -noconstrain -> <tag>nr.log.json)"""
    out = run(tmp, *extra, "-vc", 1, "-o", tag)
    meta = printed(out, os.path.join(tmp, "output", tag + ".log.txt"))
    json.dump(meta, open(os.path.join(TXT, tag + ".log.json"), "w"), indent=1, sort_keys=True)
    for suffix, flags in (("r", []), ("nr", ["-noconstrain"]))[:2 if noconstrain_too else 1]:
        rc, out = run(tmp, *extra, "-vc", 2, *flags, "-o", tag + suffix, may_fail=True)
        if rc != 0:  # the run died (a GSL error): the iterations printed before it and the error line
            meta = printed_reml(out, os.devnull)
            meta["error"] = [l.split(" in ")[0] for l in out.splitlines() if l.startswith("GSL ERROR")]
        else:
            meta = printed_reml(out, os.path.join(tmp, "output", tag + suffix + ".log.txt"))
        json.dump(meta, open(os.path.join(TXT, tag + suffix + ".log.json"), "w"), indent=1, sort_keys=True)


def snp_list(tmp, name, ids):
    open(os.path.join(tmp, name), "w").write("\n".join(ids) + "\n")
    return name


def mk(tmp, name, prefixes):
    open(os.path.join(tmp, name), "w").write("\n".join(os.path.join(tmp, "output", p + ".cXX.txt") for p in prefixes) + "\n")
    return name


def main():
    tmp = tempfile.mkdtemp()
    try:
        for ext in (".bed", ".bim", ".fam", ".cov.txt"):
            shutil.copy(os.path.join(TXT, "P" + ext), tmp)
        with open(os.path.join(tmp, "P.fam")) as f, open(os.path.join(tmp, "pheno.txt"), "w") as g:
            for line in f:
                v = line.split()[5]
                g.write(("NA" if v == "-9" else v) + "\n")
        run(tmp, "-bfile", "P", "-gk", 1, "-o", "P")
        cxx = os.path.join("output", "P.cXX.txt")
        snps = [l.split()[1] for l in open(os.path.join(tmp, "P.bim")) if l.strip()]
        for tag, cut in (("Pa", (0, 400)), ("Pb", (400, 800)), ("Pt1", (0, 250)), ("Pt2", (250, 500)), ("Pt3", (500, 800))):
            run(tmp, "-bfile", "P", "-gk", 1, "-snps", snp_list(tmp, tag + ".snps", snps[cut[0]:cut[1]]), "-o", tag)
        runs = [("V1", ["-k", cxx]), ("V1c", ["-k", cxx, "-c", "P.cov.txt"]),
                ("V2c", ["-mk", mk(tmp, "mk2.txt", ["Pa", "Pb"]), "-c", "P.cov.txt"]),
                ("V3", ["-mk", mk(tmp, "mk3.txt", ["Pt1", "Pt2", "Pt3"])])]
        for tag, extra in runs:
            both(tmp, tag, ["-p", "pheno.txt"] + extra, noconstrain_too=tag == "V1")
        # BXD
        for src, dst in (("bxd_mean_genotypes.txt.gz", "bxd_geno.txt"), ("bxd_trait.txt.gz", "bxd_pheno.txt"),
                         ("bxd_anno.txt.gz", "bxd_anno.txt")):
            with gzip.open(os.path.join(TXT, src), "rt") as f, open(os.path.join(tmp, dst), "w") as g:
                g.write(f.read())
        base = ["-g", "bxd_geno.txt", "-p", "bxd_pheno.txt", "-a", "bxd_anno.txt"]
        run(tmp, *base, "-gk", 1, "-o", "B")
        bsnps = [l.split(",")[0].strip() for l in open(os.path.join(tmp, "bxd_geno.txt")) if l.strip()]
        half = len(bsnps) // 2
        run(tmp, *base, "-gk", 1, "-snps", snp_list(tmp, "Ba.snps", bsnps[:half]), "-o", "Ba")
        run(tmp, *base, "-gk", 1, "-snps", snp_list(tmp, "Bb.snps", bsnps[half:]), "-o", "Bb")
        for tag, extra in (("VB1", ["-k", os.path.join("output", "B.cXX.txt")]), ("VB2", ["-mk", mk(tmp, "mkb.txt", ["Ba", "Bb"])])):
            both(tmp, tag, ["-p", "bxd_pheno.txt"] + extra)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()

"""gemma_amd/csrc/i8_plan.h (which form the int8 U^T x product takes, and which kernels it launches, as a pure function of the
switches and a few integers) as a stand-alone host program, tests/cpp/i8_plan_check.cpp: plain and under
-fsanitize=address,undefined.  The program only prints; every expected line below is a literal read off the launch site as it
was before the plan existed (DESIGN 3.7 has the same table), none is computed here.

A launch is printed as `kernel yN pP rR [w]`: N planes (grid.y) from plane P on, Sparse2Args::run_if R, w = an epilogue instance
(it writes U^T x).  The complete-block form queues every launch twice, run_if 1 and run_if 2, and the device runs one of each
pair; so "exactly one launch writes U^T x" is asserted for each of the two outcomes (what runs when the block has a missing call,
what runs when it has none), which is the one statement when the form is not `complete`."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _build(tmp, flags=()):
    exe = os.path.join(str(tmp), "i8_plan_check" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "cpp", "i8_plan_check.cpp"),
                           "-o", exe])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("i8_plan"))


def _run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.rstrip("\n")


R16 = "mode=r16 fuse=%d digits=%d nplanes=%d c_planes=%d mdrop=%d complete=%d epi=%d direct=1 lpad=512 mrows=1024"
PAIR_EP = " | r16_ep y1 p0 r1 w | r16_ep_g y1 p0 r2 w"
# (arguments, expected line); what is not named is at its default: sparse=2 rows=16 fuse=1 mdrop=0 complete=1 epilogue=1 direct=1,
# n = 20000 with 6 digits, l = 257 (two tile rows of 256, three of 128), no indicator map, epilogue and direct form allowed.
# GEMMA_HIP_I8_FORM=7g6m is mdrop=1 with 7 digits; digits are 7 below n = 16384.
TABLE = [
    ("", R16 % (1, 6, 3, 2, 0, 1, 1) + " | r16 y2 p1 r1 | r16_g y2 p1 r2" + PAIR_EP),
    ("n=32640", R16 % (1, 6, 3, 2, 0, 1, 1) + " | r16 y2 p1 r1 | r16_g y2 p1 r2" + PAIR_EP),
    ("n=100 digits=7", R16 % (1, 7, 4, 3, 0, 1, 1) + " | r16 y3 p1 r1 | r16_g y3 p1 r2" + PAIR_EP),
    ("complete=0", R16 % (1, 6, 3, 2, 0, 0, 1) + " | r16 y2 p1 r0 | r16_ep y1 p0 r0 w"),
    ("mdrop=1 digits=7", R16 % (1, 7, 4, 3, 1, 1, 1) + " | r16 y3 p1 r1 | r16_g y3 p1 r2 | r16_ep_g y1 p0 r0 w"),
    ("mdrop=1 digits=7 complete=0", R16 % (1, 7, 4, 3, 1, 0, 1) + " | r16 y3 p1 r0 | r16_ep_g y1 p0 r0 w"),
    ("epilogue=0", R16 % (1, 6, 3, 3, 0, 1, 0) + " | r16 y3 p0 r1 | r16_g y3 p0 r2"),
    ("allow_epi=0", R16 % (1, 6, 3, 3, 0, 1, 0) + " | r16 y3 p0 r1 | r16_g y3 p0 r2"),
    ("allow_epi=0 allow_direct=0",  # the two-block pipe
     (R16 % (1, 6, 3, 3, 0, 1, 0)).replace("direct=1", "direct=0") + " | r16 y3 p0 r1 | r16_g y3 p0 r2"),
    ("epilogue=0 complete=0", R16 % (1, 6, 3, 3, 0, 0, 0) + " | r16 y3 p0 r0"),
    ("epilogue=0 mdrop=1 digits=7", R16 % (1, 7, 4, 4, 1, 1, 0) + " | r16 y3 p1 r1 | r16_g y3 p1 r2 | r16_g y1 p0 r0"),
    ("epilogue=0 mdrop=1 digits=7 complete=0", R16 % (1, 7, 4, 4, 1, 0, 0) + " | r16 y3 p1 r0 | r16_g y1 p0 r0"),
    ("n=32641", R16 % (0, 6, 6, 5, 0, 1, 1) + " | r16 y5 p1 r1 | r16_g y5 p1 r2" + PAIR_EP),
    ("n=32641 mdrop=1 digits=7",  # unfused: the 7g6m form is silently off
     R16 % (0, 7, 7, 6, 0, 1, 1) + " | r16 y6 p1 r1 | r16_g y6 p1 r2" + PAIR_EP),
    ("fuse=0 n=100 digits=7", R16 % (0, 7, 7, 6, 0, 1, 1) + " | r16 y6 p1 r1 | r16_g y6 p1 r2" + PAIR_EP),
    ("rows=32", "mode=r32 fuse=1 digits=6 nplanes=3 c_planes=3 mdrop=0 complete=0 epi=0 direct=1 lpad=512 mrows=1024 | sparse2 y3 p0 r0"),
    ("rows=32 mdrop=1 digits=7",
     "mode=r32 fuse=1 digits=7 nplanes=4 c_planes=4 mdrop=0 complete=0 epi=0 direct=1 lpad=512 mrows=1024 | sparse2 y4 p0 r0"),
    ("sparse=1", "mode=bytes fuse=1 digits=6 nplanes=3 c_planes=3 mdrop=0 complete=0 epi=0 direct=0 lpad=384 mrows=768 | sparse y3 p0 r0"),
    ("sparse=1 mdrop=1 digits=7",
     "mode=bytes fuse=1 digits=7 nplanes=4 c_planes=4 mdrop=0 complete=0 epi=0 direct=0 lpad=384 mrows=768 | sparse y4 p0 r0"),
    ("sparse=0", "mode=dense fuse=1 digits=6 nplanes=3 c_planes=3 mdrop=0 complete=0 epi=0 direct=0 lpad=384 mrows=768 | packed<true> y3 p0 r0"),
    # direct: the switch, records mode (either row count), no indicator map, and the caller allows it
    ("direct=0", (R16 % (1, 6, 3, 2, 0, 1, 1)).replace("direct=1", "direct=0") + " | r16 y2 p1 r1 | r16_g y2 p1 r2" + PAIR_EP),
    ("have_map=1", (R16 % (1, 6, 3, 2, 0, 1, 1)).replace("direct=1", "direct=0") + " | r16 y2 p1 r1 | r16_g y2 p1 r2" + PAIR_EP),
    ("allow_direct=0", (R16 % (1, 6, 3, 2, 0, 1, 1)).replace("direct=1", "direct=0") + " | r16 y2 p1 r1 | r16_g y2 p1 r2" + PAIR_EP),
    ("rows=32 have_map=1",
     "mode=r32 fuse=1 digits=6 nplanes=3 c_planes=3 mdrop=0 complete=0 epi=0 direct=0 lpad=512 mrows=1024 | sparse2 y3 p0 r0"),
    # lpad: l rounded up to the tile height
    ("l=256", (R16 % (1, 6, 3, 2, 0, 1, 1)).replace("lpad=512 mrows=1024", "lpad=256 mrows=512") + " | r16 y2 p1 r1 | r16_g y2 p1 r2" + PAIR_EP),
    ("sparse=0 l=1", "mode=dense fuse=1 digits=6 nplanes=3 c_planes=3 mdrop=0 complete=0 epi=0 direct=0 lpad=128 mrows=256 | packed<true> y3 p0 r0"),
]


@pytest.mark.parametrize("args,line", TABLE, ids=[t[0] or "default" for t in TABLE])
def test_form_and_launches_of_the_table(exe, args, line):
    assert _run(exe, "form", *args.split()) == line


def _check_invariants(line):
    inputs, out = line.split(" => ")
    a = {k: int(v) for k, v in (kv.split("=") for kv in inputs.split())}
    head, *launches = out.split(" | ")
    f = dict(kv.split("=") for kv in head.split())
    mode = f.pop("mode")
    f = {k: int(v) for k, v in f.items()}
    L = []
    for ln in launches:
        m = re.fullmatch(r"(\S+) y(\d+) p(\d+) r([012])( w)?", ln)
        assert m, line
        L.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)), bool(m.group(5))))
    assert 1 <= len(L) <= 4, line
    r16, records = mode == "r16", mode in ("r16", "r32")
    assert mode == {0: "dense", 1: "bytes"}.get(a["sparse"], "r32" if a["rows"] == 32 else "r16"), line
    assert f["digits"] == a["digits"] and f["nplanes"] == ((a["digits"] + 1) // 2 if f["fuse"] else a["digits"]), line
    assert f["fuse"] == (1 if a["fuse"] and a["n"] <= 32640 else 0), line
    # the planes launched are exactly 0 .. nplanes - 1: once among the run_if 0 / 1 launches, once more among the run_if 2 launches
    # exactly when the form is `complete` -- but for plane 0 of the 7g6m form, the genotype product alone whatever the block
    # holds, which is queued once and runs always
    planes = lambda sel: sorted(p for (_, y, p0, r, _) in L if sel(r) for p in range(p0, p0 + y))
    assert planes(lambda r: r in (0, 1)) == list(range(f["nplanes"])), line
    assert planes(lambda r: r == 2) == (list(range(1 if f["mdrop"] else 0, f["nplanes"])) if f["complete"] else []), line
    assert {r for (_, _, _, r, _) in L} == ({0, 1, 2} if f["complete"] and f["mdrop"] else {1, 2} if f["complete"] else {0}), line
    if f["complete"] and f["mdrop"]:
        assert [(y, p0) for (_, y, p0, r, _) in L if r == 0] == [(1, 0)], line
    # for either outcome of the device-side choice every plane runs once; exactly one launch that runs writes U^T x, and only
    # when epi; it is the last one and is plane 0 alone
    for skip in (2, 1):
        ran = [x for x in L if x[3] != skip]
        assert sorted(p for (_, y, p0, _, _) in ran for p in range(p0, p0 + y)) == list(range(f["nplanes"])), line
        w = [x for x in ran if x[4]]
        assert len(w) == (1 if f["epi"] else 0), line
        if w:
            assert ran[-1] is w[0] and w[0][1:3] == (1, 0) and w[0][0] in ("r16_ep", "r16_ep_g"), line
    assert all(x[0] in ("r16_ep", "r16_ep_g") for x in L if x[4]) and all(x[4] for x in L if x[0] in ("r16_ep", "r16_ep_g")), line
    assert f["c_planes"] == f["nplanes"] - f["epi"], line
    if f["mdrop"]:
        assert f["fuse"] and f["digits"] == 7 and r16 and a["mdrop"], line
    if f["complete"]:
        assert r16 and a["complete"], line
    if f["epi"]:
        assert r16 and a["allow_epi"] and a["epilogue"], line
    if f["direct"]:
        assert records and not a["have_map"] and a["direct"] and a["allow_direct"], line
    # and the other way round: what is asked for and possible is given
    assert f["mdrop"] == (1 if a["mdrop"] and f["fuse"] and a["digits"] == 7 and r16 else 0), line
    assert f["complete"] == (1 if a["complete"] and r16 else 0), line
    assert f["epi"] == (1 if a["epilogue"] and a["allow_epi"] and r16 else 0), line  # nplanes >= 3 in every case here
    assert f["direct"] == (1 if a["direct"] and a["allow_direct"] and records and not a["have_map"] else 0), line
    tile = 256 if records else 128
    assert f["lpad"] >= a["l"] and f["lpad"] % tile == 0 and f["lpad"] - a["l"] < tile and f["mrows"] == 2 * f["lpad"], line
    # kernels belong to their mode
    names = {x[0] for x in L}
    assert names <= ({"r16", "r16_g", "r16_ep", "r16_ep_g"} if r16 else
                     {{"r32": "sparse2", "bytes": "sparse", "dense": "packed<true>"}[mode]}), line
    if not r16:
        assert L == [(L[0][0], f["nplanes"], 0, 0, False)], line


def test_invariants_over_the_cross_product(exe):
    lines = _run(exe, "sweep").split("\n")
    assert len(lines) == 3 * 2 * 2 * 2 * 2 ** 9 and len(set(lines)) == len(lines)
    for line in lines:
        _check_invariants(line)


@pytest.mark.parametrize("args,want", [
    ("l=20000", 1),                                  # GEMMA_HIP_OVERLAP is off
    ("overlap=1 l=1023", 1),
    ("overlap=1 l=1024", 2),                         # four asked for (the default), two tile rows per chunk
    ("overlap=1 l=2048", 4),
    ("overlap=1 l=20000", 4),
    ("overlap=1 chunks=100 l=20000", 16),
    ("overlap=1 chunks=0 l=20000", 1),
    ("overlap=1 chunks=3 l=1536", 3),
    ("overlap=1 chunks=3 l=1535", 2),
    ("overlap=1 utx_i8=0 l=20000", 1),
    ("overlap=1 sparse=1 l=20000", 1),
    ("overlap=1 sparse=0 l=20000", 1),
    ("overlap=1 rows=32 l=20000", 4),                # records, either row count
])
def test_chunks(exe, args, want):
    assert _run(exe, "chunks", *args.split()) == str(want)


@pytest.mark.parametrize("args,want", [
    ("kind=1", 1), ("kind=1 rows=32", 1), ("kind=0", 0), ("kind=2", 0), ("kind=1 utx_i8=0", 0), ("kind=1 sparse=1", 0),
    ("kind=1 sparse=0", 0),
])
def test_pipe_eligible(exe, args, want):
    """kind: GEMMA_GENO_F64_SNP_MAJOR = 0, GEMMA_GENO_PLINK_2BIT = 1, GEMMA_GENO_F64_IDV_MAJOR = 2 (include/gemma_hip.h)."""
    assert _run(exe, "pipe", *args.split()) == str(want)


def test_under_sanitizers(tmp_path):
    """Its own main: no preloading.  Skipped only where g++ cannot link -fsanitize=address,undefined at all."""
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++", *SAN, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ does not link -fsanitize=address,undefined here")
    san = _build(tmp_path, SAN)
    plain = _build(tmp_path)
    for args in (["sweep"], ["form"], ["form", "sparse=0", "l=1"], ["chunks", "overlap=1", "l=1024"], ["pipe"]):
        assert _run(san, *args) == _run(plain, *args)
    for args, line in TABLE:
        assert _run(san, "form", *args.split()) == line

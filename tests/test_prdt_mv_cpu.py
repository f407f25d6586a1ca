"""Kinship-only prediction for several phenotypes without a GPU: the two numpy restatements against each other and against the
files the reference printed (with the C restatement's null fit), and the declarations the feature adds."""
import os
import re
import subprocess

import numpy as np
import pytest

import prdtcases as pc
import prdtmvcases as mc

ROOT = pc.ROOT
NEW = ("gemma_hip_prdt_kin_mv_apply", "gemma_hip_prdt_kin_mv_apply_d", "gemma_hip_prdt_kin_mv")


@pytest.mark.parametrize("tag", sorted(mc.RUNS))
def test_dense_and_structured_restatement_agree(tag, oracle):
    c, f = mc.inputs(tag), mc.oracle_fit(oracle, tag)
    dense = mc.mvnorm_prdt_multi_dense(c["G_full"], c["ind"], c["W"], c["Y"], f["Vg"], f["Ve"], f["B"])
    struct = mc.mvnorm_prdt_multi(c["G_full"], c["ind"], c["W"], c["Y"], f["Vg"], f["Ve"], f["B"])
    miss = c["ind"] == 0
    diff = np.abs(dense - struct)[miss].max()
    print("%s: %d missing entries, largest difference %.3g, largest prediction %.3g" % (tag, int(miss.sum()), diff, np.abs(dense[miss]).max()))
    assert np.array_equal(dense[~miss], c["Y"][~miss]) and np.array_equal(struct[~miss], c["Y"][~miss])
    assert diff <= 1e-12 * np.abs(dense[miss]).max()


@pytest.mark.parametrize("tag", sorted(mc.RUNS))
def test_dense_restatement_meets_the_reference_file(tag, oracle):
    """the reference's .prdt.txt and its printed Vg / Ve at the bound of six printed digits, nothing added"""
    c, f, log = mc.inputs(tag), mc.oracle_fit(oracle, tag), mc.fx_log(tag)
    assert int(log["number of individuals with full phenotypes"]) == len(mc.complete(c["ind"]))
    assert int(log["number of observed data"]) == int((c["ind"] != 0).sum())
    assert int(log["number of missing data"]) == int((c["ind"] == 0).sum())
    dense = mc.mvnorm_prdt_multi_dense(c["G_full"], c["ind"], c["W"], c["Y"], f["Vg"], f["Ve"], f["B"])
    pc.assert_printed(dense, mc.fx_prdt(tag), tag + " Y_full")
    pc.assert_printed(mc.lower(f["Vg"]), mc.log_lower(log["Vg"]), tag + " Vg")
    pc.assert_printed(mc.lower(f["Ve"]), mc.log_lower(log["Ve"]), tag + " Ve")


def test_header_and_binding_declare_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "gemma_hip.h")).read()
    declared = set(re.findall(r"\b(gemma_hip_[A-Za-z0-9_]+)\s*\(", hdr))
    from gemma_amd import _lib
    for name in NEW:
        assert name in declared, name
        assert name in _lib.SYMBOLS, name
    assert "is not provided" not in hdr[hdr.index("int gemma_hip_prdt_end"):hdr.index("int gemma_hip_prdt_kin(")]


def test_cpp_mirror_and_driver_compile():
    for src in (os.path.join("tests", "cpp", "prdt_mv_driver.cpp"),):
        subprocess.check_call(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, src)])
    hpp = open(os.path.join(ROOT, "include", "gemma_host.hpp")).read()
    assert "gemma_hip_prdt_kin_mv(" in hpp and "gemma_hip_prdt_kin_mv_apply(" in hpp

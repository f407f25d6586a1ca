"""CPU: the records of the records kernel taken straight from 2-bit PLINK codes (gemma_amd/csrc/plink_records.hip.h) against the
numpy record encoder of tests/test_sparse_mask_words.py.

1. The encoder fed from 2-bit codes through the code -> value map (0 -> 2, 1 -> missing, 2 -> 1, 3 -> 0) gives what it gives from
   the packed bytes g | m << 4 that ingest_i8_kernel writes, the index word 0xCCCCCCCC of an all-padding group included.
2. The word arithmetic of the one-pass kernel, compiled for the host (tests/host/plink_records_harness.cpp), gives those records,
   the row sums behind mean_s and the dropped-call count -- for ragged rows, K padding, rows missing for most individuals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from test_sparse_mask_words import encode, record

HERE = os.path.dirname(os.path.abspath(__file__))
BK = 128  # I8_BK: individuals of a K-tile
CODE_TO_BYTE = np.array([2, 16, 1, 0], dtype=np.uint8)  # ingest_i8_kernel: (0x00011002 >> 8 c) & 0xFF


def _pack(codes):
    pad = np.zeros((len(codes) + 3) // 4 * 4, dtype=np.uint8)
    pad[:len(codes)] = codes
    return (pad[0::4] | (pad[1::4] << 2) | (pad[2::4] << 4) | (pad[3::4] << 6)).astype(np.uint8)


def _codes_from_bed(bed, n):
    """the n calls of a .bed row, as plink_records_kernel reads them: call i at bits 2 (i % 4) of byte i / 4"""
    return np.array([(int(bed[i >> 2]) >> (2 * (i & 3))) & 3 for i in range(n)], dtype=np.uint8)


def _records_from_codes(codes, ldk):
    """numpy encoder fed from 2-bit codes: value and missing flag by the map, calls n .. ldk absent"""
    n = len(codes)
    val = np.zeros(ldk, dtype=np.uint8)
    mis = np.zeros(ldk, dtype=np.uint8)
    val[:n] = np.array([2, 0, 1, 0], dtype=np.uint8)[codes]
    mis[:n] = codes == 1
    row = (val | (mis << 4)).astype(np.uint8)
    out, dropped = [], 0
    for kt in range(ldk // BK):
        for c in range(4):
            w0, w1, idx, bits, d = record(row[kt * BK:(kt + 1) * BK], c >> 1, c & 1)
            out += [w0, w1, idx, bits]
            dropped += len(d)
    return np.array(out, dtype=np.uint32), dropped


def _records_from_bytes(codes, ldk):
    """numpy encoder fed from ingest_i8_kernel's bytes"""
    row = np.zeros(ldk, dtype=np.uint8)
    row[:len(codes)] = CODE_TO_BYTE[codes]
    out, dropped = [], 0
    for kt in range(ldk // BK):
        for c in range(4):
            w0, w1, idx, bits, d = record(row[kt * BK:(kt + 1) * BK], c >> 1, c & 1)
            out += [w0, w1, idx, bits]
            dropped += len(d)
    return np.array(out, dtype=np.uint32), dropped


CASES = [(613, 0.01, 1), (530, 0.05, 2), (200, 0.3, 3), (257, 0.7, 4), (128, 0.0, 5), (1, 1.0, 6), (131, 1.0, 7)]


@pytest.mark.parametrize("n,miss,seed", CASES)
def test_encoder_from_codes_equals_encoder_from_bytes(n, miss, seed):
    rng = np.random.default_rng(seed)
    codes = rng.choice([0, 1, 2, 3], size=n, p=[0.3 * (1 - miss), miss, 0.4 * (1 - miss), 0.3 * (1 - miss)]).astype(np.uint8)
    ldk = (n + BK - 1) // BK * BK + BK  # one all-padding K-tile behind the data
    a, da = _records_from_codes(codes, ldk)
    b, db = _records_from_bytes(codes, ldk)
    assert a.tobytes() == b.tobytes() and da == db
    # the all-padding K-tile: genotype 0, kept bits 0, index word 0xCCCCCCCC
    assert a[-16:].reshape(4, 4).tolist() == [[0, 0, 0xCCCCCCCC, 0]] * 4
    assert encode([0] * 32)[:2] == (0xCCCCCCCC, 0)


@pytest.fixture(scope="module")
def harness():
    src = os.path.join(HERE, "host", "plink_records_harness.cpp")
    so = os.path.join(HERE, "host", "libplink_records_harness.so")
    hdr = os.path.join(HERE, "..", "gemma_amd", "csrc", "plink_records.hip.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    H = C.CDLL(so)
    for f in (H.pr_row_new, H.pr_row_ref):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return H


def _run(fn, bed, n, ldk):
    out = np.zeros(ldk // BK * 16, dtype=np.uint32)
    tot, mis = C.c_int(), C.c_int()
    sur = fn(bed.ctypes.data, n, ldk, out.ctypes.data, C.byref(tot), C.byref(mis))
    return out, sur, tot.value, mis.value


@pytest.mark.parametrize("n,miss,seed", CASES)
def test_one_pass_words_equal_the_numpy_encoder(harness, n, miss, seed):
    rng = np.random.default_rng(100 + seed)
    codes = rng.choice([0, 1, 2, 3], size=n, p=[0.3 * (1 - miss), miss, 0.4 * (1 - miss), 0.3 * (1 - miss)]).astype(np.uint8)
    bed = _pack(codes)
    if n % 4:  # the calls behind a ragged last byte are no calls, whatever the byte holds
        bed[-1] |= np.uint8((0x55 << (2 * (n % 4))) & 0xFF)
    assert np.array_equal(_codes_from_bed(bed, n), codes)
    ldk = (n + BK - 1) // BK * BK + BK
    want, dropped = _records_from_codes(codes, ldk)
    got, sur, tot, mis = _run(harness.pr_row_new, bed, n, ldk)
    assert got.tobytes() == want.tobytes()
    assert sur == dropped and mis == int((codes == 1).sum())
    assert tot == int(np.array([2, 0, 1, 0])[codes].sum())
    ref, sur_r, tot_r, mis_r = _run(harness.pr_row_ref, bed, n, ldk)  # the restatement of the two replaced kernels agrees
    assert ref.tobytes() == want.tobytes() and (sur_r, tot_r, mis_r) == (sur, tot, mis)
    if miss >= 0.3 and n >= BK:
        assert dropped > 0  # a case that meets no dropped call proves nothing

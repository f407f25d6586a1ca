"""Build-quality guard for the epilogue instances of the 16-row records kernel (CPU; the built library and llvm-objdump):
i8gemm_sparse2_r16_ep_kernel / _ep_g_kernel are plane 0 of the digit product with the digit combine behind their K loop
(gemma_amd/csrc/i8gemm_sparse2_r16.hip.h, COMBINE).  They must keep the steady-state K loop of the instances they are built from,
instruction count for instruction count, and must not spill anywhere: a scratch access is a vector-memory operation the counted
s_waitcnt vmcnt of the LDS-DMA pipeline does not know about."""
import os
import re

import pytest

from test_isa_schedule import LIB, OBJDUMP, _kernel_text, _steady_loop

needs_lib = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP)), reason="needs the built library and llvm-objdump")

LOOP_OPS = (r"v_mfma_i32_16x16x64_i8", r"v_smfmac_i32_16x16x128_i8", r"global_load_lds_dwordx4", r"ds_read_b128", r"ds_read",
            r"s_barrier", r"s_waitcnt vmcnt\(8\)", r"s_waitcnt vmcnt\(0\)", r"s_waitcnt vmcnt", r"v_permlane", r"v_mov_b32",
            r"global_load_dword", r"global_store", r"scratch_", r"buffer_")


def _loop_counts(tmp_path, sub, symbol):
    work = tmp_path / sub
    work.mkdir()
    lines = _kernel_text(work, symbol)
    assert lines, "%s not found in the gfx950 code object" % symbol
    ops, body = _steady_loop(lines)
    assert body is not None
    return ops, body, {pat: sum(bool(re.match(pat, o)) for o in body) for pat in LOOP_OPS}


@needs_lib
@pytest.mark.parametrize("new, base, dense, sparse", [
    ("i8gemm_sparse2_r16_ep_kernel", "i8gemm_sparse2_r16_kernel", 32, 16),
    ("i8gemm_sparse2_r16_ep_g_kernel", "i8gemm_sparse2_r16_g_kernel", 32, 0),
])
def test_epilogue_instance_keeps_the_k_loop_and_does_not_spill(tmp_path, new, base, dense, sparse):
    ops, body, got = _loop_counts(tmp_path, "new", new)
    _, base_body, want = _loop_counts(tmp_path, "base", base)
    # no scratch access anywhere in the kernel, the epilogue included
    assert not any(o.startswith("scratch_") for o in ops), [o for o in ops if o.startswith("scratch_")][:4]
    # the loop is the base instance's: same counts of everything the schedule is made of
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert len(body) == len(base_body), (len(body), len(base_body))
    # and those counts are the ones the kernel writes down
    assert got[r"v_mfma_i32_16x16x64_i8"] == dense and got[r"v_smfmac_i32_16x16x128_i8"] == sparse
    assert got[r"global_load_lds_dwordx4"] == 4 and got[r"ds_read_b128"] == 20 and got[r"ds_read"] == 20
    assert got[r"s_barrier"] == 1
    assert got[r"s_waitcnt vmcnt\(8\)"] == 1 and got[r"s_waitcnt vmcnt"] == 1, [o for o in body if "vmcnt" in o]
    # none of the epilogue's memory operations inside the loop
    assert got[r"global_load_dword"] == 0 and got[r"global_store"] == 0 and got[r"scratch_"] == 0 and got[r"buffer_"] == 0
    # the epilogue is there: it reads planes (dword loads), stores fp64 (dwordx2) and stores no int32 plane
    assert any(re.match(r"global_load_dword\s", o) for o in ops)
    assert any(re.match(r"global_store_dwordx2\s", o) for o in ops)
    assert not any(re.match(r"global_store_dword\s", o) for o in ops)
    # every plane load is issued behind the last matrix instruction of the kernel
    last_mat = max(i for i, o in enumerate(ops) if re.match(r"v_s?mfma", o))
    first_ld = min(i for i, o in enumerate(ops) if re.match(r"global_load_dword\s", o))
    assert first_ld > last_mat


@needs_lib
def test_epilogue_instance_without_mask_product_has_no_sparse_instruction(tmp_path):
    lines = _kernel_text(tmp_path, "i8gemm_sparse2_r16_ep_g_kernel")
    assert lines
    assert not any("v_smfmac" in ln for ln in lines)

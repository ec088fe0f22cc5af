"""CPU tier: the kernels of csrc/ans_coder.hip keep an element's four calls and the coder state in registers (no
scratch), as test_mixture_no_scratch.py checks for the mixture coder.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_ans_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    # the encoder, the decoder with its tables in LDS and read through L2, and the two kernels that pack the strings
    parts = ("ans_enc_kernel", "ans_dec_kernel", "ans_offsets_kernel", "ans_pack_kernel")
    named = {n: r for n, r in table.items() if any(part in n for part in parts)}
    counts = {part: sum(part in n for n in named) for part in parts}
    assert counts == {"ans_enc_kernel": 1, "ans_dec_kernel": 2, "ans_offsets_kernel": 1, "ans_pack_kernel": 1}, counts
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled

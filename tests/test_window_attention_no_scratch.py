"""CPU tier: every kernel of csrc/window_attention.hip keeps its q row, its scores and its accumulators in registers
(no scratch), as test_vecvq_no_scratch.py checks for the ECVQ kernels.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["wa_forward_kernel", "wa_forward_mfma_kernel", "wa_backward_kernel", "wa_dtable_merge_kernel"]


def test_window_attention_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    # every kernel of the file (they all carry the wa_ prefix), not only the ones listed
    named = {n: r for n, r in table.items() if "wa_" in n and "kernel" in n and "WaParams" in n or "wa_dtable" in n}
    for key in HOT:
        assert any(key in n for n in named), key
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    # one forward (float32: VALU, bfloat16: MFMA) and one backward per (window, head dimension, dtype)
    assert len([n for n in named if "wa_forward_kernel" in n]) == 4
    assert len([n for n in named if "wa_forward_mfma_kernel" in n]) == 4
    assert len([n for n in named if "wa_backward_kernel" in n]) == 8

"""CPU tier: the kernels of csrc/integer_conv.hip keep their sixteen accumulator tiles and both sets of operand fragments
in registers (no scratch), as test_window_attention_no_scratch.py checks for the attention kernels.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_integer_conv_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "integer_conv_kernel" in n}
    # one kernel per activation type: int8, and uint8 carried as a - 128
    assert len(named) == 2, sorted(named)
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled

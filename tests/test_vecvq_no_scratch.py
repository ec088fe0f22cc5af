"""CPU tier: every kernel of csrc/vecvq.hip keeps its rows, partial sums and batches in registers (no scratch), as
test_lpips_no_scratch.py checks for LPIPS.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["vecvq_assign_narrow_kernel", "vecvq_assign_wide_kernel", "vecvq_assign_merge_kernel", "vecvq_bwd_x_kernel",
       "vecvq_bwd_gather_kernel", "vecvq_bwd_merge_kernel"]


def test_vecvq_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "vecvq" in n}
    for key in HOT:
        assert any(key in n for n in named), key
    # every kernel of the file, not only the ones listed: a new one is held to the same rule
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    assert len([n for n in named if "vecvq_assign_narrow_kernel" in n]) >= 2     # one per padded width

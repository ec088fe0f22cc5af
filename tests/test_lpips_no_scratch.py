"""CPU tier: the LPIPS distance head keeps a pixel's two rows, the weights and the sums in registers, and the max-pool its
window state (no scratch), as test_channel_norm_no_scratch.py checks for ChannelNorm.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["lpips_vec_kernel", "lpips_row_kernel", "lpips_final_kernel", "maxpool_fwd_kernel", "maxpool_bwd_kernel"]


def test_lpips_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    for key in HOT:
        hits = {n: r for n, r in table.items() if key in n}
        assert hits, key
        spilled = {n: r["scratch"] for n, r in hits.items() if r["scratch"]}
        assert not spilled, spilled

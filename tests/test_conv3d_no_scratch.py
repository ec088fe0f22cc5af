"""CPU tier: the rank-3 convolution kernels keep their state in registers (no scratch), as test_no_scratch.py checks
for the other hot kernels."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["conv3d_fwd_kernel", "conv3d_wgrad_kernel", "conv3d_pack_kernel", "conv_split_x_kernel", "conv3d_wgrad_sum_kernel"]


def test_conv3d_kernels_do_not_spill():
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

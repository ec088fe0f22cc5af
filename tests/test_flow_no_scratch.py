"""CPU tier: every kernel of csrc/scale_space.hip keeps its tiles and accumulators in registers and LDS (no scratch)
and its LDS within 64 KiB (two workgroups a CU), as test_lvac_no_scratch.py checks for the LVAC kernels.  Metadata
only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["scale_space_row_forward_kernel", "scale_space_col_kernel", "scale_space_row_adjoint_kernel",
       "scale_space_warp_forward_kernel", "scale_space_warp_backward_kernel", "scale_space_absmax_kernel",
       "scale_space_absmax_final_kernel", "scale_space_fixed_to_float_kernel"]


def test_scale_space_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "scale_space" in n}
    for key in HOT:
        assert any(key in n for n in named), key
    # every instantiation (channel counts 1..8, float and fixed-point adjoints), not only the ones listed
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    over = {n: r["lds"] for n, r in named.items() if r["lds"] > 65536}
    assert not over, over

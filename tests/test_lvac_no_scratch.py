"""CPU tier: every kernel of csrc/lvac.hip keeps its tiles, accumulators and level loops in registers and LDS (no
scratch), as test_vecvq_no_scratch.py checks for the ECVQ kernels.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["lvac_raht_forward_kernel", "lvac_raht_backward_kernel", "lvac_point_mlp_forward_kernel",
       "lvac_point_mlp_sum_kernel", "lvac_point_mlp_bwd_input_kernel", "lvac_point_mlp_bwd_blocks_kernel",
       "lvac_point_mlp_bwd_param_kernel", "lvac_point_mlp_merge_kernel"]


def test_lvac_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if any(key in n for key in ("lvac", "raht", "point_mlp"))}
    for key in HOT:
        assert any(key in n for n in named), key
    # every kernel of the file, not only the ones listed: a new one is held to the same rule
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    # the two recomputing kernels hold a 64 KiB LDS budget (two workgroups a CU)
    assert all(r["lds"] <= 65536 for r in named.values())

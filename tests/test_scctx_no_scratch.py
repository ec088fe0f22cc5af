"""CPU tier: exactly the kernels of csrc/space_channel.hip exist, which run the space-channel and the checkerboard
context model (its one-group case), keep their accumulators in registers (no scratch) and their LDS within what they
state: the two instantiations of scctx_params_kernel declare gfx950's whole 160 KiB on purpose (CKB_LDS_FLOATS; DESIGN
sections 22 and 23), scctx_place_kernel uses none.  No kernel of the former checkerboard.hip is left.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_scctx_kernels_exist_and_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "scctx_" in n}
    params = {n: r for n, r in named.items() if "scctx_params_kernel" in n}
    place = {n: r for n, r in named.items() if "scctx_place_kernel" in n}
    assert len(params) == 2 and len(place) == 1 and len(named) == 3, sorted(named)      # pass 0, pass 1, place
    # the counts of the other kernel families' metadata tests go by these substrings
    assert not any(s in n for n in named for s in ("checkerboard_", "context_kernel", "scale_space"))
    # the checkerboard model has no kernels of its own
    assert not [n for n in table if "checkerboard_" in n]
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    from compression_amd.ops.checkerboard_ops import CHECKERBOARD_CONSTANTS
    stated = 4 * CHECKERBOARD_CONSTANTS["CKB_LDS_FLOATS"]
    assert stated == 160 * 1024
    # the activations are a static array: the metadata shows all the LDS the kernels use
    assert all(r["lds"] == stated for r in params.values()), params
    assert all(r["lds"] == 0 for r in place.values()), place
    # one workgroup of four waves per CU: a wave may fill a SIMD's register file (the metadata's vgpr count is the
    # unified one, accumulation registers included), and no more
    assert all(r["agpr"] <= r["vgpr"] <= 512 for r in params.values()), params

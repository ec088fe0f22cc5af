"""CPU tier: the kernels of csrc/checkerboard.hip exist, keep their accumulators in registers (no scratch) and their
LDS within what they state: the two instantiations of checkerboard_params_kernel declare gfx950's whole 160 KiB on
purpose (CKB_LDS_FLOATS), checkerboard_place_kernel uses none.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_checkerboard_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "checkerboard_" in n}
    params = {n: r for n, r in named.items() if "checkerboard_params_kernel" in n}
    place = {n: r for n, r in named.items() if "checkerboard_place_kernel" in n}
    assert len(params) == 2 and len(place) == 1 and len(named) == 3, sorted(named)      # pass 0, pass 1, place
    assert not any("context_kernel" in n for n in named)
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

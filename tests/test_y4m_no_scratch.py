"""CPU tier: every kernel of csrc/y4m.hip keeps its pixels in registers (no scratch), as test_vecvq_no_scratch.py checks
for the ECVQ kernels.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["y4m_unpack_kernel", "y4m_pack_kernel", "ycbcr_to_rgb_kernel", "rgb_to_ycbcr_kernel"]


def test_y4m_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "y4m" in n or "ycbcr" in n}
    for key in HOT:
        assert any(key in n for n in named), key
    # every kernel of the file, not only the ones listed: a new one is held to the same rule
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    # one conversion kernel per element type and chroma mode
    assert len([n for n in named if "ycbcr_to_rgb_kernel" in n]) == 9
    assert len([n for n in named if "rgb_to_ycbcr_kernel" in n]) == 6

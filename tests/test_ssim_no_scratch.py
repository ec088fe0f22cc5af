"""CPU tier: the SSIM scale-pass kernels are in libtfc_hip.so and keep their accumulators and run-time taps out of
scratch memory, as test_channel_norm_no_scratch.py checks for ChannelNorm."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["ssim_fwd_kernel", "ssim_bwd_kernel"]


def test_ssim_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    for key in HOT:
        hits = {n: r for n, r in table.items() if key in n}
        assert len(hits) == 12, (key, sorted(hits))         # 4 input dtypes x (two tile sizes + the 11-tap variant)
        spilled = {n: r["scratch"] for n, r in hits.items() if r["scratch"]}
        assert not spilled, spilled

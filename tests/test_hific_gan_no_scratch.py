"""CPU tier: the kernels of csrc/hific_gan.hip keep everything in registers (no scratch), as
test_channel_norm_no_scratch.py checks for ChannelNorm."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _kernels_of_the_source():
    text = open(os.path.join(ROOT, "compression_amd", "csrc", "hific_gan.hip")).read()
    return sorted(set(re.findall(r"__global__ void __launch_bounds__\(\d+\) (\w+)\(", text)))


def test_hific_gan_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    names = _kernels_of_the_source()
    assert len(names) >= 12, names
    for key in names:
        hits = {n: r for n, r in table.items() if key in n}
        assert hits, key
        spilled = {n: r["scratch"] for n, r in hits.items() if r["scratch"]}
        assert not spilled, spilled

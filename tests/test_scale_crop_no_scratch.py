"""CPU tier: the kernel of csrc/scale_crop.hip keeps its values in registers (no scratch), as test_train_no_scratch.py
checks for the kernels of csrc/train.hip.  Metadata of the built library only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_scale_crop_kernel_does_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "scale_crop_kernel" in n}
    # one kernel per output type: float32 and bfloat16
    assert len(named) == 2, sorted(named)
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled

"""CPU tier: both kernels of csrc/train.hip keep their values in registers (no scratch), as test_y4m_no_scratch.py checks
for the Y4M kernels.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ["crop_patches_kernel", "keras_adam_kernel"]


def test_train_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if any(key in n for key in HOT)}
    for key in HOT:
        assert any(key in n for n in named), key
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    # one crop kernel per element type, one optimiser kernel
    assert len([n for n in named if "crop_patches_kernel" in n]) == 3
    assert len([n for n in named if "keras_adam_kernel" in n]) == 1

"""CPU tier: both instantiations of the context-model kernel (csrc/context_model.hip) keep their accumulators in
registers (no scratch) and their activations within 64 KiB of LDS, as test_flow_no_scratch.py checks for the scale-space
kernels.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_context_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "context_kernel" in n}
    assert len(named) == 2, sorted(named)                   # scan and decode
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled
    over = {n: r["lds"] for n, r in named.items() if r["lds"] > 65536}
    assert not over, over
    # the activations are a static array: the metadata shows all the LDS the kernels use
    from compression_amd.ops.context_ops import CONTEXT_CONSTANTS
    assert all(r["lds"] >= 4 * CONTEXT_CONSTANTS["CTX_LDS_FLOATS"] for r in named.values())

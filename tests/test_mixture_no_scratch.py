"""CPU tier: the kernels of csrc/mixture_coder.hip and csrc/mixture_bits.hip keep a mixture's 3 K parameters and the
coder state in registers (no scratch), for every K they are instantiated for, as test_integer_conv_no_scratch.py
checks for the integer convolution.  Metadata only."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def test_mixture_kernels_do_not_spill():
    lib = os.path.join(ROOT, "compression_amd", "libtfc_hip.so")
    if not os.path.exists(lib):
        pytest.skip("libtfc_hip.so is not built")
    import check_scratch
    table = check_scratch.scan(lib)
    named = {n: r for n, r in table.items() if "mixture_" in n and "_kernel" in n}
    # K = 1 ... 4 of the encoder, the decoder and the table dump; K x {float32, bfloat16} of the two likelihood kernels;
    # the offsets and gather kernels behind the encoder
    counts = {part: sum(part in n for n in named) for part in (
        "mixture_enc_kernel", "mixture_dec_kernel", "mixture_cdf_kernel", "mixture_bits_forward_kernel",
        "mixture_bits_backward_kernel", "mixture_offsets_kernel", "mixture_gather_kernel")}
    assert counts == {"mixture_enc_kernel": 4, "mixture_dec_kernel": 4, "mixture_cdf_kernel": 4,
                      "mixture_bits_forward_kernel": 8, "mixture_bits_backward_kernel": 8,
                      "mixture_offsets_kernel": 1, "mixture_gather_kernel": 1}, counts
    spilled = {n: r["scratch"] for n, r in named.items() if r["scratch"]}
    assert not spilled, spilled

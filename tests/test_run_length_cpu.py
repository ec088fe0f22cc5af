"""CPU tier of the run-length gamma / Rice codec: the two restatements (tests/run_length_ref.py) against the
reference's pinned vectors and each other, decode error texts, model validation, and the C ABI entries."""
import ctypes
import os
import re

import numpy as np
import pytest

import run_length_ref as ref
from conftest import ROOT

# run_length_kernels_test.cc: EncodeConsistent / DecodeConsistent, ManualEncode-, ManualDecodeWithBitcodingLibrary
PINNED = [
    ([-6, 3, 0, 0], bytes([0b11010001, 0b01101101])),
    ([0, -3, 1], bytes([0xE2, 0x03])),       # gamma(2), 0, gamma(3), gamma(1), 1, gamma(1)
    ([-3, 1, 0, 0], bytes([0xF9, 0x06])),    # gamma(1), 0, gamma(3), gamma(1), 1, gamma(1), gamma(3)
]
COMBOS = [(rl, mag, flag) for rl in (-1, 0, 2, 3) for mag in (-1, 0, 4, 5) for flag in (False, True)]


@pytest.mark.parametrize("data,code", PINNED)
def test_pinned_vectors(data, code):
    assert ref.encode(data) == code
    assert ref.gamma_encode(data) == code
    assert ref.encode_np(data) == code
    assert ref.decode(code, len(data)).tolist() == data


def test_hand_built_bitwriter_sequences():
    w = ref.BitWriter()
    for g, bit in ((2, 0), (3, None), (1, 1), (1, None)):
        w.write_gamma(g)
        if bit is not None:
            w.write_one_bit(bit)
    assert w.data() == PINNED[1][1]


def _random(rng, n, zeros=0.7, scale=6.0):
    x = np.round(rng.laplace(0, scale, n)).astype(np.int64)
    x[rng.random(n) < zeros] = 0
    return x


@pytest.mark.parametrize("rl,mag,flag", COMBOS)
def test_restatements_agree(rl, mag, flag):
    rng = np.random.default_rng(abs(hash((rl, mag, flag))) % 1000)
    cases = [np.zeros(0, np.int64), np.zeros(7, np.int64), np.array([5, -1, 2]), np.array([0, 0, 3, 0, 0]),
             np.array([ref.INT32_MIN, 0x7fffffff, 0, -1], np.int64)]
    cases += [_random(rng, int(n)) for n in rng.integers(1, 300, 12)]
    for x in cases:
        if mag >= 0 and np.abs(x).max(initial=0) > 1000:
            x = x.copy()
            x[np.abs(x) > 1000] = 7          # keep the bit-by-bit writer's unary Rice runs short
        a = ref.encode(x, rl, mag, flag)
        assert ref.encode_np(x, rl, mag, flag) == a
        if (rl, mag, flag) == (-1, -1, False):
            assert ref.gamma_encode(x) == a
        want = x.copy()
        if mag < 0:
            want[want == ref.INT32_MIN] = -0x7fffffff
        assert ref.decode(a, x.size, rl, mag, flag).tolist() == want.tolist()


def test_decode_error_texts():
    code = ref.encode([3, 0, -2, 0, 0])
    with pytest.raises(ValueError, match=re.escape(ref.OUT_OF_BITS)):
        ref.decode(code[:1], 5)
    with pytest.raises(ValueError, match=re.escape(ref.PAST_END)):
        ref.decode(code, 4)
    with pytest.raises(ValueError, match=re.escape(ref.OUT_OF_BITS)):
        ref.decode(b"", 1)
    assert ref.decode(b"", 0).size == 0
    w = ref.BitWriter()
    w.write_bits(31, 0)
    w.write_bits(1, 1)
    w.write_bits(40, 0)
    with pytest.raises(ValueError, match=re.escape(ref.GAMMA_WIDTH)):
        ref.decode(w.data(), 3)
    w = ref.BitWriter()
    w.write_bits(40, 0)                     # a prefix that reaches the end: out of bits first
    with pytest.raises(ValueError, match=re.escape(ref.OUT_OF_BITS)):
        ref.decode(w.data(), 3)
    # trailing bits after a complete parse are ignored
    assert ref.decode(code + b"\xff\x00", 5).tolist() == [3, 0, -2, 0, 0]


def test_model_validation():
    import compression_amd as tfc
    with pytest.raises(ValueError, match="`coding_rank` must be at least 0."):
        tfc.PowerLawEntropyModel(coding_rank=-1)
    with pytest.raises(ValueError, match="`alpha` must be greater than 0."):
        tfc.PowerLawEntropyModel(coding_rank=1, alpha=0)
    with pytest.raises(ValueError, match="`coding_rank` must be at least 0."):
        tfc.LaplaceEntropyModel(coding_rank=-1)
    with pytest.raises(ValueError, match="`l1` must be greater than 0."):
        tfc.LaplaceEntropyModel(coding_rank=1, l1=-1.0)
    with pytest.raises(ValueError, match="at most 31"):
        tfc.LaplaceEntropyModel(coding_rank=1, magnitude_code=32)
    import torch
    m = tfc.PowerLawEntropyModel(coding_rank=2)
    assert (m.coding_rank, m.alpha, m.bottleneck_dtype) == (2, 1e-2, torch.get_default_dtype())
    m = tfc.LaplaceEntropyModel(coding_rank=1, bottleneck_dtype=torch.bfloat16)
    assert (m.l1, m.run_length_code, m.magnitude_code, m.use_run_length_for_non_zeros) == (0.01, -1, 0, False)
    assert m.bottleneck_dtype == torch.bfloat16
    # penalty and quantize are plain torch: they run on the CPU
    x = torch.tensor([[-2.4, 0.0, 1.6]], requires_grad=True)
    p = tfc.PowerLawEntropyModel(coding_rank=1).penalty(x)
    assert p.shape == (1,) and float(p.detach()) > 0
    q = tfc.LaplaceEntropyModel(coding_rank=1).quantize(x)
    assert q.tolist() == [[-2.0, 0.0, 2.0]]
    for name in ("run_length_gamma_encode", "run_length_gamma_decode", "run_length_encode", "run_length_decode"):
        assert name in tfc.gen_ops.__all__ and callable(getattr(tfc, name))


def test_run_length_entries_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "tfc_hip.h")).read()
    for needle in ("run_length_kernels.cc", "run_length_gamma_kernels.cc", "bit_coder.cc"):
        assert needle in text
    from compression_amd import _lib
    lib = _lib.lib()
    names = ["tfc_run_length_workspace", "tfc_run_length_encode_size", "tfc_run_length_encode_write",
             "tfc_run_length_decode"]
    for name in names:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.tfc_abi_version() == 2


def test_rice_parameter_above_31_is_rejected_on_the_host():
    from compression_amd import _lib
    lib = _lib.lib()
    total = ctypes.c_int64()
    rc = lib.tfc_run_length_encode_size(None, 0, 1, 4, 32, 0, 0, None, None, ctypes.byref(total), None)
    assert rc != 0 and "at most 31" in _lib.last_error()
    rc = lib.tfc_run_length_decode(None, None, None, 1, 4, 0, 40, 0, 0, None, None, None)
    assert rc != 0 and "at most 31" in _lib.last_error()

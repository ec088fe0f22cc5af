"""GPU tier of the run-length gamma / Rice codec: bytes equal to the restatements of tests/run_length_ref.py,
round trips through both decoder families, error strings in a batch, fused quantise / dequantise."""
import os
import re
from contextlib import contextmanager

import numpy as np
import pytest
import torch

import run_length_ref as ref

pytestmark = pytest.mark.gpu
COMBOS = [(rl, mag, flag) for rl in (-1, 0, 2, 3) for mag in (-1, 0, 4, 5) for flag in (False, True)]
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _laplace(rng, shape, zeros=0.7, scale=6.0):
    x = np.round(rng.laplace(0, scale, shape)).astype(np.int64)
    x[rng.random(shape) < zeros] = 0
    return x.astype(np.int32)


def _cases(rng, mag):
    """[units, L] int32 arrays over the data axes."""
    big = 100000 if mag == 0 else 5000
    out = [np.zeros((3, 50), np.int32), (rng.integers(1, 9, (4, 33)) * rng.choice([-1, 1], (4, 33))).astype(np.int32),
           np.zeros((1, 0), np.int32), _laplace(rng, (5, 1)), _laplace(rng, (7, 1237))]
    lead = np.zeros((2, 3000), np.int32)         # zero runs spanning several 1024-symbol encoder tiles
    lead[:, 2500] = [4, -9]
    lead[0, 17] = 1
    out.append(lead)
    ext = np.zeros((2, 9), np.int32)
    ext[0, [0, 3, 8]] = [I32_MIN, I32_MAX, -1]
    ext[1, [1, 2]] = [I32_MAX, I32_MIN]
    if mag < 0:
        out.append(ext)                          # under a Rice magnitude code these are 2^26..2^31 bits each
    wide = _laplace(rng, (3, 600))
    wide[:, ::97] = big                          # Rice-0 unary runs of 10^5 bits, wider than a chunk
    out.append(wide)
    return out


def _ref_bytes(x, rl, mag, flag):
    return [ref.encode_np(row, rl, mag, flag) for row in x]


def _expect(x, mag):
    y = x.astype(np.int64).copy()
    if mag < 0:
        y[y == I32_MIN] = -I32_MAX
    return y


@pytest.mark.parametrize("rl,mag,flag", COMBOS)
def test_bytes_and_round_trip(rl, mag, flag):
    import compression_amd as tfc
    rng = np.random.default_rng((rl + 1) * 100 + (mag + 1) * 3 + flag + 7)
    for x in _cases(rng, mag):
        got = tfc.run_length_encode_batched(torch.from_numpy(x), rl, mag, flag)
        assert list(got) == _ref_bytes(x, rl, mag, flag), (x.shape,)
        for fam in ("lane", "chunk"):
            with env(TFC_RL_DECODER=fam, TFC_RL_CHUNK_BITS=64):
                dec = tfc.run_length_decode_batched(got, [x.shape[1]], rl, mag, flag)
            assert (dec.cpu().numpy().astype(np.int64) == _expect(x, mag)).all(), (fam, x.shape)


def test_gamma_op_equals_run_length_encode():
    import compression_amd as tfc
    rng = np.random.default_rng(3)
    for x in (_laplace(rng, 5000), np.array([-6, 3, 0, 0], np.int32), np.zeros(9, np.int32),
              np.array([I32_MIN, 0, I32_MAX], np.int32)):
        t = torch.from_numpy(x).cuda()
        a = tfc.run_length_gamma_encode(t)
        assert a == tfc.run_length_encode(t, -1, -1, False) == ref.gamma_encode(x)
        back = tfc.run_length_gamma_decode(a, torch.tensor(x.shape, dtype=torch.int32))
        assert (back.cpu().numpy().astype(np.int64) == _expect(x, -1)).all()
    assert tfc.run_length_gamma_encode(torch.zeros(0, dtype=torch.int32)) == b""
    assert tfc.run_length_gamma_encode(torch.tensor([-6, 3, 0, 0], dtype=torch.int32)) == bytes([0xD1, 0x6D])
    assert tfc.run_length_gamma_decode(bytes([0xD1, 0x6D]), [4]).tolist() == [-6, 3, 0, 0]
    with pytest.raises(ValueError, match=re.escape("Invalid `code` shape: [2]")):
        tfc.run_length_gamma_decode(np.array([b"a", b"b"], dtype=object), [4])
    with pytest.raises(ValueError, match=re.escape("Invalid `shape` shape: [1, 1]")):
        tfc.run_length_decode(b"", torch.zeros(1, 1, dtype=torch.int32), -1, 0, False)


@pytest.mark.parametrize("flag", [False, True])
def test_long_strings_families_agree(flag):
    import compression_amd as tfc
    rng = np.random.default_rng(11 + flag)
    x = _laplace(rng, (2, 1 << 20))
    x[0, 1000:300000] = 0
    x[1, ::50000] = 100000
    for rl, mag in ((-1, -1), (2, 0), (0, 4)):
        got = tfc.run_length_encode_batched(torch.from_numpy(x).cuda(), rl, mag, flag)
        assert list(got) == _ref_bytes(x, rl, mag, flag)
        outs = []
        for kv in ({}, {"TFC_RL_DECODER": "chunk", "TFC_RL_CHUNK_BITS": 8}, {"TFC_RL_DECODER": "lane"},
                   {"TFC_RL_DECODER": "chunk", "TFC_RL_SYNC_ROUNDS": 0}):
            with env(**kv):
                outs.append(tfc.run_length_decode_batched(got, [x.shape[1]], rl, mag, flag).cpu().numpy())
        for o in outs:
            assert (o == x).all()


def test_many_units():
    import compression_amd as tfc
    rng = np.random.default_rng(5)
    for units, L in ((1, 7), (200003, 3), (196608, 192 // 16)):
        x = _laplace(rng, (units, L))
        blob, offsets, shape = tfc.run_length_encode_batched(torch.from_numpy(x).cuda(), -1, 0, False,
                                                             device_result=True)
        strings = tfc.gen_ops.strings_from_blob(blob, offsets, shape)
        for i in rng.integers(0, units, 50):
            assert strings[i] == ref.encode_np(x[i], -1, 0, False)
        for fam in ("lane", "chunk"):
            with env(TFC_RL_DECODER=fam):
                dec = tfc.run_length_decode_batched((blob, offsets, shape), [L], -1, 0, False)
            assert (dec.cpu().numpy() == x).all(), fam


def test_error_strings_in_a_batch():
    import compression_amd as tfc
    good = ref.encode([3, 0, -2, 0, 0])
    w = ref.BitWriter()
    w.write_bits(31, 0)
    w.write_bits(1, 1)
    w.write_bits(40, 0)
    gamma31 = w.data()
    bad = {"Out of bits to read.": good[:1], "Decoded past end of tensor.": ref.encode([3, 0, -2, 0, 0, 0]),
           "Exceeded maximum gamma bit width.": gamma31}
    for fam in ("lane", "chunk"):
        with env(TFC_RL_DECODER=fam, TFC_RL_CHUNK_BITS=8):
            ok = tfc.run_length_decode_batched([good, good + b"\xff"], [5])
            assert ok.tolist() == [[3, 0, -2, 0, 0]] * 2
            for text, s in bad.items():
                with pytest.raises(ValueError, match=re.escape(text)):
                    tfc.run_length_decode_batched([good, s, good], [5])
            with pytest.raises(ValueError, match=re.escape("Out of bits to read.")):
                tfc.run_length_decode_batched([good, b""], [5])
            assert tfc.run_length_decode_batched([b"", b""], [0]).shape == (2, 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_fused_quantise_and_dequantise(dtype):
    import compression_amd as tfc
    g = torch.Generator().manual_seed(0)
    x = (torch.randn(6, 3001, generator=g) * 4).to(dtype)
    x[0, :5] = torch.tensor([0.5, 1.5, 2.5, -0.5, -2.5]).to(dtype)      # ties to even
    want = tfc.run_length_encode_batched(torch.round(x).int(), 2, 1, True)
    got = tfc.run_length_encode_batched(x.cuda(), 2, 1, True)
    assert list(got) == list(want)
    for out in (torch.float32, torch.bfloat16):
        dec = tfc.run_length_decode_batched(got, [3001], 2, 1, True, dtype=out)
        assert dec.dtype == out and torch.equal(dec.cpu(), torch.round(x).int().to(out))

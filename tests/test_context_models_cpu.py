"""CPU tier of what the two context models share: the checkpoint layout of both models against a recorded fixture, the
state a CheckerboardConv2D forward leaves behind, and the decoder's two stream-format rules of csrc/range_wave.h,
compiled for the host, against the RowDecoder of tests/context_ref.py."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import context_ref
from compression_amd.layers import CheckerboardConv2D, MaskedConv2D
from compression_amd.models import Checkerboard2021Model, MBT2018Model
from compression_amd.ops import checkerboard_ops, context_ops
from test_context_cpu import NUM_SCALES, _tables

HERE = os.path.dirname(os.path.abspath(__file__))


def test_state_dict_names_and_shapes_are_the_recorded_ones():
    """tests/golden/context_model_state_dicts.json was written before the two models got their common base class."""
    with open(os.path.join(HERE, "golden", "context_model_state_dicts.json")) as f:
        want = json.load(f)
    models = {"mbt2018_context": MBT2018Model(num_filters=8, latent_depth=8),
              "mbt2018_mean": MBT2018Model(num_filters=8, latent_depth=8, context=False),
              "checkerboard2021": Checkerboard2021Model(num_filters=8, latent_depth=8)}
    assert sorted(want) == sorted(models)
    for name, model in models.items():
        got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
        assert got == want[name], name
    assert len(want["mbt2018_context"]) == len(want["checkerboard2021"]) == 54


def test_checkerboard_conv_forward_leaves_the_layer_as_it_was():
    torch.manual_seed(0)
    layer = CheckerboardConv2D(8, 4).double()
    # whole numbers: every sum below is exact in float64, whatever order a convolution adds its taps in
    with torch.no_grad():
        layer.kernel_variable.copy_(torch.randint(-4, 5, layer.kernel_variable.shape))      # the masked taps too
        layer.bias.copy_(torch.randint(-4, 5, layer.bias.shape))
    x = torch.randint(-4, 5, (1, 3, 4, 4)).double()
    out = layer(x)
    assert layer.use_bias is True
    assert "mask" not in layer.state_dict()
    assert torch.equal(layer.mask, checkerboard_ops.CheckerboardParams.mask())
    assert torch.equal(MaskedConv2D(8, 4).mask, context_ops.ContextParams.mask())
    assert CheckerboardConv2D.TAPS is checkerboard_ops.CHECKER_TAPS and MaskedConv2D.TAPS is context_ops.CAUSAL_TAPS
    taps = context_ops.tap_sum(torch.zeros(1, 3, 4, 8, dtype=torch.float64), x, layer.kernel_variable.detach(),
                               checkerboard_ops.CHECKER_TAPS)
    others = (~checkerboard_ops.anchor_mask(3, 4)).double()[None, :, :, None]
    assert torch.equal(out.detach(), layer.bias.detach() + taps * others)
    assert taps.abs().sum() > 0 and not torch.equal(out.detach(), layer.bias.detach() + taps)


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("native") / "decoder_rules_check.so")
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--offload-host-only", "-std=c++17",
                    "-O2", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "native", "decoder_rules_check.cc")],
                   check=True)
    lib = C.CDLL(so)
    lib.decoder_finalize_ok.restype = C.c_int
    lib.decoder_finalize_ok.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_uint, C.c_longlong]
    lib.decoder_open_state.restype = None
    lib.decoder_open_state.argtypes = [C.c_char_p, C.c_longlong, C.POINTER(C.c_uint * 4)]
    return lib


def test_decoder_rules_agree_with_the_row_decoder(rules, monkeypatch):
    """dec_finalize_ok on the states the decode loop of test_context_cpu ends in, intact strings and one with four
    bytes appended, and dec_open_state on those strings and on ones shorter than the window."""
    seen = []
    ok = context_ref.RowDecoder.ok

    def recording(self):
        verdict = ok(self)
        seen.append(((self.base, self.span_m1, self.window, self.pulls, len(self.data)), verdict))
        return verdict

    monkeypatch.setattr(context_ref.RowDecoder, "ok", recording)
    y, psi, weights = context_ref.make_case((2, 3, 2, 4, 9, 6), NUM_SCALES)
    want = context_ref.context_scan(y, psi, weights, NUM_SCALES)
    port, lookup, rows, cdf_offset = _tables()
    b, hl, wl, m = y.shape
    idx = want["idx"].reshape(b * hl, wl * m)
    value = want["sym"].reshape(b * hl, wl * m) - cdf_offset[idx]
    strings, _, _ = port.encode(lookup, value.astype(np.int32), index=idx.astype(np.int32))
    nested = [strings[n * hl:(n + 1) * hl] for n in range(b)]
    _, intact = context_ref.context_decode(nested, psi, weights, NUM_SCALES, rows, cdf_offset)
    longer = [list(per) for per in nested]
    longer[0][0] = longer[0][0] + b"\x12\x34\x56\x78"
    _, surplus = context_ref.context_decode(longer, psi, weights, NUM_SCALES, rows, cdf_offset)
    assert intact.all() and not surplus[0, 0] and surplus.reshape(-1)[1:].all()
    assert len(seen) == 2 * b * hl and sum(not verdict for _, verdict in seen) == 1
    for state, verdict in seen:
        assert bool(rules.decoder_finalize_ok(*state)) == verdict, state
    for data in [bytes(s) for s in strings] + [b"", b"\xab", b"\xab\xcd\xef"]:
        out = (C.c_uint * 4)()
        rules.decoder_open_state(data, len(data), C.byref(out))
        fresh = context_ref.RowDecoder(data)
        assert tuple(out) == (fresh.base, fresh.span_m1, fresh.window, fresh.pulls), data

"""CPU tier: the geometry of KerasConv2D / KerasConv2DTranspose (`padding="same"`).  The two convolution kernels are
replaced by float64 statements of what they compute (tests/keras_conv_emulation.py), and the layers' pad / crop /
channel-padding logic is checked against torch.nn.functional.conv2d / conv_transpose2d in float64 with the explicit
asymmetric TF "SAME" padding and crop."""
import numpy as np
import pytest
import torch

import keras_conv_emulation
from compression_amd.layers import KerasConv2D, KerasConv2DTranspose
from compression_amd.layers.keras_conv import same_before


@pytest.fixture
def emulated(monkeypatch):
    keras_conv_emulation.install(monkeypatch)


def want_conv(x, kernel, bias, k, s):
    """TF SAME: out = ceil(L / s), total = max((out - 1) s + k - L, 0), before = total // 2, the rest behind."""
    pads = []
    for length in (x.shape[2], x.shape[1]):
        out = -(-length // s)
        total = max((out - 1) * s + k - length, 0)
        pads += [total // 2, total - total // 2]
    xp = torch.nn.functional.pad(x.permute(0, 3, 1, 2).double(), pads)
    y = torch.nn.functional.conv2d(xp, kernel.permute(3, 2, 0, 1).double(), bias.double(), stride=s)
    return y.permute(0, 2, 3, 1)


def want_transpose(x, kernel, bias, k, s):
    """The gradient of the SAME convolution that maps L s to L: the full convolution from offset max(k - s, 0) // 2."""
    f = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2).double(), kernel.permute(3, 2, 0, 1).double(), stride=s)
    f = torch.nn.functional.pad(f, (0, s, 0, s))
    b = max(k - s, 0) // 2
    y = f[:, :, b:b + x.shape[1] * s, b:b + x.shape[2] * s] + bias.double()[None, :, None, None]
    return y.permute(0, 2, 3, 1)


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("size", [(8, 6), (9, 7), (8, 5)])
@pytest.mark.parametrize("cin,cout", [(3, 60), (60, 220), (220, 3)])
def test_conv2d_same(emulated, k, s, size, cin, cout):
    torch.manual_seed(k * 10 + s)
    x = torch.randn((2,) + size + (cin,), dtype=torch.float64)
    layer = KerasConv2D(cout, k, strides=s, in_channels=cin).double()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(cout))
        y = layer(x)
    want = want_conv(x, layer.kernel, layer.bias, k, s)
    assert tuple(y.shape) == (2, -(-size[0] // s), -(-size[1] // s), cout) == tuple(want.shape)
    assert tuple(layer.kernel.shape) == (k, k, cin, cout)
    assert (y - want).abs().max() <= 1e-10


@pytest.mark.parametrize("k", [3, 7])
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("size", [(4, 6), (5, 3)])
@pytest.mark.parametrize("cin,cout", [(3, 60), (60, 220), (220, 3)])
def test_conv2d_transpose_same(emulated, k, s, size, cin, cout):
    torch.manual_seed(k * 10 + s)
    x = torch.randn((2,) + size + (cin,), dtype=torch.float64)
    layer = KerasConv2DTranspose(cout, k, strides=s, in_channels=cin).double()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(cout))
        y = layer(x)
    want = want_transpose(x, layer.kernel, layer.bias, k, s)
    assert tuple(y.shape) == (2, size[0] * s, size[1] * s, cout) == tuple(want.shape)
    assert tuple(layer.kernel.shape) == (k, k, cout, cin)
    assert (y - want).abs().max() <= 1e-10


def test_stride_two_differs_from_same_zeros(emulated):
    """k = 3, s = 2, even L: Keras starts its windows at x[0] (before = 0), `same_zeros` at x[-1] (k // 2 = 1)."""
    assert same_before(8, 3, 2) == (4, 0) and same_before(9, 3, 2) == (5, 1) and same_before(8, 7, 1) == (8, 3)
    x = torch.arange(8, dtype=torch.float64).reshape(1, 8, 1, 1).expand(1, 8, 8, 1).contiguous()
    layer = KerasConv2D(1, 3, strides=2, in_channels=1).double()
    with torch.no_grad():
        layer.kernel.zero_()
        layer.kernel[0, 1, 0, 0] = 1.0                           # picks x[2 i + 0 - before] along H
        y = layer(x)
    assert y[0, :, 0, 0].tolist() == [0.0, 2.0, 4.0, 6.0]
    assert keras_conv_emulation.emu_down(x, layer.kernel.detach(), None, 2)[0, :, 0, 0].tolist() == [0.0, 1.0, 3.0, 5.0]


def test_gradients_flow_through_the_padding(emulated):
    x = torch.randn(1, 6, 6, 60, dtype=torch.float64, requires_grad=True)
    layer = KerasConv2D(60, 3, strides=2, in_channels=60).double()
    layer(x).sum().backward()
    assert x.grad is not None and layer.kernel.grad.shape == layer.kernel.shape and layer.bias.grad.shape == (60,)

"""GPU tier: KerasConv2D / KerasConv2DTranspose on the MFMA convolution kernels against float64 torch, for HiFiC's layer
shapes (models/hific/archs.py:86-103, 130-161) at a small spatial size."""
import numpy as np
import pytest
import torch

from compression_amd.layers import KerasConv2D, KerasConv2DTranspose
from test_keras_conv_cpu import want_conv, want_transpose

pytestmark = pytest.mark.gpu

# (class, k, s, cin, cout): every layer shape of the encoder and the generator
LAYERS = [(KerasConv2D, 7, 1, 3, 60), (KerasConv2D, 3, 2, 60, 120), (KerasConv2D, 3, 2, 120, 240),
          (KerasConv2D, 3, 2, 240, 480), (KerasConv2D, 3, 2, 480, 960), (KerasConv2D, 3, 1, 960, 220),
          (KerasConv2D, 3, 1, 220, 960), (KerasConv2D, 3, 1, 960, 960), (KerasConv2DTranspose, 3, 2, 960, 480),
          (KerasConv2DTranspose, 3, 2, 480, 240), (KerasConv2DTranspose, 3, 2, 240, 120),
          (KerasConv2DTranspose, 3, 2, 120, 60), (KerasConv2D, 7, 1, 60, 3)]


@pytest.mark.parametrize("cls,k,s,cin,cout", LAYERS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("size", [(8, 6), (9, 7)])
def test_layer_against_float64(cls, k, s, cin, cout, dtype, size):
    """Bars of tests/test_signal_conv_gpu.py for the same dtype: float32 2e-5 max(1, max |want|) (line 57), bfloat16
    2**-7 max(1, max |want|) (line 132), the reference taken on the inputs and weights as the kernels see them
    (bfloat16-rounded for bfloat16)."""
    torch.manual_seed(k + s + cin)
    layer = cls(cout, k, strides=s, in_channels=cin).cuda()
    with torch.no_grad():
        layer.bias.copy_(torch.randn(cout))
    x = torch.randn((2,) + size + (cin,), device="cuda").to(dtype)
    with torch.no_grad():
        y = layer(x)
    want_fn = want_transpose if cls is KerasConv2DTranspose else want_conv
    kernel = layer.kernel.detach().to(dtype).float().cpu()
    want = want_fn(x.float().cpu(), kernel, layer.bias.detach().cpu(), k, s)
    assert tuple(y.shape) == tuple(want.shape) and y.dtype == dtype
    assert s != 1 or y.is_contiguous()         # stride 1 under no_grad: `filters` channels straight from the kernel, no slice
    err = (y.double().cpu() - want).abs().max().item()
    bound = (2e-5 if dtype == torch.float32 else 2 ** -7) * max(1.0, want.abs().max().item())
    print(f"keras {cls.__name__} k={k} s={s} {cin}->{cout} {dtype} {size}: max err = {err:.3e}, bar = {bound:.3e}")
    assert err <= bound


def test_gradients_against_float64():
    torch.manual_seed(1)
    for cls, k, s, cin, cout in [(KerasConv2D, 3, 2, 60, 120), (KerasConv2DTranspose, 3, 2, 120, 60),
                                 (KerasConv2D, 7, 1, 3, 60)]:
        layer = cls(cout, k, strides=s, in_channels=cin).cuda()
        x = torch.randn(2, 8, 6, cin, device="cuda", requires_grad=True)
        y = layer(x)
        w = torch.randn_like(y)
        (y * w).sum().backward()
        xd = x.detach().cpu().double().requires_grad_()
        kd = layer.kernel.detach().cpu().double().requires_grad_()
        bd = layer.bias.detach().cpu().double().requires_grad_()
        want = (want_transpose if cls is KerasConv2DTranspose else want_conv)(xd, kd, bd, k, s)
        (want * w.cpu().double()).sum().backward()
        for got, ref, name in ((x.grad, xd.grad, "dx"), (layer.kernel.grad, kd.grad, "dw"), (layer.bias.grad, bd.grad, "db")):
            err = (got.cpu().double() - ref).abs().max().item()
            assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (cls.__name__, name, err)


def test_padded_weights_are_kept_and_follow_the_weights():
    layer = KerasConv2D(60, 3, in_channels=60).cuda()
    x = torch.randn(1, 8, 8, 60, device="cuda")
    with torch.no_grad():
        a = layer(x)
        hit = layer.__dict__["_padded_cache"]
        assert torch.equal(layer(x), a) and layer.__dict__["_padded_cache"] is hit
        layer.kernel.mul_(2.0)                                     # an autograd-visible write: new version, new padding
        layer.bias.zero_()
        b = layer(x)
    assert layer.__dict__["_padded_cache"] is not hit
    assert (b - 2 * a).abs().max() <= 1e-4

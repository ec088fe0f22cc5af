"""GPU tier: SignalConv1D / SignalConv3D on the rank-3 kernels — the reference's rank-1 and rank-3 cases
(tests/signal_conv_nd_cases.py) against its SciPy oracle, gradients to every parameter, and a small 3-D autoencoder
that trains."""
import numpy as np
import pytest
import torch

import signal_conv_nd_cases as cases
from test_signal_conv_nd_cpu import layer_class

pytestmark = pytest.mark.gpu


def run_layer(kernel, x_ncs, dtype, **kw):
    layer = layer_class(x_ncs.ndim - 2)(kernel.shape[-1], kw.pop("kernel_support"),
                                        kernel_parameter=torch.from_numpy(kernel).cuda(), **kw)
    with torch.no_grad():
        y = layer(torch.from_numpy(np.ascontiguousarray(np.moveaxis(x_ncs, 1, -1))).cuda().to(dtype))
    return np.moveaxis(y.float().cpu().numpy(), -1, 1)


@pytest.mark.parametrize("case", [c for c in cases.valid_cases()
                                  if cases.is_implemented(c["input_support"], c["kernel_support"], c["corr"],
                                                          c["strides_up"], c["channel_separable"], c["filters"])],
                         ids=cases.case_id)
def test_valid_against_scipy(case):
    case = dict(case)
    rng = np.random.default_rng(1)
    support, channels, filters = case.pop("input_support"), case.pop("channels"), case.pop("filters")
    x = rng.integers(0, 32, (1, channels) + support).astype(np.float32)
    kernel = rng.integers(0, 16, case["kernel_support"] + (channels, filters)).astype(np.float32)
    want = cases.scipy_convolve_valid(case["corr"], x, kernel, case["strides_down"], case["strides_up"],
                                      case["extra_pad_end"], case["channel_separable"])
    got = run_layer(kernel, x, torch.float32, padding="valid",
                    activation=(lambda t: t) if case["use_bias"] else None, **case)
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=0, atol=1e-3)


@pytest.mark.parametrize("case", [c for c in cases.same_cases()
                                  if cases.is_implemented(c["input_support"], c["kernel_support"], c["corr"],
                                                          c["strides_up"], False, 1)], ids=cases.case_id)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_same_identity_kernels(case, dtype):
    case = dict(case)
    support = case.pop("input_support")
    x = np.arange(np.prod(support), dtype=np.float32).reshape((1, 1) + support)
    got = run_layer(cases.identity_kernel(case["kernel_support"]), x, dtype, **case)
    want = x
    if not all(s == 1 for s in case["strides_up"]):
        want = cases.numpy_upsample(want, case["strides_up"], case["extra_pad_end"])
    want = want[(slice(None), slice(None)) + tuple(slice(None, None, s) for s in case["strides_down"])]
    assert got.shape == want.shape
    assert np.allclose(got, want, rtol=0, atol=1e-3)       # (integers below 256: exact in bfloat16 too)


def test_gradients_reach_every_parameter():
    from compression_amd import layers
    torch.manual_seed(0)
    l1 = layers.SignalConv1D(16, 5, corr=True, strides_down=2, padding="same_zeros", use_bias=True).cuda()
    l3 = layers.SignalConv3D(16, (3, 3, 3), corr=False, strides_up=(1, 2, 2), padding="same_zeros",
                             kernel_parameter="variable", use_bias=True, activation=torch.relu).cuda()
    y1 = l1(torch.randn(2, 20, 8, device="cuda"))
    y3 = l3(torch.randn(2, 3, 4, 5, 16, device="cuda"))
    (y1.square().sum() + y3.square().sum()).backward()
    for p in (l1.kernel_real, l1.kernel_imag, l1.bias, l3.kernel_variable, l3.bias):
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0
    # and their values, against the float64 definition (tests/signal_conv_oracle.py) on integer inputs and cotangents:
    # the rdft layer at its random kernel, the ReLU layer at integer weights (everything exact)
    from test_signal_conv_grad_gpu import check_module, integers
    check_module(l1, integers((2, 20, 8), 0, 7, 1))
    with torch.no_grad():
        l3.kernel_variable.copy_(integers(l3.kernel_variable.shape, -3, 3, 2))
        l3.bias.copy_(integers(l3.bias.shape, -20, 20, 3))
    check_module(l3, integers((2, 3, 4, 5, 16), 0, 7, 4))


def test_small_3d_autoencoder_trains():
    from compression_amd import layers
    torch.manual_seed(0)
    model = torch.nn.Sequential(
        layers.SignalConv3D(32, (3, 5, 5), corr=True, strides_down=(1, 2, 2), padding="same_zeros", use_bias=True,
                            activation=layers.GDN()),
        layers.SignalConv3D(32, (3, 5, 5), corr=False, strides_up=(1, 2, 2), padding="same_zeros", use_bias=True,
                            activation=layers.GDN(inverse=True))).cuda()
    x = torch.rand(2, 4, 16, 16, 32, device="cuda")        # (the GDN kernels take multiples of 32 channels)
    model(x)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = (model(x) - x).square().mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert losses[-1] < 0.8 * losses[0], losses

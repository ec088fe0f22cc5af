"""CPU tier: SignalConv1D / SignalConv3D for every rank-1 and rank-3 configuration of the reference's own test
(python/layers/signal_conv_test.py:388-502, 620-735) against that test's SciPy oracle, in both data formats.  The two
rank-3 kernels are replaced by torch-CPU float64 statements of what they compute (include/tfc_hip.h; pinned to torch
on the GPU by tests/test_conv3d_gpu.py), per axis:
    down_s(x)[i] = sum_t x[i s + t - k // 2] w[t]                i < ceil(len / s), zeros outside x
    up_s(x)[n]   = sum_j w[j] u[n + k // 2 - j]                  n < len s, u = x with s - 1 zeros behind every sample
so that the layers' host logic is checked without a device."""
import numpy as np
import pytest
import torch

import signal_conv_nd_cases as cases


def _epilogue(y, bias, activation):
    if bias is not None:
        y = y + bias.double()
    return torch.relu(y) if activation == "relu" else y


def emu_down(x, kernel, bias=None, strides=1, activation=None):
    s = (strides,) * 3 if isinstance(strides, int) else tuple(strides)
    k = kernel.shape[:3]
    out = [-(-x.shape[1 + a] // s[a]) for a in range(3)]
    pad = []
    for a in (2, 1, 0):
        pad += [k[a] // 2, k[a] + s[a]]
    xp = torch.nn.functional.pad(x.permute(0, 4, 1, 2, 3).double(), pad)
    y = torch.nn.functional.conv3d(xp, kernel.permute(4, 3, 0, 1, 2).double().contiguous(), stride=s)[:, :, :out[0], :out[1], :out[2]]
    return _epilogue(y.permute(0, 2, 3, 4, 1), bias, activation).to(x.dtype).contiguous()


def emu_up(x, kernel, bias=None, strides=1, activation=None):
    s = (strides,) * 3 if isinstance(strides, int) else tuple(strides)
    k = kernel.shape[:3]
    # conv_transpose3d = the full convolution of the zero-upsampled input: f[m] = sum_q x[q] w[m - q s]
    f = torch.nn.functional.conv_transpose3d(x.permute(0, 4, 1, 2, 3).double(), kernel.permute(3, 4, 0, 1, 2).double().contiguous(),
                                             stride=s)
    f = torch.nn.functional.pad(f, (0, s[2] + k[2], 0, s[1] + k[1], 0, s[0] + k[0]))
    sl = [slice(k[a] // 2, k[a] // 2 + x.shape[1 + a] * s[a]) for a in range(3)]
    y = f[:, :, sl[0], sl[1], sl[2]]
    return _epilogue(y.permute(0, 2, 3, 4, 1), bias, activation).to(x.dtype).contiguous()


@pytest.fixture
def emulated(monkeypatch):
    from compression_amd.layers import functional
    monkeypatch.setattr(functional, "conv3d_down", emu_down)
    monkeypatch.setattr(functional, "conv3d_up", emu_up)


def layer_class(rank):
    from compression_amd import layers
    return {1: layers.SignalConv1D, 3: layers.SignalConv3D}[rank]


def run_layer(kernel, x_ncs, data_format, **kw):
    cls = layer_class(x_ncs.ndim - 2)
    layer = cls(kernel.shape[-1], kw.pop("kernel_support"), kernel_parameter=torch.from_numpy(kernel),
                data_format=data_format, **kw)
    x = x_ncs if data_format == "channels_first" else np.moveaxis(x_ncs, 1, -1)
    with torch.no_grad():
        y = layer(torch.from_numpy(np.ascontiguousarray(x))).numpy()
    return y if data_format == "channels_first" else np.moveaxis(y, -1, 1)


def test_emulations_state_the_kernels():
    """The emulations against the definitions, summed term by term on a small rank-3 case with unequal strides."""
    rng = np.random.default_rng(0)
    x = rng.integers(-4, 5, (1, 3, 4, 5, 2)).astype(np.float64)
    w = rng.integers(-3, 4, (3, 2, 3, 2, 1)).astype(np.float64)
    s = (2, 1, 3)
    got = emu_down(torch.from_numpy(x), torch.from_numpy(w), None, s).numpy()
    up = emu_up(torch.from_numpy(x), torch.from_numpy(w), None, s).numpy()
    k = w.shape[:3]
    want = np.zeros(got.shape)
    want_up = np.zeros(up.shape)
    for i in np.ndindex(*got.shape[1:4]):
        for t in np.ndindex(*k):
            p = [i[a] * s[a] + t[a] - k[a] // 2 for a in range(3)]
            if all(0 <= p[a] < x.shape[1 + a] for a in range(3)):
                want[(0,) + i] += x[(0,) + tuple(p)] @ w[t]
    for q in np.ndindex(*x.shape[1:4]):
        for t in np.ndindex(*k):
            m = [q[a] * s[a] + t[a] - k[a] // 2 for a in range(3)]
            if all(0 <= m[a] < up.shape[1 + a] for a in range(3)):
                want_up[(0,) + tuple(m)] += x[(0,) + q] @ w[t]
    assert np.array_equal(got, want)
    assert np.array_equal(up, want_up)


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("case", list(cases.valid_cases()), ids=cases.case_id)
def test_valid_against_scipy(emulated, case, data_format):
    case = dict(case)
    rng = np.random.default_rng(1)
    support, channels, filters = case.pop("input_support"), case.pop("channels"), case.pop("filters")
    x = rng.integers(0, 32, (1, channels) + support).astype(np.float32)
    kernel = rng.integers(0, 16, case["kernel_support"] + (channels, filters)).astype(np.float32)
    if not cases.is_implemented(support, case["kernel_support"], case["corr"], case["strides_up"],
                                case["channel_separable"], filters):
        with pytest.raises(NotImplementedError, match="SignalConv"):
            layer_class(len(support))(filters, case["kernel_support"], corr=case["corr"],
                                      strides_down=case["strides_down"], strides_up=case["strides_up"],
                                      channel_separable=case["channel_separable"],
                                      kernel_parameter=torch.from_numpy(kernel))
        return
    want = cases.scipy_convolve_valid(case["corr"], x, kernel, case["strides_down"], case["strides_up"],
                                      case["extra_pad_end"], case["channel_separable"])
    got = run_layer(kernel, x, data_format, padding="valid",
                    activation=(lambda t: t) if case["use_bias"] else None, **case)
    assert got.shape == want.shape
    assert np.array_equal(got, want)            # small integers: every sum exact


@pytest.mark.parametrize("data_format", ["channels_last", "channels_first"])
@pytest.mark.parametrize("case", list(cases.same_cases()), ids=cases.case_id)
def test_same_identity_kernels(emulated, case, data_format):
    """signal_conv_test.py:262-315 `run_same`: with the identity kernel the layer returns its input, up- and downsampled."""
    case = dict(case)
    support = case.pop("input_support")
    x = np.arange(np.prod(support), dtype=np.float32).reshape((1, 1) + support)
    if not cases.is_implemented(support, case["kernel_support"], case["corr"], case["strides_up"], False, 1):
        with pytest.raises(NotImplementedError, match="SignalConv"):
            layer_class(len(support))(1, case["kernel_support"], corr=case["corr"], strides_up=case["strides_up"],
                                      strides_down=case["strides_down"], padding=case["padding"])
        return
    kernel = cases.identity_kernel(case["kernel_support"])
    got = run_layer(kernel, x, data_format, **case)
    want = x
    if not all(s == 1 for s in case["strides_up"]):
        want = cases.numpy_upsample(want, case["strides_up"], case["extra_pad_end"])
    want = want[(slice(None), slice(None)) + tuple(slice(None, None, s) for s in case["strides_down"])]
    assert got.shape == want.shape
    assert np.array_equal(got, want)


def test_rank_errors():
    from compression_amd import layers
    with pytest.raises(ValueError, match=r"Input tensor must have rank 3, received shape \(2, 3, 4, 5\)"):
        layers.SignalConv1D(2, 3)(torch.zeros(2, 3, 4, 5))
    with pytest.raises(ValueError, match=r"Input tensor must have rank 5, received shape \(2, 3, 4\)"):
        layers.SignalConv3D(2, 3)(torch.zeros(2, 3, 4))


def test_channel_separable_rank3_not_implemented():
    from compression_amd import layers
    with pytest.raises(NotImplementedError, match="SignalConv3D arguments is not currently implemented"):
        layers.SignalConv3D(1, 3, corr=True, channel_separable=True)
    layers.SignalConv1D(1, 3, corr=True, channel_separable=True)          # rank 1 has it


def test_extra_pad_end_default_follows_padding():
    """signal_conv.py:416-419: extra_pad_end=None means padding.startswith("same_")."""
    from compression_amd import layers
    for cls in (layers.SignalConv1D, layers.SignalConv3D):
        assert cls(1, 3).extra_pad_end is False
        assert cls(1, 3, padding="same_zeros").extra_pad_end is True
        assert cls(1, 3, padding="same_reflect").extra_pad_end is True
        assert cls(1, 3, padding="valid", extra_pad_end=True).extra_pad_end is True
    assert layers.SignalConv2D(1, 3).extra_pad_end is True                # SignalConv2D's default stays


def test_rdft_round_trip_rank3_and_rank5():
    from compression_amd import layers
    torch.manual_seed(0)
    for cls, shape in ((layers.SignalConv1D, (5, 3, 4)), (layers.SignalConv3D, (3, 4, 5, 2, 3))):
        k = torch.randn(shape)
        layer = cls(shape[-1], shape[:-2], kernel_initializer=lambda s, k=k: k.clone(), in_channels=shape[-2])
        assert layer.kernel_real is not None and layer.kernel_variable is None
        assert torch.allclose(layer.kernel, k, atol=1e-5)
        p = layers.RDFTParameter(k)
        assert torch.allclose(p(), k, atol=1e-5)
        assert torch.allclose(layer.kernel_real, p.real, atol=1e-6)


def test_default_initializer_fan_in():
    from compression_amd import layers
    torch.manual_seed(0)
    layer = layers.SignalConv3D(64, (3, 5, 5), kernel_parameter="variable", in_channels=32)
    std = float(layer.kernel.detach().std())
    assert abs(std - (1.0 / (75 * 32)) ** 0.5) < 0.1 * std


def test_default_arguments_construct_and_run(emulated):
    """`SignalConv1D(filters, k)` / `SignalConv3D(filters, k)`: padding="valid", convolution, rdft kernel."""
    from compression_amd import layers
    torch.manual_seed(0)
    for cls, shape in ((layers.SignalConv1D, (2, 9, 3)), (layers.SignalConv3D, (2, 5, 6, 7, 3))):
        layer = cls(4, 3)
        x = torch.randn(shape)
        with torch.no_grad():
            y = layer(x)
        want = cases.scipy_convolve_valid(False, np.moveaxis(x.numpy(), -1, 1), layer.kernel.detach().numpy(),
                                          (1,) * (x.dim() - 2), (1,) * (x.dim() - 2), True, False)
        assert np.allclose(np.moveaxis(y.numpy(), -1, 1), want, atol=1e-5)


def test_model_configuration_is_one_kernel_call(monkeypatch):
    """same_zeros + extra_pad_end + one-sided strides reach the kernel once, without pad or crop."""
    from compression_amd.layers import functional
    calls = []

    def spy(name, fn):
        def f(x, *a, **k):
            calls.append((name, tuple(x.shape)))
            return fn(x, *a, **k)
        return f
    monkeypatch.setattr(functional, "conv3d_down", spy("down", emu_down))
    monkeypatch.setattr(functional, "conv3d_up", spy("up", emu_up))
    monkeypatch.setattr(functional, "pad3d", lambda *a, **k: pytest.fail("padded"))
    from compression_amd import layers
    x = torch.randn(2, 4, 8, 8, 16)
    y = layers.SignalConv3D(32, (3, 5, 5), corr=True, strides_down=(1, 2, 2), padding="same_zeros",
                            use_bias=True, activation=torch.relu)(x)
    assert tuple(y.shape) == (2, 4, 4, 4, 32) and calls == [("down", (2, 4, 8, 8, 16))]
    calls.clear()
    y = layers.SignalConv1D(8, 9, strides_up=4, padding="same_zeros")(torch.randn(2, 10, 16))
    assert tuple(y.shape) == (2, 40, 8) and calls == [("up", (2, 1, 1, 10, 16))]

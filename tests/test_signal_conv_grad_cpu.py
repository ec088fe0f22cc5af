"""CPU tier: the training path of SignalConv1D / 2D / 3D — the grad-enabled forward, dx and dkernel — against the float64
definition of tests/signal_conv_oracle.py, exactly, on integer data.  The HIP kernels are replaced by the float64
emulations of the forward tests (tests/test_signal_conv_cpu.py, tests/test_signal_conv_nd_cpu.py), in two ways:
    "autograd":       functional.conv{2,3}d_{down,up} are the emulations and torch differentiates them — the layer's own
                      pad / crop / zero-insertion / channel padding as autograd nodes;
    "conv_function":  only the launchers under functional._ConvFunction are emulated (forward kernel, weight gradient
                      kernel, with the channel counts the rank-2 kernels reject rejected), so that _conv_dispatch,
                      _ConvFunction.backward and conv2d_wgrad's channel blocks run as on the device.
The oracle itself is pinned first: to SciPy, to the identity-kernel expectation and to `same_reflect_oracle`."""
import itertools

import numpy as np
import pytest
import torch

import signal_conv_cases as cases2
import signal_conv_nd_cases as cases_nd
import signal_conv_oracle as so
import test_signal_conv_cpu as emu2
import test_signal_conv_nd_cpu as emu3


# ---- the oracle against the forward tests' oracles -----------------------------------------------------------------------
def _oracle_nchw(x_ncs, kernel, **kw):
    y = so.layer_oracle(torch.from_numpy(x_ncs), torch.from_numpy(kernel), data_format="channels_first", **kw)
    return y.numpy()


@pytest.mark.parametrize("module", [cases2, cases_nd], ids=["rank2", "rank1and3"])
def test_oracle_equals_scipy_on_valid_cases(module):
    rng = np.random.default_rng(1)
    ran = 0
    for c in module.valid_cases():
        x = rng.integers(0, 32, (2, c["channels"]) + c["input_support"]).astype(np.float32)
        kernel = rng.integers(0, 16, c["kernel_support"] + (c["channels"], c["filters"])).astype(np.float32)
        kw = dict(corr=c["corr"], strides_down=c["strides_down"], strides_up=c["strides_up"], padding="valid",
                  extra_pad_end=c["extra_pad_end"], channel_separable=c["channel_separable"])
        if not so.oracle_implements(c["kernel_support"], c["corr"], c["strides_up"]):
            with pytest.raises(NotImplementedError):
                _oracle_nchw(x, kernel, **kw)
            continue
        want = cases2.scipy_convolve_valid(c["corr"], x, kernel, c["strides_down"], c["strides_up"], c["extra_pad_end"],
                                           c["channel_separable"])
        got = _oracle_nchw(x, kernel, **kw)
        assert got.shape == want.shape and np.array_equal(got, want), c
        ran += 1
    assert ran > 100


@pytest.mark.parametrize("module", [cases2, cases_nd], ids=["rank2", "rank1and3"])
def test_oracle_returns_the_input_for_identity_kernels(module):
    ran = 0
    for c in module.same_cases():
        support, ks = c["input_support"], c["kernel_support"]
        if not so.oracle_implements(ks, c["corr"], c["strides_up"]):
            continue
        x = np.arange(np.prod(support), dtype=np.float32).reshape((1, 1) + support)
        kernel = np.zeros(ks + (1, 1), np.float32)
        kernel[tuple(s // 2 for s in ks) + (0, 0)] = 1.0
        got = _oracle_nchw(x, kernel, corr=c["corr"], strides_down=c["strides_down"], strides_up=c["strides_up"],
                           padding=c["padding"], extra_pad_end=c["extra_pad_end"])
        want = x
        if not all(s == 1 for s in c["strides_up"]):
            want = cases2.numpy_upsample(want, c["strides_up"], c["extra_pad_end"])
        want = want[(slice(None), slice(None)) + tuple(slice(None, None, s) for s in c["strides_down"])]
        assert got.shape == want.shape and np.array_equal(got, want), c
        ran += 1
    assert ran > 80


@pytest.mark.parametrize("corr", [True, False])
@pytest.mark.parametrize("ks", [(3, 3), (5, 3), (4, 3)])
def test_oracle_equals_same_reflect_oracle(corr, ks):
    rng = np.random.default_rng(2)
    x = rng.integers(0, 32, (2, 3, 7, 9)).astype(np.float32)
    kernel = rng.integers(0, 16, ks + (3, 2)).astype(np.float32)
    got = _oracle_nchw(x, kernel, corr=corr, strides_down=(1, 1), strides_up=(1, 1), padding="same_reflect",
                       extra_pad_end=True)
    assert np.array_equal(got, cases2.same_reflect_oracle(x, kernel, ks, corr))


# ---- the kernels' stand-ins ---------------------------------------------------------------------------------------------
def emu_wgrad(a, b, support, strides, transpose):
    """include/tfc_hip.h, tfc_conv3d_wgrad: G[t][ca][cb] = sum_{n, q} A[n, q s + t - k // 2, ca] B[n, q, cb] (zeros outside
    A), summed tap by tap in float64; transpose: [.., cb, ca]."""
    k, s, q = tuple(support), tuple(strides), tuple(b.shape[1:4])
    pad = [0, 0]
    for d in (2, 1, 0):
        pad += [k[d], k[d] + q[d] * s[d]]
    ap, bd = torch.nn.functional.pad(a.double(), pad), b.double()
    g = torch.zeros(k + (a.shape[-1], b.shape[-1]), dtype=torch.float64)
    for t in itertools.product(*(range(n) for n in k)):
        first = [k[d] + t[d] - k[d] // 2 for d in range(3)]
        win = ap[(slice(None),) + tuple(slice(first[d], first[d] + q[d] * s[d], s[d]) for d in range(3))]
        g[t] = torch.einsum("ndhwa,ndhwb->ab", win, bd)
    return (g.transpose(-1, -2) if transpose else g).float()


def emu_conv3d(x, kernel, bias, strides, activation, up):
    return (emu3.emu_up if up else emu3.emu_down)(x, kernel, bias, strides, activation)


def emu_conv2d(x, kernel, bias, stride, activation, up, weights_key=0):
    if not (x.shape[-1] <= 4 or x.shape[-1] % 16 == 0):
        raise ValueError(f"tfc_conv2d: input channels must be a multiple of 16 or <= 4 (got {x.shape[-1]})")
    return emu_conv3d(x[:, None], kernel[None], bias, (1, stride, stride), activation, up)[:, 0]


def emu_conv2d_wgrad_launch(a, b, kernel_support, stride, transpose):
    if not all(c <= 4 or (c % 32 == 0 and c <= 256) for c in (a.shape[-1], b.shape[-1])):
        raise ValueError(f"tfc_conv2d_wgrad: channel counts must be <= 4 or multiples of 32 up to 256 "
                         f"(got {a.shape[-1]}, {b.shape[-1]})")
    return emu_wgrad(a[:, None], b[:, None], (1,) + tuple(kernel_support), (1, stride, stride), transpose)[0]


def _emulate_launchers(monkeypatch):
    from compression_amd import _lib
    from compression_amd.layers import functional
    monkeypatch.setattr(_lib, "require_device", lambda: None)
    monkeypatch.setattr(functional, "_conv2d_wgrad_launch", emu_conv2d_wgrad_launch)
    monkeypatch.setitem(functional._CONV_KERNELS, 2, (emu_conv2d, functional.conv2d_wgrad))
    monkeypatch.setitem(functional._CONV_KERNELS, 3, (emu_conv3d, emu_wgrad))


@pytest.fixture(params=["autograd", "conv_function"])
def emulated(request, monkeypatch):
    from compression_amd.layers import functional
    if request.param == "autograd":
        monkeypatch.setattr(functional, "conv2d_down", emu2.emu_down)
        monkeypatch.setattr(functional, "conv2d_up", emu2.emu_up)
        monkeypatch.setattr(functional, "conv3d_down", emu3.emu_down)
        monkeypatch.setattr(functional, "conv3d_up", emu3.emu_up)
    else:
        _emulate_launchers(monkeypatch)
    return request.param


@pytest.fixture
def conv_function(monkeypatch):
    _emulate_launchers(monkeypatch)


def test_weight_gradient_emulation_is_the_gradient_of_the_forward_emulations():
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.integers(-4, 5, (2, 3, 5, 7, 3)).astype(np.float64))
    w = torch.from_numpy(rng.integers(-3, 4, (2, 3, 4, 3, 2)).astype(np.float64)).requires_grad_(True)
    s = (1, 2, 3)
    for up, fn in ((False, emu3.emu_down), (True, emu3.emu_up)):
        y = fn(x, w, None, s)
        gy = so.cotangent(y.shape, 3).double()
        want, = torch.autograd.grad(y, w, gy)
        got = emu_wgrad(gy, x, w.shape[:3], s, True) if up else emu_wgrad(x, gy, w.shape[:3], s, False)
        assert torch.equal(got.double(), want)


# ---- the layers ----------------------------------------------------------------------------------------------------------
def layer_class(rank):
    from compression_amd import layers
    return {1: layers.SignalConv1D, 2: layers.SignalConv2D, 3: layers.SignalConv3D}[rank]


def check_case(case, seed=1, batch=2, activation=None, data_format="channels_last"):
    """y, dx, dkernel (and dbias) of the layer in all three requires_grad modes, equal to the oracle's."""
    x, kernel, bias = so.integer_data(case, seed, batch)
    if data_format == "channels_first":
        x = x.movedim(-1, 1).contiguous()
    want = so.oracle_with_gradients(case, x, kernel, bias, seed + 1, activation, data_format)
    y, gy, dx, dkernel, dbias = want
    for mode in so.MODES:
        got = so.layer_with_gradients(layer_class(len(case["input_support"])), case, x, kernel, bias, gy, mode,
                                      activation, data_format)
        assert got[0].shape == y.shape and torch.equal(got[0], y), (mode, "y")
        for name, g, w in zip(("dx", "dkernel", "dbias"), got[1:], (dx, dkernel, dbias)):
            assert g is None or (g.shape == w.shape and torch.equal(g, w)), (mode, name)
    return want


CASES_2D = so.implemented(itertools.chain(so.reference_cases(cases2), so.same_general_cases_2d()))
CASES_ND = so.implemented(itertools.chain(so.reference_cases(cases_nd), so.same_general_cases_nd()))


@pytest.mark.parametrize("case", CASES_2D, ids=so.case_id)
def test_rank2_training_path_equals_the_definition(emulated, case):
    check_case(case, activation=(lambda t: t) if case["use_bias"] else None)


@pytest.mark.parametrize("case", CASES_ND, ids=so.case_id)
def test_rank1_and_rank3_training_path_equals_the_definition(emulated, case):
    check_case(case, activation=(lambda t: t) if case["use_bias"] else None)


def test_case_lists_cover_what_they_are_for():
    """Unequal strides_up on rank 2 (zeros inserted by the layer), strides_up = (1, 2, 2), a mirror on all three axes,
    every padding mode with both directions, channel counts the kernels take padded."""
    assert any(c["strides_up"] == (2, 3) and c["padding"] == "same_reflect" for c in CASES_2D)
    assert any(c["strides_up"] == (1, 2, 2) for c in CASES_ND)
    assert any(c["padding"] == "same_reflect" and len(c["kernel_support"]) == 3 and min(c["kernel_support"]) >= 2
               for c in CASES_ND)
    for padding in ("valid", "same_zeros", "same_reflect"):
        for cs in (CASES_2D, CASES_ND):
            assert any(c["padding"] == padding and max(c["strides_up"]) > 1 for c in cs)
            assert any(c["padding"] == padding and max(c["strides_down"]) > 1 for c in cs)
    assert {(c["channels"], c["filters"]) for c in CASES_2D} >= {(3, 2), (5, 3), (16, 4)}


# the model configuration (`same_zeros`, one launch) at widths the models do not use: 1 ... 4, multiples of 16 that are
# no multiples of 32, and counts that are neither, on either side
MODEL_WIDTHS = [(3, 8), (16, 8), (16, 40), (48, 16), (5, 96), (160, 48), (32, 5)]
MODEL_KERNELS = [(5, 2), (3, 1), (9, 4)]


def model_width_cases():
    for i, ((k, s), (cin, filters), up) in enumerate(itertools.product(MODEL_KERNELS, MODEL_WIDTHS, (False, True))):
        case = so._case((7, 9), cin, filters, (k, k), not up, (1, 1) if up else (s, s), (s, s) if up else (1, 1), True,
                        "same_zeros", use_bias=i % 2 == 0)
        yield case, ("relu" if i % 2 == 0 else None)


def relu_safe_bias(case, x, kernel, bias):
    """The bias moved off every value that would make a pre-activation exactly 0 (checked on the oracle)."""
    pre = so.layer_oracle(x, kernel, corr=case["corr"], strides_down=case["strides_down"], strides_up=case["strides_up"],
                          padding=case["padding"], extra_pad_end=case["extra_pad_end"])
    bias = bias.clone()
    for c in range(bias.numel()):
        taken = set((-pre[..., c]).flatten().tolist())
        while float(bias[c]) in taken:
            bias[c] += 1
    assert not bool((pre + bias.double() == 0).any())
    return bias


@pytest.mark.parametrize("case,activation", list(model_width_cases()),
                         ids=lambda v: so.case_id(v) if isinstance(v, dict) else str(v))
def test_model_configuration_trains_at_every_width(conv_function, case, activation):
    x, kernel, bias = so.integer_data(case, 5, small=True)
    if bias is not None:
        bias = relu_safe_bias(case, x, kernel, bias)
    y, gy, dx, dkernel, dbias = so.oracle_with_gradients(case, x, kernel, bias, 6, activation)
    for mode in so.MODES:
        got = so.layer_with_gradients(layer_class(2), case, x, kernel, bias, gy, mode, activation)
        assert torch.equal(got[0], y), mode
        for name, g, w in zip(("dx", "dkernel", "dbias"), got[1:], (dx, dkernel, dbias)):
            assert g is None or (g.shape == w.shape and torch.equal(g, w)), (mode, name)


@pytest.mark.parametrize("rank,data_format,separable", [(1, "channels_first", True), (2, "channels_first", True),
                                                         (3, "channels_first", False), (2, "channels_last", True)])
def test_separable_channels_first_bias_and_callable_activation(emulated, rank, data_format, separable):
    support, ks = {1: ((11,), (3,)), 2: ((7, 6), (3, 3)), 3: ((4, 5, 6), (3, 2, 3))}[rank]
    case = so._case(support, 3, 2, ks, True, (2,) * rank, (1,) * rank, True, "same_reflect", sep=separable, use_bias=True)
    check_case(case, activation=lambda t: 2 * t, data_format=data_format)
    case = so._case(support, 3, 1 if separable else 2, ks, False, (1,) * rank, (2,) * rank, False, "valid", sep=separable,
                    use_bias=True)
    check_case(case, activation=lambda t: 2 * t, data_format=data_format)

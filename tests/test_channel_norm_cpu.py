"""CPU tier: ChannelNorm's tensor-op path (what the layer evaluates for a CPU tensor, and the statement of the formula the
kernels are tested against on the GPU) against a float64 NumPy evaluation of models/hific/archs.py:255-273, and the
host-side argument checks of the two C entries."""
import ctypes

import numpy as np
import pytest
import torch

from compression_amd import _lib
from compression_amd.layers import ChannelNorm, functional


def numpy_channel_norm(x, gamma, beta, epsilon=1e-3, relu=False, residual=None):
    x = np.asarray(x, np.float64)
    C = x.shape[-1]
    mean = x.sum(-1, keepdims=True) / C
    var = ((x - mean) ** 2).sum(-1, keepdims=True) / (C - 1)
    y = (x - mean) / np.sqrt(var + epsilon)
    if gamma is not None:
        y = y * np.asarray(gamma, np.float64)
    if beta is not None:
        y = y + np.asarray(beta, np.float64)
    if relu:
        y = np.maximum(y, 0)
    if residual is not None:
        y = y + np.asarray(residual, np.float64)
    return y


@pytest.mark.parametrize("C", [2, 3, 60, 61, 220, 960])
@pytest.mark.parametrize("form", ["plain", "relu", "residual"])
def test_layer_matches_the_float64_formula(C, form):
    rng = np.random.default_rng(C)
    x = (rng.standard_normal((2, 3, 5, C)) * rng.uniform(0.5, 2, C)).astype(np.float32)
    r = rng.standard_normal(x.shape).astype(np.float32)
    layer = ChannelNorm(num_channels=C)
    with torch.no_grad():
        layer.gamma.copy_(torch.from_numpy(rng.uniform(0.5, 2, C)))
        layer.beta.copy_(torch.from_numpy(rng.standard_normal(C)))
    kw = dict(relu=form == "relu", residual=torch.from_numpy(r) if form == "residual" else None)
    got = layer(torch.from_numpy(x), **kw).detach().numpy()
    want = numpy_channel_norm(x, layer.gamma.detach().numpy(), layer.beta.detach().numpy(), 1e-3,
                              form == "relu", r if form == "residual" else None)
    err = np.abs(got - want) / np.maximum(1, np.abs(want))
    assert got.shape == x.shape and err.max() <= 1e-5, err.max()


def test_the_variance_divides_by_c_minus_one():
    """C = 2, epsilon = 0: deviations +-1, unbiased variance 2, outputs +-1 / sqrt(2).  Dividing by N instead would
    give a variance of 1 and outputs +-1: a factor of sqrt(2)."""
    layer = ChannelNorm(epsilon=0.0, center=False, scale=False)
    y = layer(torch.tensor([[1.0, 3.0], [-2.0, 6.0]]))
    np.testing.assert_allclose(y.numpy(), [[-2 ** -0.5, 2 ** -0.5]] * 2, rtol=1e-6)
    assert list(layer.parameters()) == []


@pytest.mark.parametrize("center,scale", [(True, False), (False, True), (False, False)])
def test_center_and_scale_off(center, scale):
    rng = np.random.default_rng(1)
    x = rng.standard_normal((7, 12)).astype(np.float32)
    layer = ChannelNorm(center=center, scale=scale, beta_initializer=lambda c: torch.full((c,), 0.25),
                        gamma_initializer=lambda c: torch.full((c,), 1.5))
    got = layer(torch.from_numpy(x)).detach().numpy()
    want = numpy_channel_norm(x, np.full(12, 1.5) if scale else None, np.full(12, 0.25) if center else None)
    assert (layer.gamma is not None) == scale and (layer.beta is not None) == center
    assert np.abs(got - want).max() <= 1e-5


def _float64_formula(x, gamma, beta, eps, relu, detach):
    mean = x.mean(-1, keepdim=True)
    var = ((x - (mean.detach() if detach else mean)) ** 2).sum(-1, keepdim=True) / (x.shape[-1] - 1)
    y = (x - mean) * torch.rsqrt(var + eps) * gamma + beta
    return torch.relu(y) if relu else y


@pytest.mark.parametrize("relu", [False, True])
def test_gradients_and_the_immaterial_stop_gradient(relu):
    """The closed form the backward kernel implements (include/tfc_hip.h) against torch.autograd of the float64 formula
    WITH mean.detach() inside the variance (archs.py:267), and that formula against the one without: the term the
    stop-gradient removes is proportional to sum_c (x - mean) = 0."""
    torch.manual_seed(0)
    C = 24
    x = (torch.randn(11, C, dtype=torch.float64) * 2 + 3).requires_grad_()
    gamma = (torch.rand(C, dtype=torch.float64) + 0.5).requires_grad_()
    beta = torch.randn(C, dtype=torch.float64).requires_grad_()
    g = torch.randn(11, C, dtype=torch.float64)
    grads = {}
    for detach in (True, False):
        y = _float64_formula(x, gamma, beta, 1e-3, relu, detach)
        grads[detach] = torch.autograd.grad(y, (x, gamma, beta), g)
    for a, b in zip(grads[True], grads[False]):
        assert (a - b).abs().max() <= 1e-12
    with torch.no_grad():
        mean = x.mean(-1, keepdim=True)
        rstd = torch.rsqrt(((x - mean) ** 2).sum(-1, keepdim=True) / (C - 1) + 1e-3)
        xhat = (x - mean) * rstd
        gp = g * ((xhat * gamma + beta) > 0) if relu else g
        gg = gp * gamma
        dx = rstd * (gg - gg.sum(-1, keepdim=True) / C - xhat * (gg * xhat).sum(-1, keepdim=True) / (C - 1))
        closed = (dx, (gp * xhat).sum(0), gp.sum(0))
    for a, b in zip(grads[True], closed):
        assert (a - b).abs().max() <= 1e-12
    # and the layer's own CPU path (float32) differentiates to the same
    layer = ChannelNorm(num_channels=C)
    with torch.no_grad():
        layer.gamma.copy_(gamma)
        layer.beta.copy_(beta)
    x32 = x.detach().float().requires_grad_()
    layer(x32, relu=relu).backward(g.float())
    assert (x32.grad.double() - closed[0]).abs().max() <= 1e-4
    assert (layer.gamma.grad.double() - closed[1]).abs().max() <= 1e-4 * 11


def test_rejects_bad_input():
    with pytest.raises(ValueError):
        ChannelNorm()(torch.zeros(5))
    with pytest.raises(ValueError):
        ChannelNorm()(torch.zeros(5, 1))
    with pytest.raises(ValueError):
        ChannelNorm(beta_initializer="nope")


@pytest.mark.parametrize("entry", ["forward", "backward"])
def test_entries_validate_on_the_host(entry):
    """Bad arguments are refused before any launch (null pointers, no device needed), with a text in tfc_last_error."""
    lib = _lib.lib()

    def call(dtype=0, pixels=4, channels=8, epsilon=1e-3):
        if entry == "forward":
            return lib.tfc_channel_norm_forward(None, None, None, None, None, dtype, pixels, channels, epsilon, 0, None)
        return lib.tfc_channel_norm_backward(None, None, None, None, None, None, None, dtype, pixels, channels, epsilon,
                                             0, None)
    for kw, word in ((dict(dtype=2), "dtype"), (dict(channels=1), "channels"), (dict(pixels=-1), "pixels"),
                     (dict(epsilon=-1.0), "epsilon"), (dict(epsilon=float("nan")), "epsilon"),
                     (dict(epsilon=float("inf")), "epsilon"), (dict(), "null")):
        assert call(**kw) != 0
        assert word in _lib.last_error(), (kw, _lib.last_error())
    if entry == "forward":
        assert call(pixels=0) == 0

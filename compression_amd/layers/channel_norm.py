"""`ChannelNorm` of HiFiC (models/hific/archs.py:214-297) on the fused HIP kernel."""
from __future__ import annotations

import torch

from . import functional

__all__ = ["ChannelNorm"]

_INITIALIZERS = {"zeros": torch.zeros, "ones": torch.ones}


def _initializer(spec):
    if callable(spec):
        return spec
    if spec not in _INITIALIZERS:
        raise ValueError(f"Unknown initializer: '{spec}' (\"zeros\", \"ones\" or a callable of the channel count).")
    return _INITIALIZERS[spec]


class ChannelNorm(torch.nn.Module):
    """Per pixel, normalise over the channel (last) axis with the UNBIASED variance (archs.py:262-273 divides by
    C - 1), then scale by `gamma` and shift by `beta`:

        y = (x - mean) / sqrt(var + epsilon) * gamma + beta

    Same constructor arguments as the reference layer (archs.py:223-247).  `gamma` / `beta` [C] are created on the first
    call like a Keras `build` (`scale=False` / `center=False`: none).  `forward(x, relu=True)` and
    `forward(x, residual=r)` ask for the fused forms `relu(y)` and `y + r` in the same launch: the layers HiFiC puts
    behind 22 of its 24 norms.  Tensors on the device run `functional.channel_norm` (forward and backward kernels); a
    CPU tensor evaluates the same formula as tensor ops (`functional.channel_norm_reference`)."""

    def __init__(self, epsilon=1e-3, center=True, scale=True, beta_initializer="zeros", gamma_initializer="ones",
                 num_channels=None):
        super().__init__()
        self.epsilon = float(epsilon)
        self.center, self.scale = bool(center), bool(scale)
        self._beta_init, self._gamma_init = _initializer(beta_initializer), _initializer(gamma_initializer)
        self.gamma = self.beta = None
        if num_channels is not None:
            self.build(int(num_channels))

    def build(self, c, device=None):
        if self.scale and self.gamma is None:
            self.gamma = torch.nn.Parameter(self._gamma_init(c).float().to(device))
        if self.center and self.beta is None:
            self.beta = torch.nn.Parameter(self._beta_init(c).float().to(device))

    def forward(self, inputs, relu=False, residual=None):
        if inputs.dim() < 2:
            raise ValueError(f"Input tensor must have at least rank 2, received shape {tuple(inputs.shape)}.")
        if inputs.shape[-1] < 2:
            raise ValueError(f"ChannelNorm divides by channels - 1: at least 2 channels, got {inputs.shape[-1]}")
        self.build(inputs.shape[-1], inputs.device)
        if not inputs.is_cuda:
            return functional.channel_norm_reference(inputs, self.gamma, self.beta, self.epsilon, relu, residual)
        return functional.channel_norm(inputs, self.gamma, self.beta, self.epsilon, relu, residual)

    def extra_repr(self):
        return f"epsilon={self.epsilon}, center={self.center}, scale={self.scale}"

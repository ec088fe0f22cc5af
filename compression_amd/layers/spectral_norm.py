"""compare_gan's `conv2d(..., use_sn=True)` as HiFiC's discriminator uses it (models/hific/archs.py:340-367): a Keras
`SAME` cross-correlation whose kernel is divided by an estimate of its largest singular value, one power iteration per
call from a persistent vector `u`.

  W = kernel.reshape(-1, cout) [R, C];  l2n(a) = a * rsqrt(max(sum(a ** 2), 1e-12))
  v = l2n(W^T u);  u' = l2n(W v);  sigma = u'^T W v (u', v constants);  the convolution uses kernel / sigma

The window arithmetic, the channel padding and the kernels are KerasConv2D's; the normalisation, the bias gradient and
the optional leaky ReLU behind the convolution are the kernels of csrc/hific_gan.hip (`gan_functional`)."""
from __future__ import annotations

import functools

import torch

from . import gan_functional
from .keras_conv import KerasConv2D, _padded_channels

__all__ = ["SpectralNormConv2D"]


class SpectralNormConv2D(KerasConv2D):
    """Parameters `kernel` [kh, kw, in, out] ~ N(0, 0.02 ** 2) and `bias` [out] = 0; buffer `u` [kh kw in, 1] ~ N(0, 1),
    part of the state dict.  In `train()` mode every call advances `u` to u'; in `eval()` the stored `u` is used and left
    alone.  `forward(x, lrelu=True)` applies max(y, 0.2 y) in place behind the convolution.  `x` may already carry the
    zero channels the kernels want (`padded_in_channels`)."""

    def build(self, cin, device=None):
        if self.kernel is not None:
            return
        kh, kw = self.kernel_size
        self.kernel = torch.nn.Parameter(torch.randn(kh, kw, cin, self.filters, device=device) * 0.02)
        self.bias = torch.nn.Parameter(torch.zeros(self.filters, device=device))
        self.register_buffer("u", torch.randn(kh * kw * cin, 1, device=device))

    def padded_in_channels(self):
        """The input channel count the kernels take in the current gradient mode."""
        return _padded_channels(self.kernel.shape[2], 32 if torch.is_grad_enabled() else 16)

    def normalized_kernel(self):
        """kernel / sigma; advances `u` in train() mode."""
        w_sn, u_new = gan_functional.spectral_norm(self.kernel, self.u)
        if self.training:
            with torch.no_grad():
                self.u.copy_(u_new.reshape(self.u.shape))
        return w_sn

    def _padded(self, cin_act):
        k = self.normalized_kernel()
        if torch.is_grad_enabled():
            cin_p, cout_p = _padded_channels(cin_act, 32), _padded_channels(self.filters, 32)
        else:
            cin_p, cout_p = _padded_channels(cin_act, 16), self.filters
        k = torch.nn.functional.pad(k, (0, cout_p - k.shape[3], 0, cin_p - k.shape[2]))
        return k, torch.nn.functional.pad(self.bias, (0, cout_p - self.filters)), 0

    def forward(self, x, lrelu=False):
        if x.dim() != 4:
            raise ValueError(f"Input tensor must have rank 4, received shape {tuple(x.shape)}.")
        if self.kernel is None:
            self.build(x.shape[-1], x.device)
        cin = self.kernel.shape[2]
        kernel, bias, key = self._padded(cin)
        if x.shape[-1] == cin and kernel.shape[2] != cin:
            x = torch.nn.functional.pad(x, (0, kernel.shape[2] - cin))
        if x.shape[-1] != kernel.shape[2]:
            raise ValueError(f"kernel expects {cin} input channels (or {kernel.shape[2]} with its zero channels), "
                             f"input has {x.shape[-1]}")
        conv = functools.partial(gan_functional.conv2d_bias_lrelu, lrelu=lrelu)
        y = self._run(x, kernel, bias, key, conv=conv)
        return y if y.shape[-1] == self.filters else y[..., :self.filters]

"""The masked 5x5 correlation of a spatial context model (Minnen, Ballé, Toderici 2018, section 2; the mask of van
den Oord et al.'s PixelCNN, type A): output (i, j) sees input rows above i and, in row i, the columns left of j."""
from __future__ import annotations

import math

import torch

from ..ops.context_ops import CAUSAL_TAPS, tap_mask
from .signal_conv import SignalConv2D

__all__ = ["MaskedConv2D"]


class MaskedConv2D(SignalConv2D):
    """`SignalConv2D(filters, (5, 5), corr=True, padding="same_zeros", use_bias=True)` whose kernel is the variable
    `kernel_variable` [5, 5, in, filters] times the mask of `TAPS` (the causal taps; a subclass names its own 12),
    handed to the base class as a callable `kernel_parameter`: the layer runs on the convolution kernels of every other
    layer, gradients included, and the masked taps of `kernel_variable` get zero gradient.  CPU tensors take the same
    definition as a tensor op."""

    TAPS = CAUSAL_TAPS

    def __init__(self, filters, in_channels, kernel_initializer=None, use_bias=True):
        super().__init__(filters, (5, 5), corr=True, padding="same_zeros", use_bias=use_bias,
                         kernel_parameter=self._masked_kernel)
        cin = int(in_channels)
        shape = (5, 5, cin, self.filters)
        if kernel_initializer is not None:
            k = torch.as_tensor(kernel_initializer(shape)).float()
        else:
            # Keras VarianceScaling(fan_in, truncated normal) over the 12 taps that count
            std = math.sqrt(1.0 / (12 * cin)) / 0.87962566103423978
            k = torch.empty(shape)
            torch.nn.init.trunc_normal_(k, std=std, a=-2 * std, b=2 * std)
        self.build(cin)                                  # the bias; the kernel is given
        self.kernel_variable = torch.nn.Parameter(k)
        self.register_buffer("mask", tap_mask(self.TAPS), persistent=False)

    def _masked_kernel(self):
        return self.kernel_variable * self.mask.to(self.kernel_variable.dtype)

    def _forward(self, inputs, with_bias=True):
        if inputs.is_cuda or self.data_format != "channels_last":
            return super()._forward(inputs, with_bias)
        kernel = self.kernel.to(inputs.dtype)
        bias = self._bias_value() if with_bias else None
        y = torch.nn.functional.conv2d(inputs.permute(0, 3, 1, 2), kernel.permute(3, 2, 0, 1),
                                       None if bias is None else bias.to(inputs.dtype), padding=2)
        return y.permute(0, 2, 3, 1)

"""The masked 5x5 correlation of the checkerboard context model (He, Zheng, Sun, Wang, Qin 2021): a non-anchor output
(i + j odd) sees the 12 inputs of its 5x5 window at odd distance (di + dj odd), which are all anchors; an anchor
output sees nothing and is the bias alone.  Applied to a whole latent it is the model's definition, teacher-forced."""
from __future__ import annotations

from .masked_conv import MaskedConv2D

__all__ = ["CheckerboardConv2D"]


class CheckerboardConv2D(MaskedConv2D):
    """`MaskedConv2D`'s construction with the checkerboard mask: the kernel is `kernel_variable` [5, 5, in, filters]
    times the mask, the layer runs on the convolution kernels of every other layer, and the masked taps get zero
    gradient.  The forward multiplies the convolution term by the non-anchor mask, so anchor outputs keep the bias
    only."""

    def __init__(self, filters, in_channels, kernel_initializer=None, use_bias=True):
        from ..ops.checkerboard_ops import checkerboard_mask
        super().__init__(filters, in_channels, kernel_initializer=kernel_initializer, use_bias=use_bias)
        self.mask = checkerboard_mask()                  # replaces the buffer; 12 taps as well, so the same initialiser

    def forward(self, inputs):
        from ..ops.checkerboard_ops import anchor_mask
        if self.data_format != "channels_last":
            raise ValueError("CheckerboardConv2D needs channels_last inputs")
        bias = self._bias_value()
        use_bias, self.use_bias = self.use_bias, False          # the convolution term alone: the bias is added below
        try:
            conv = super().forward(inputs)
        finally:
            self.use_bias = use_bias
        others = (~anchor_mask(inputs.shape[-3], inputs.shape[-2], inputs.device)).to(conv.dtype)[:, :, None]
        return conv * others if bias is None else conv * others + bias.to(conv.dtype)

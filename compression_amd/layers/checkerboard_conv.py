"""The masked 5x5 correlation of the checkerboard context model (He, Zheng, Sun, Wang, Qin 2021): a non-anchor output
(i + j odd) sees the 12 inputs of its 5x5 window at odd distance (di + dj odd), which are all anchors; an anchor
output sees nothing and is the bias alone.  Applied to a whole latent it is the model's definition, teacher-forced."""
from __future__ import annotations

from ..ops.checkerboard_ops import CHECKER_TAPS, anchor_mask
from .masked_conv import MaskedConv2D

__all__ = ["CheckerboardConv2D"]


class CheckerboardConv2D(MaskedConv2D):
    """`MaskedConv2D` with the checkerboard taps (12 as well, so the same initialiser).  The forward multiplies the
    convolution term by the non-anchor mask, so anchor outputs keep the bias only."""

    TAPS = CHECKER_TAPS

    def forward(self, inputs):
        if self.data_format != "channels_last":
            raise ValueError("CheckerboardConv2D needs channels_last inputs")
        bias = self._bias_value()
        conv = self._forward(inputs, with_bias=False)           # the convolution term alone: the bias is added below
        others = (~anchor_mask(inputs.shape[-3], inputs.shape[-2], inputs.device)).to(conv.dtype)[:, :, None]
        return conv * others if bias is None else conv * others + bias.to(conv.dtype)

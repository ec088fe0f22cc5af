"""The entropy model of the overfitted codecs (Ladune et al., Cool-chic; Kim et al., C3): a latent grid is coded by a
tiny autoregressive MLP, the ARM, which reads the nearest already-decoded neighbours of a pixel and gives the location
and scale of a Laplace distribution.  The model owns the MLP and reports a rate (`ops/arm_ops.py`, csrc/arm_bits.hip);
like LVAC's auto-decoder it has no bitstream yet: the wavefront decode is a later step, as are Cool-chic's upsampling
and synthesis networks and its quantisation schedule."""
from __future__ import annotations

import torch
from torch import nn

from ..ops import arm_ops

__all__ = ["ArmEntropyModel"]


class ArmEntropyModel(nn.Module):
    """`context` (8, 16, 24 or 32) causal neighbours, `hidden_layers` (1..3) residual layers of that width and an output
    layer to (mu, log scale).  Latents are grids [B, H, W]; the grids of one call share the MLP, as the latent pyramid
    of one image does (one call per resolution)."""

    def __init__(self, context=24, hidden_layers=2):
        super().__init__()
        arm_ops.arm_context_offsets(context)               # raises on a size the kernels do not have
        if not 1 <= hidden_layers <= arm_ops.ARM_CONSTANTS["ARM_MAX_L"]:
            raise ValueError(f"hidden_layers must be in [1, {arm_ops.ARM_CONSTANTS['ARM_MAX_L']}], got {hidden_layers}")
        self.context, self.hidden_layers = int(context), int(hidden_layers)
        self.weight = nn.Parameter(torch.empty(hidden_layers, context, context))
        self.bias = nn.Parameter(torch.empty(hidden_layers, context))
        self.weight_out = nn.Parameter(torch.empty(context, 2))
        self.bias_out = nn.Parameter(torch.empty(2))
        self.reset_parameters()

    def reset_parameters(self, generator=None):
        """Residual layers start small (the MLP starts near the identity), the output layer at N(0, 1 / context), the
        biases at zero: mu = 0, scale = 1 on a zero grid."""
        with torch.no_grad():
            self.weight.normal_(0.0, 0.1 * self.context ** -0.5, generator=generator)
            self.weight_out.normal_(0.0, self.context ** -0.5, generator=generator)
            self.bias.zero_()
            self.bias_out.zero_()

    @property
    def context_offsets(self):
        return arm_ops.arm_context_offsets(self.context)

    def forward(self, y):
        """y [B, H, W] -> (bits [B], mu, scale [B, H, W]); bits is differentiable in y and the parameters."""
        return arm_ops.arm_bits(y, self.weight, self.bias, self.weight_out, self.bias_out, want_params=True)

    def bits(self, y):
        return arm_ops.arm_bits(y, self.weight, self.bias, self.weight_out, self.bias_out)

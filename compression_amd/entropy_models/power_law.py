"""PowerLawEntropyModel — python/entropy_models/power_law.py of tensorflow/compression.

Quantises by rounding (straight-through gradient), penalises log((|x| + alpha) / alpha), and codes each coding
unit with the run-length gamma code (RunLengthGammaEncode) on the GPU: one launch sequence for the whole batch,
rounding fused into the encoder's load."""
from __future__ import annotations

import torch

from ..ops import gen_ops
from ..ops.round_ops import round_st


def _units_view(bottleneck, coding_rank):
    """-> ([units, unit_len...] view, strings shape)."""
    shape = tuple(bottleneck.shape)
    if coding_rank > len(shape):
        raise ValueError(f"`bottleneck` must have at least {coding_rank} dimensions, got shape {list(shape)}")
    if coding_rank == 0:
        return bottleneck.reshape(-1, 1), shape
    return bottleneck.reshape((-1,) + shape[len(shape) - coding_rank:]), shape[:len(shape) - coding_rank]


class _RunLengthModelBase(torch.nn.Module):
    """compress / decompress over the run-length codec, shared by both models."""

    _codes = (-1, -1, False)

    def __init__(self, coding_rank, bottleneck_dtype=None):
        super().__init__()
        self._coding_rank = int(coding_rank)
        if self._coding_rank < 0:
            raise ValueError("`coding_rank` must be at least 0.")
        self._bottleneck_dtype = bottleneck_dtype or torch.get_default_dtype()

    @property
    def bottleneck_dtype(self):
        """Data type of the bottleneck tensor."""
        return self._bottleneck_dtype

    @property
    def coding_rank(self):
        """Number of innermost dimensions considered a coding unit."""
        return self._coding_rank

    def _convert(self, bottleneck):
        return torch.as_tensor(bottleneck).to(self.bottleneck_dtype)

    def forward(self, bottleneck):
        """(self.quantize(bottleneck), self.penalty(bottleneck))."""
        bottleneck = self._convert(bottleneck)
        return self.quantize(bottleneck), self.penalty(bottleneck)

    def quantize(self, bottleneck):
        """Rounds to integers with a straight-through (identity) gradient."""
        return round_st(self._convert(bottleneck))

    def compress(self, bottleneck):
        """-> numpy object array of strings shaped like `bottleneck` without its coding_rank innermost
        dimensions: round(bottleneck) coded per coding unit (rounding fused into the encoder's load)."""
        bottleneck = self._convert(bottleneck)
        units, strings_shape = _units_view(bottleneck, self.coding_rank)
        if units.dtype not in (torch.float32, torch.bfloat16, torch.float16, torch.int32):
            units = units.float()
        strings = gen_ops.run_length_encode_batched(units, *self._codes)
        return strings.reshape(strings_shape)

    def decompress(self, strings, code_shape):
        """-> tensor of shape strings.shape + code_shape and bottleneck_dtype (on the device)."""
        code_shape = gen_ops._shape_list(code_shape)
        if len(code_shape) != self.coding_rank:
            raise ValueError(f"`code_shape` must have {self.coding_rank} dimensions, got {code_shape}")
        direct = self.bottleneck_dtype if self.bottleneck_dtype in (torch.float32, torch.bfloat16) else torch.int32
        out = gen_ops.run_length_decode_batched(strings, code_shape, *self._codes, dtype=direct)
        return out.to(self.bottleneck_dtype)


class PowerLawEntropyModel(_RunLengthModelBase):
    """Entropy model for power-law distributed random variables: rounding, the penalty
    log((|x| + alpha) / alpha), and the run-length gamma code (RunLengthGammaEncode)."""

    _codes = (-1, -1, False)

    def __init__(self, coding_rank, alpha=1e-2, bottleneck_dtype=None):
        coding_rank = int(coding_rank)
        if coding_rank < 0:
            raise ValueError("`coding_rank` must be at least 0.")
        self_alpha = float(alpha)
        if self_alpha <= 0:
            raise ValueError("`alpha` must be greater than 0.")
        super().__init__(coding_rank, bottleneck_dtype)
        self._alpha = self_alpha

    @property
    def alpha(self):
        """Alpha parameter."""
        return self._alpha

    def penalty(self, bottleneck):
        """sum over the coding unit of log((|x| + alpha) / alpha); differentiable."""
        bottleneck = self._convert(bottleneck)
        penalty = torch.log((bottleneck.abs() + self.alpha) / self.alpha)
        return penalty.sum(dim=tuple(range(-self.coding_rank, 0))) if self.coding_rank else penalty

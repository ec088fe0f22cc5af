"""LaplaceEntropyModel — python/entropy_models/laplace.py of tensorflow/compression.

Quantises by rounding (straight-through gradient), penalises l1 * sum(|x|), and codes each coding unit with
RunLengthEncode(run_length_code, magnitude_code, use_run_length_for_non_zeros) on the GPU."""
from __future__ import annotations

from .power_law import _RunLengthModelBase


class LaplaceEntropyModel(_RunLengthModelBase):
    """Entropy model for Laplace distributed random variables: rounding, the penalty l1 * sum(|x|), and the
    run-length code with Rice or gamma codes for runs and magnitudes (RunLengthEncode)."""

    def __init__(self, coding_rank, l1=0.01, run_length_code=-1, magnitude_code=0,
                 use_run_length_for_non_zeros=False, bottleneck_dtype=None):
        coding_rank = int(coding_rank)
        if coding_rank < 0:
            raise ValueError("`coding_rank` must be at least 0.")
        l1 = float(l1)
        if l1 <= 0:
            raise ValueError("`l1` must be greater than 0.")
        super().__init__(coding_rank, bottleneck_dtype)
        self._l1 = l1
        self._run_length_code = int(run_length_code)
        self._magnitude_code = int(magnitude_code)
        self._use_run_length_for_non_zeros = bool(use_run_length_for_non_zeros)
        if self._run_length_code > 31 or self._magnitude_code > 31:
            raise ValueError("`run_length_code` and `magnitude_code` must be at most 31.")
        self._codes = (self._run_length_code, self._magnitude_code, self._use_run_length_for_non_zeros)

    @property
    def l1(self):
        """L1 parameter."""
        return self._l1

    @property
    def run_length_code(self):
        """run_length_code parameter."""
        return self._run_length_code

    @property
    def magnitude_code(self):
        """magnitude_code parameter."""
        return self._magnitude_code

    @property
    def use_run_length_for_non_zeros(self):
        """use_run_length_for_non_zeros parameter."""
        return self._use_run_length_for_non_zeros

    def penalty(self, bottleneck):
        """l1 * sum over the coding unit of |x|; differentiable."""
        bottleneck = self._convert(bottleneck)
        return self.l1 * bottleneck.abs().sum(dim=tuple(range(-self.coding_rank, 0))) \
            if self.coding_rank else self.l1 * bottleneck.abs()

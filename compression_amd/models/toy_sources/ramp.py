"""The ramp process (models/toy_sources/ramp.py)."""
from __future__ import annotations

import torch

from ._source import Source, index_points_tensor


class Ramp(Source):
    """Y(t) = (t + V) mod 1 - 0.5, V uniform over [0, 1]; `phase` fixes V."""

    def __init__(self, index_points, phase=None, dtype=torch.float32):
        super().__init__(dtype)
        self.index_points = index_points_tensor(index_points, dtype)
        self.phase = phase

    @property
    def event_shape(self):
        return self.index_points.shape

    def _sample_n(self, n, generator, device):
        if self.phase is None:
            phase = self._uniform((n, 1), generator, device)
        else:
            phase = torch.full((n, 1), float(self.phase), dtype=self.dtype, device=device)
        return torch.remainder(self._points(device) + phase, 1.0) - 0.5

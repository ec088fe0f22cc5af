"""The sawbridge process (models/toy_sources/sawbridge.py)."""
from __future__ import annotations

import torch

from ._source import Source, index_points_tensor


class Sawbridge(Source):
    """B(t) = t - 1(t > Z), Z uniform over [0, 1]; the stationary sawbridge is B((t + V) mod 1) with V uniform and
    independent of Z.  `order` sawbridges sharing V are added and divided by sqrt(order).  `phase` / `drop` fix V / Z."""

    def __init__(self, index_points, phase=None, drop=None, stationary=True, order=1, dtype=torch.float32):
        super().__init__(dtype)
        self.index_points = index_points_tensor(index_points, dtype)
        self.phase = phase
        self.drop = drop
        self.stationary = bool(stationary)
        self.order = int(order)

    @property
    def event_shape(self):
        return self.index_points.shape

    def _sample_n(self, n, generator, device):
        if self.drop is None:
            uniform = self._uniform((self.order, n, 1), generator, device)
        else:
            uniform = torch.full((self.order, n, 1), float(self.drop), dtype=self.dtype, device=device)
        ind = self._points(device)
        if self.stationary:
            if self.phase is None:
                phase = self._uniform((n, 1), generator, device)
            else:
                phase = torch.tensor(float(self.phase), dtype=self.dtype, device=device)
            ind = torch.remainder(ind + phase, 1.0)
        less = uniform < ind                                   # [order, n, time]
        sample = ind - less.to(self.dtype).sum(dim=0)
        return (sample * self.order ** -0.5).expand(n, -1)

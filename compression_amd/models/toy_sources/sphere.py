"""Uniform distribution on the unit hypersphere (models/toy_sources/sphere.py)."""
from __future__ import annotations

import torch

from ._source import Source


class Sphere(Source):
    """Normal draws divided by their norm; with `width` the norm is multiplied by a uniform factor in
    [1 - width / 2, 1 + width / 2] before the division (the reference's formula), a band around the sphere."""

    def __init__(self, order=2, width=0.0, dtype=torch.float32):
        super().__init__(dtype)
        self.order = int(order)
        self.width = float(width)

    @property
    def event_shape(self):
        return torch.Size((self.order,))

    def _sample_n(self, n, generator, device):
        samples = torch.randn((n, self.order), generator=generator, dtype=self.dtype, device=device)
        radius = torch.sqrt(torch.sum(samples * samples, dim=-1, keepdim=True))
        if self.width:
            radius = radius * (1.0 - self.width / 2.0 + self.width * self._uniform((n, 1), generator, device))
        return samples / radius

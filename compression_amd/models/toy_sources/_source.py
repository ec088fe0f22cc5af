"""What the four sources share.  The reference's sources are tfp Distributions drawing with TensorFlow's stateless
generators; those streams cannot be reproduced here (TensorFlow is not available where this was written), so a source
draws from a `torch.Generator` instead and only the closed forms (`phase` / `drop` given) are pinned by tests."""
from __future__ import annotations

import torch


class Source:
    """A vector-valued source: `event_shape` [D], `batch_shape` (), `sample(n)` -> [n, D]."""

    def __init__(self, dtype=torch.float32):
        self.dtype = dtype

    @property
    def batch_shape(self):
        return torch.Size(())

    @property
    def event_shape(self):
        raise NotImplementedError

    def sample(self, n, generator=None, device=None):
        """`n` realisations [n, D] on `device` (that of `generator` if one is given)."""
        if device is None and generator is not None:
            device = generator.device
        return self._sample_n(int(n), generator, torch.device(device if device is not None else "cpu"))

    def _uniform(self, shape, generator, device):
        return torch.rand(shape, generator=generator, dtype=self.dtype, device=device)

    def _points(self, device):
        return self.index_points.to(device)


def index_points_tensor(index_points, dtype):
    points = torch.as_tensor(index_points, dtype=dtype)
    if points.dim() != 1:
        raise ValueError(f"index_points must be 1-D, received shape {tuple(points.shape)}")
    return points

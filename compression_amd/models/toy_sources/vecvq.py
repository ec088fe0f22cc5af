"""Variational entropy-constrained vector quantisation (models/toy_sources/vecvq.py), the baseline the NTC results are
judged against.  The assignment, which is the whole cost of the model, runs on `ecvq_assign` (csrc/vecvq.hip)."""
from __future__ import annotations

import math

import torch

from ...ops import vq_ops
from .compression_model import CompressionModel


class VECVQModel(CompressionModel):
    """`codebook` [K, D] and `_logits` [K].  `initialize`: "sample" (draws from the source), "sample-<scale>" (plus
    normal noise of that standard deviation) or "uniform-<width>"."""

    def __init__(self, codebook_size, initialize="sample", logit_scale=1.0, generator=None, **kwargs):
        super().__init__(**kwargs)
        self.codebook_size = int(codebook_size)
        self.logit_scale = float(logit_scale)
        shape = (self.codebook_size, self.ndim_source)
        if initialize.startswith("sample"):
            codebook = self.source.sample(self.codebook_size, generator=generator).to("cpu", self.dtype)
            if len(initialize) > 6:
                codebook = codebook + float(initialize[7:]) * torch.randn(shape, generator=generator, dtype=self.dtype)
        elif initialize.startswith("uniform-"):
            width = float(initialize[8:])
            codebook = (torch.rand(shape, generator=generator, dtype=self.dtype) - 0.5) * width
        else:
            raise ValueError(f"Unknown initialize: '{initialize}'.")
        assert tuple(codebook.shape) == shape
        logits = torch.randn(self.codebook_size, generator=generator, dtype=self.dtype) * (self.logit_scale / 10)
        self.codebook = torch.nn.Parameter(codebook.contiguous())
        self._logits = torch.nn.Parameter(logits)

    @property
    def logits(self):
        return self._logits / self.logit_scale

    def rates(self):
        """Bits per codeword: (logsumexp(l) - l) / ln 2.  K numbers, tensor ops."""
        logits = self.logits
        return (torch.logsumexp(logits, dim=0) - logits) / math.log(2.0)

    def all_rd(self, x):
        """-> (rates [K], distortions [..., K]): the full matrix, for small inputs and for checks."""
        return self.rates(), self.distortion_fn(x.unsqueeze(-2), self.codebook)

    def quantize(self, x):
        rates = self.rates()
        indexes, _, _ = vq_ops.ecvq_assign(x.to(self.dtype).detach(), self.codebook.detach(), rates.detach(),
                                           self.lmbda, self.distortion_loss)
        return self.codebook, rates, indexes

    def test_losses(self, x):
        _, rates, distortions = vq_ops.ecvq_assign(x.to(self.dtype), self.codebook, self.rates(), self.lmbda,
                                                   self.distortion_loss)
        return rates, distortions

    train_losses = test_losses

    def usage(self, x):
        """int32 [K]: how many elements of `x` each codeword takes."""
        return vq_ops.ecvq_counts(x.to(self.dtype).reshape(-1, self.ndim_source), self.codebook, self.rates(),
                                  self.lmbda, self.distortion_loss)

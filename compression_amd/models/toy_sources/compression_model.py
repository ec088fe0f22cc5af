"""Base class of the toy-source coding experiments (models/toy_sources/compression_model.py): the rate-distortion
train and test steps.  Keras `fit` / `compile`, tf.data and the plotting methods are not restated."""
from __future__ import annotations

import torch


class CompressionModel(torch.nn.Module):
    """`source` (see sawbridge.py ...), the trade-off `lmbda` and `distortion_loss` in {"sse", "mse"}.  Subclasses
    give `quantize`, `train_losses` and `test_losses`."""

    def __init__(self, source, lmbda, distortion_loss):
        super().__init__()
        self.source = source
        self.lmbda = float(lmbda)
        self.distortion_loss = str(distortion_loss)
        if self.distortion_loss not in ("sse", "mse"):
            raise ValueError(f"distortion_loss must be 'sse' or 'mse', got {distortion_loss!r}")

    @property
    def dtype(self):
        return self.source.dtype

    @property
    def ndim_source(self):
        return int(self.source.event_shape[0])

    def quantize(self, x):
        """An equivalent vector quantiser for the batch `x` -> (codebook, rates, indexes): the vectors that represent
        the elements of `x`, the bits each of them costs, and for every element of `x` its index into the codebook."""
        raise NotImplementedError

    def train_losses(self, x):
        """-> (rates, distortions) per element of `x`, as the training objective sees them."""
        raise NotImplementedError

    def test_losses(self, x):
        """-> (rates, distortions) per element of `x`: bits to encode it, and its distortion loss."""
        raise NotImplementedError

    def distortion_fn(self, reference, reconstruction):
        diff = (reference.to(self.dtype) - reconstruction) ** 2
        return diff.sum(dim=-1) if self.distortion_loss == "sse" else diff.mean(dim=-1)

    def train_step(self, x, optimizer):
        """One step on the mean of rate + lmbda distortion -> {"loss", "rate", "distortion", "gradient RMS"} of this
        batch (the reference reports running Keras means of the same four)."""
        if hasattr(self, "alpha"):
            self.alpha = self.force_alpha
        optimizer.zero_grad(set_to_none=True)
        rates, distortions = self.train_losses(x)
        losses = rates + self.lmbda * distortions
        loss = losses.mean()
        loss.backward()
        energy, size = 0.0, 0
        for param in self.parameters():
            if param.grad is None:
                continue
            energy = energy + param.grad.detach().to(torch.float64).pow(2).sum()
            size += param.grad.numel()
        optimizer.step()
        rms = torch.sqrt(energy / size) if size else torch.zeros((), dtype=torch.float64)
        return {"loss": loss.detach(), "rate": rates.detach().mean(), "distortion": distortions.detach().mean(),
                "gradient RMS": rms}

    @torch.no_grad()
    def test_step(self, x):
        rates, distortions = self.test_losses(x)
        losses = rates + self.lmbda * distortions
        return {"loss": losses.mean(), "rate": rates.mean(), "distortion": distortions.mean()}

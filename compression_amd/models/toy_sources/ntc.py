"""Nonlinear transform coding (models/toy_sources/ntc.py): an analysis / synthesis pair around a prior, with dither
and soft rounding.  Everything below the model is already in this package (DeepFactorized, MixtureSameFamily, the
soft-round and uniform-noise adapters, round_st, quantization_offset).  The plotting methods are not restated."""
from __future__ import annotations

import math

import torch

from ... import distributions as tfcd
from ...ops import round_ops
from .compression_model import CompressionModel

_MIXTURES = ("gsm-", "gmm-", "lsm-", "lmm-")


class NTCModel(CompressionModel):
    """`analysis`, `synthesis`: modules mapping [N, ndim_source] -> [N, ndim_latent] and back.
    `prior_type`: "deep" (DeepFactorized) or "gsm/gmm/lsm/lmm-X", a Gaussian / logistic scale mixture / mixture model
    of X components.  `dither`: four flags, dither for the rate and for the distortion term in training, then in
    testing.  `soft_round`: two flags, training and testing.  `guess_offset`: without soft rounding, centre the
    quantiser on the prior's mode in testing.  `ndim_latent`: the width of the latent; where it is None it is found
    with one call of `analysis` on zeros (there is no Keras `output_shape` to read)."""

    def __init__(self, analysis, synthesis, prior_type="deep", dither=(1, 1, 0, 0), soft_round=(1, 0),
                 guess_offset=False, ndim_latent=None, generator=None, **kwargs):
        super().__init__(**kwargs)
        self._analysis = analysis
        self._synthesis = synthesis
        self.prior_type = str(prior_type)
        self.dither = tuple(bool(i) for i in dither)
        self.soft_round = tuple(bool(i) for i in soft_round)
        self.guess_offset = bool(guess_offset)
        if len(self.dither) != 4 or len(self.soft_round) != 2:
            raise ValueError("dither takes 4 flags and soft_round 2")
        if ndim_latent is None:
            with torch.no_grad():
                probe = analysis(torch.zeros(1, self.ndim_source, dtype=self.dtype,
                                             device=next(iter(analysis.parameters()), torch.zeros(())).device))
            ndim_latent = probe.shape[-1]
        self.ndim_latent = int(ndim_latent)

        if self.prior_type == "deep":
            self._prior = tfcd.DeepFactorized(batch_shape=(self.ndim_latent,), dtype=self.dtype)
        elif self.prior_type[:4] in _MIXTURES:
            shape = (self.ndim_latent, int(self.prior_type[4:]))
            self.logits = torch.nn.Parameter(torch.randn(shape, generator=generator, dtype=self.dtype))
            self.log_scale = torch.nn.Parameter(2.0 + torch.randn(shape, generator=generator, dtype=self.dtype))
            if self.prior_type[1] == "s":
                self.loc = 0.0
            else:
                self.loc = torch.nn.Parameter(torch.randn(shape, generator=generator, dtype=self.dtype))
        else:
            raise ValueError(f"Unknown prior_type: '{prior_type}'.")
        self._logit_alpha = torch.nn.Parameter(torch.tensor(-3.0, dtype=self.dtype))
        self.register_buffer("_force_alpha", torch.tensor(-1.0, dtype=self.dtype))

    def prior(self, soft_round, alpha=None, skip_noise=False):
        if self.prior_type == "deep":
            prior = self._prior
        else:
            family = tfcd.Normal if self.prior_type.startswith("g") else tfcd.Logistic
            loc = self.loc if torch.is_tensor(self.loc) else torch.zeros_like(self.log_scale)
            prior = tfcd.MixtureSameFamily(torch.softmax(self.logits, dim=-1),
                                           family(loc=loc, scale=torch.exp(self.log_scale), dtype=self.dtype))
        if soft_round:
            prior = tfcd.SoftRoundAdapter(prior, self.alpha if alpha is None else alpha)
        return prior if skip_noise else tfcd.UniformNoiseAdapter(prior)

    def _flat_apply(self, transform, values, width_in, width_out):
        values = values.to(self.dtype)
        if values.shape[-1] != width_in:
            raise ValueError(f"Expected {width_in} trailing dimensions, received {values.shape[-1]}.")
        out = transform(values.reshape(-1, width_in))
        assert out.shape[-1] == width_out
        return out.reshape(*values.shape[:-1], width_out)

    def analysis(self, x):
        return self._flat_apply(self._analysis, x, self.ndim_source, self.ndim_latent)

    def synthesis(self, y):
        return self._flat_apply(self._synthesis, y, self.ndim_latent, self.ndim_source)

    @property
    def force_alpha(self):
        return self._force_alpha

    @force_alpha.setter
    def force_alpha(self, value):
        with torch.no_grad():
            self._force_alpha.fill_(-1.0 if value is None else float(value))

    @property
    def alpha(self):
        return torch.sigmoid(self._logit_alpha) * 4.0

    @alpha.setter
    def alpha(self, value):
        """A negative value (force_alpha's "not forced") leaves alpha as it is."""
        value = float(value.detach()) if torch.is_tensor(value) else float(value)
        if value < 0:
            return
        a = min(max(value / 4.0, 0.0), 1.0)
        with torch.no_grad():
            self._logit_alpha.fill_(math.inf if a >= 1.0 else -math.inf if a <= 0.0 else math.log(a / (1.0 - a)))

    def encode_decode(self, x, dither_rate, dither_dist, soft_round, guess_offset=None, offset=0.0, generator=None):
        """-> (y_dist, x_hat, rates): the latent the synthesis sees, the reconstruction, and the bits per element."""
        if guess_offset is None:
            guess_offset = self.guess_offset
        assert not (guess_offset and soft_round), "guess_offset makes no sense with soft rounding"
        prior = self.prior(soft_round=soft_round)

        def perturb(inputs, dither):
            if dither:
                if soft_round:
                    inputs = round_ops.soft_round(inputs, self.alpha)
                noise = torch.rand(inputs.shape, generator=generator, dtype=self.dtype,
                                   device=inputs.device if generator is None else generator.device)
                inputs = inputs + (noise.to(inputs.device) - 0.5)
                if soft_round:
                    inputs = round_ops.soft_round_conditional_mean(inputs, self.alpha)
                return inputs
            shift = offset
            if guess_offset:
                shift = shift + tfcd.quantization_offset(prior).to(inputs.device)
            return round_ops.round_st(inputs, shift)

        assert x.shape[-1] == self.ndim_source
        y = self.analysis(x)
        y_dist = perturb(y, dither_dist)
        y_rate = y_dist if dither_rate == dither_dist else perturb(y, dither_rate)
        x_hat = self.synthesis(y_dist)
        rates = prior.log_prob(y_rate).sum(dim=-1) / -math.log(2.0)
        return y_dist, x_hat, rates

    def quantize(self, x, **kwargs):
        """The equivalent vector quantiser of this batch: the distinct latents (rows, sorted) index a codebook of
        their reconstructions, which is only valid for these inputs."""
        y_hat, x_hat, rates = self.encode_decode(x, False, False, False, **kwargs)
        flat = y_hat.reshape(-1, self.ndim_latent)
        _, inverse = torch.unique(flat, dim=0, return_inverse=True)
        count = int(inverse.max()) + 1 if inverse.numel() else 0
        rows = torch.arange(flat.shape[0], device=flat.device)
        first = torch.full((count,), flat.shape[0], dtype=torch.int64, device=flat.device)
        first = first.scatter_reduce(0, inverse, rows, "amin")        # what np.unique's return_index gives
        codebook = x_hat.reshape(-1, self.ndim_source)[first]
        rates = rates.reshape(-1)[first]
        return codebook, rates, inverse.to(torch.int32).reshape(x.shape[:-1])

    def train_losses(self, x):
        _, x_hat, rates = self.encode_decode(x, self.dither[0], self.dither[1], self.soft_round[0])
        return rates, self.distortion_fn(x, x_hat)

    def test_losses(self, x):
        _, x_hat, rates = self.encode_decode(x, self.dither[2], self.dither[3], self.soft_round[1])
        return rates, self.distortion_fn(x, x_hat)

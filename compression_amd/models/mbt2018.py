"""Minnen, Ballé and Toderici, "Joint autoregressive and hierarchical priors for learned image compression" (NeurIPS
2018): a mean-scale hyperprior combined with a spatially autoregressive context model.

The reference tree publishes this model's rate-distortion curves (results/image_compression) and lists its
context-free variant (models/tfci.py, `mbt2018-mean`) but carries no program text for it; the layer shapes follow the
paper's table 1, the definition of the context model (ops/context_ops.py, include/tfc_hip.h) and the container layout
are this project's own, and parity with the authors' checkpoints is unpinned.

With `context=True` the entropy parameters of latent position (i, j) come from the hyper-synthesis output psi and the
decoded values above and to the left of it.  Training evaluates that in parallel (teacher forcing on the noisy
latent, `MaskedConv2D` on the convolution kernels); evaluation, `compress` and `decompress` run the serial definition
in one launch each (`context_scan` / `context_decode`): every latent row is a code stream of its own, which is what
lets a wavefront of rows be coded side by side.  With `context=False` the class is the mean-scale hyperprior alone.

    python -m compression_amd.models.mbt2018 --model_path m.pt train --train_glob 'images/*.png'
    python -m compression_amd.models.mbt2018 --model_path m.pt compress in.png out.tfci
    python -m compression_amd.models.mbt2018 --model_path m.pt decompress out.tfci rec.png"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import distributions, entropy_models, layers
from ..ops import context_ops
from .ms2020 import AnalysisTransform, SynthesisTransform

__all__ = ["HyperAnalysisTransform", "HyperSynthesisTransform", "EntropyParameters", "MBT2018Model"]


def _conv(C, k, cin, **kw):
    return layers.SignalConv2D(C, (k, k), padding="same_zeros", in_channels=cin, **kw)


def _lrelu(v):
    return torch.nn.functional.leaky_relu(v, 0.2)


class HyperAnalysisTransform(torch.nn.Module):
    """3x3, 5x5 / 2, 5x5 / 2 as in bmshj2018, on y itself (no abs: the means need the signs)."""

    def __init__(self, latent_depth, num_filters):
        super().__init__()
        kw = dict(corr=True)
        self.layer_0 = _conv(num_filters, 3, latent_depth, strides_down=1, use_bias=True, activation=_lrelu, **kw)
        self.layer_1 = _conv(num_filters, 5, num_filters, strides_down=2, use_bias=True, activation=_lrelu, **kw)
        self.layer_2 = _conv(num_filters, 5, num_filters, strides_down=2, use_bias=False, activation=None, **kw)

    def forward(self, y):
        return self.layer_2(self.layer_1(self.layer_0(y)))


class HyperSynthesisTransform(torch.nn.Module):
    """5x5 x 2, 5x5 x 2, 3x3 with widths M, 3M / 2, 2M (the paper's table 1)."""

    def __init__(self, num_filters, latent_depth):
        super().__init__()
        M = latent_depth
        kw = dict(corr=False, use_bias=True, kernel_parameter="variable")
        self.layer_0 = _conv(M, 5, num_filters, strides_up=2, activation=_lrelu, **kw)
        self.layer_1 = _conv(3 * M // 2, 5, M, strides_up=2, activation=_lrelu, **kw)
        self.layer_2 = _conv(2 * M, 3, 3 * M // 2, strides_up=1, activation=None, **kw)

    def forward(self, z):
        return self.layer_2(self.layer_1(self.layer_0(z)))


class EntropyParameters(torch.nn.Module):
    """Pointwise 4M -> 10M / 3 -> 8M / 3 -> 2M on concat(context features, psi), leaky ReLU (0.2) between.  With a
    `hyper_depth` P other than 2M (a channel group of models/elic2022.py) the input is 2M + P wide and the hidden widths
    keep their thirds between input and output: 2M + 2P // 3 and 2M + P // 3."""

    def __init__(self, latent_depth, hyper_depth=None):
        super().__init__()
        M = latent_depth
        P = 2 * M if hyper_depth is None else int(hyper_depth)
        h1, h2 = 2 * M + 2 * P // 3, 2 * M + P // 3
        kw = dict(corr=True, use_bias=True, kernel_parameter="variable", activation=None)
        self.layer_0 = _conv(h1, 1, 2 * M + P, **kw)
        self.layer_1 = _conv(h2, 1, h1, **kw)
        self.layer_2 = _conv(2 * M, 1, h2, **kw)

    def forward(self, features):
        return self.layer_2(_lrelu(self.layer_1(_lrelu(self.layer_0(features)))))


class HyperpriorContextModel(torch.nn.Module):
    """A mean-scale hyperprior whose entropy parameters come from psi and a context model over decoded values: what
    `MBT2018Model` and `Checkerboard2021Model` share.  A subclass names its context layer and packed-parameter class and
    supplies `_scan`, `_write_strings` and `_read_strings` (and `_check_latent` where a latent can be too small); a
    scheme with more than one context layer (models/elic2022.py) builds its own modules in `_build_context` and supplies
    `_training_parameters` and `context_params` as well.  With `context=False` the class is the hyperprior alone."""

    context_layer = params_class = None

    def __init__(self, lmbda=0.01, num_filters=192, latent_depth=192, context=True, num_scales=64, scale_min=0.11,
                 scale_max=256.0, compute_dtype=torch.float32):
        super().__init__()
        self.lmbda, self.num_scales, self.compute_dtype = lmbda, int(num_scales), compute_dtype
        self.latent_depth, self.context = int(latent_depth), bool(context)
        offset = math.log(scale_min)
        factor = (math.log(scale_max) - math.log(scale_min)) / (num_scales - 1.0)
        self.scale_fn = lambda i: torch.exp(offset + factor * i)
        M = self.latent_depth
        self.analysis_transform = AnalysisTransform(M, num_filters)
        self.synthesis_transform = SynthesisTransform(M, num_filters)
        self.hyper_analysis_transform = HyperAnalysisTransform(M, num_filters)
        self.hyper_synthesis_transform = HyperSynthesisTransform(num_filters, M)
        self.hyperprior = distributions.NoisyDeepFactorized(batch_shape=(num_filters,))
        if self.context:
            self._build_context()
        self.em_y = self.em_z = None
        self._packed = None

    # .tfci layout = decompress()'s signature: three shapes, the z string(s), the y strings
    container_dtypes = [np.int32] * 3 + [bytes] * 2

    @property
    def coding_rank(self):
        return 2 if self.context else 3

    def _models(self, compression):
        em_z = entropy_models.ContinuousBatchedEntropyModel(
            self.hyperprior, coding_rank=3, compression=compression, offset_heuristic=False,
            bottleneck_dtype=self.compute_dtype)
        em_y = entropy_models.LocationScaleIndexedEntropyModel(
            distributions.NoisyNormal, self.num_scales, self.scale_fn, coding_rank=self.coding_rank,
            compression=compression, bottleneck_dtype=torch.float32 if self.context else self.compute_dtype)
        return em_y, em_z

    def init_compression(self):
        self.em_y, self.em_z = self._models(True)
        return self

    def context_params(self):
        """The context model's weights as the kernels take them, packed once per value of the parameters."""
        sources = [self.context_prediction.kernel_variable, self.context_prediction.bias]
        for layer in (self.entropy_parameters.layer_0, self.entropy_parameters.layer_1, self.entropy_parameters.layer_2):
            sources += [layer.kernel_variable, layer.bias]
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in sources)
        if self._packed is None or self._packed[0] != key:
            ep = self.entropy_parameters
            params = self.params_class.from_layers(self.context_prediction, (ep.layer_0, ep.layer_1, ep.layer_2),
                                                   self.num_scales)
            self._packed = (key, params)
        return self._packed[1]

    def _psi(self, z_hat, y_shape):
        return self.hyper_synthesis_transform(z_hat)[:, :y_shape[0], :y_shape[1], :].contiguous()

    # --- what a context scheme supplies -------------------------------------------------------------------------------
    def _build_context(self):
        """Creates the context modules; a scheme with other modules also overrides `context_params` and
        `_training_parameters`."""
        self.context_prediction = self.context_layer(2 * self.latent_depth, self.latent_depth)
        self.entropy_parameters = EntropyParameters(self.latent_depth)

    def _training_parameters(self, y_tilde, psi):
        """(mu, indexes) of every position in parallel, teacher-forced on the noisy latent."""
        M = self.latent_depth
        out = self.entropy_parameters(torch.cat([self.context_prediction(y_tilde), psi], dim=-1))
        return out[..., :M].contiguous(), out[..., M:].contiguous()

    def _check_latent(self, y_shape):
        """Raises for a latent the scheme cannot code."""

    def _scan(self, y, psi, params):
        """float32 y and psi -> the scheme's scan tuple (mu, index_float, y_hat, ...), full layout."""
        raise NotImplementedError

    def _write_strings(self, y, scan):
        """The y strings of `compress` from the float32 latent and its scan."""
        raise NotImplementedError

    def _read_strings(self, y_strings, psi, batch, y_shape):
        """The flat y strings of `decompress` -> y_hat; raises when their count is not the scheme's."""
        raise NotImplementedError

    # --- the three places where the context scheme meets the entropy model; a scheme whose likelihood is not
    # (mu, indexes) over the table set (models/cstk2020.py) overrides these and `_models` instead of the four above ------
    def _rate_context(self, em_y, y, psi, training):
        """(y_bits, y_hat) of `forward` with the context model."""
        if training:
            # one noise sample: the same y + u feeds the context convolution, the rate and the synthesis
            u = torch.rand_like(y) - 0.5
            y_tilde = y + u
            mu, indexes = self._training_parameters(y_tilde, psi)
            _, y_bits = em_y(y.float(), indexes.float(), loc=mu.float(), training=True, noise=u.float())
            return y_bits, y_tilde
        scan = self._scan(y.float(), psi.float(), self.context_params())
        _, y_bits = em_y(y.float(), scan.index_float, loc=scan.mu, training=False)
        return y_bits, scan.y_hat.to(self.compute_dtype)

    def _compress_context(self, y, psi):
        """(y_strings, y_hat, extras) of `compress`: `extras` is a tuple of further int32 container entries, stored
        between the shapes and the strings and handed back to `_decompress_context`."""
        y = y.float().contiguous()
        scan = self._scan(y, psi.float(), self.context_params())
        return self._write_strings(y, scan), scan.y_hat, ()

    def _decompress_context(self, y_strings, psi, batch, y_shape, extras):
        """y_hat of `decompress` from the y strings as the container holds them."""
        y_strings = np.asarray(y_strings, dtype=object).reshape(-1)
        return self._read_strings(y_strings, psi.float(), batch, y_shape)

    # ------------------------------------------------------------------------------------------------------------------
    def forward(self, x, training=True, return_y_hat=False):
        """x [B, H, W, 3] on the 0...255 scale -> (loss, bpp, mse) (and y_hat on request)."""
        em_y, em_z = self._models(False)
        x = x.to(self.compute_dtype)
        M = self.latent_depth
        y = self.analysis_transform(x)
        y_shape = tuple(y.shape[1:-1])
        self._check_latent(y_shape)
        z = self.hyper_analysis_transform(y)
        num_pixels = x.shape[0] * x.shape[1] * x.shape[2]
        _, z_bits = em_z(z, training=training)
        z_hat = em_z.quantize(z).to(self.compute_dtype)
        psi = self._psi(z_hat, y_shape)
        if not self.context:
            means, indexes = psi[..., :M].contiguous(), psi[..., M:].contiguous()
            _, y_bits = em_y(y, indexes, loc=means, training=training)
            y_hat = em_y.quantize(y, loc=means).to(self.compute_dtype)
        else:
            y_bits, y_hat = self._rate_context(em_y, y, psi, training)
        x_hat = self.synthesis_transform(y_hat)[:, :x.shape[1], :x.shape[2], :]
        bpp = (y_bits.sum() + z_bits.sum()) / num_pixels
        mse = torch.mean((x.float() - x_hat.float()) ** 2).to(bpp.dtype)
        out = (bpp + self.lmbda * mse, bpp, mse)
        return out + (y_hat,) if return_y_hat else out

    def _reconstruct(self, y_hat, x_shape):
        x_hat = self.synthesis_transform(y_hat.to(self.compute_dtype))[:, :x_shape[0], :x_shape[1], :]
        return torch.clamp(torch.round(x_hat.float()), 0, 255).to(torch.uint8)

    @torch.no_grad()
    def compress(self, x, return_reconstruction=False):
        """uint8 [B, H, W, 3] (or [H, W, 3]) -> (x_shape, y_shape, z_shape, z_string, y_strings); with
        `return_reconstruction` also the encoder's own closed-loop reconstruction, uint8 [B, H, W, 3]."""
        if self.em_y is None:
            raise RuntimeError("compress needs init_compression()")
        if x.dim() == 3:
            x = x[None]
        x = x.to(self.compute_dtype)
        M = self.latent_depth
        y = self.analysis_transform(x)
        z = self.hyper_analysis_transform(y)
        x_shape, y_shape, z_shape = tuple(x.shape[1:-1]), tuple(y.shape[1:-1]), tuple(z.shape[1:-1])
        self._check_latent(y_shape)
        z_string = self.em_z.compress(z)
        # the closed loop uses quantize() in place of a decode of the string (as ms2020's compress does)
        z_hat = self.em_z.quantize(z).to(self.compute_dtype)
        psi = self._psi(z_hat, y_shape)
        extras = ()
        if self.context:
            y_strings, y_hat, extras = self._compress_context(y, psi)
        else:
            means, indexes = psi[..., :M].contiguous(), psi[..., M:].contiguous()
            y_strings = self.em_y.compress(y, indexes, loc=means)
            y_hat = self.em_y.quantize(y, loc=means)
        packed = (x_shape, y_shape, z_shape) + tuple(extras) + (z_string, y_strings)
        return packed + (self._reconstruct(y_hat, x_shape),) if return_reconstruction else packed

    def decompress(self, x_shape, y_shape, z_shape, z_string, y_strings):
        """The arguments `compress` returned -> uint8 [B, H, W, 3]."""
        return self._decompress(x_shape, y_shape, z_shape, z_string, y_strings, ())

    @torch.no_grad()
    def _decompress(self, x_shape, y_shape, z_shape, z_string, y_strings, extras):
        if self.em_y is None:
            raise RuntimeError("decompress needs init_compression()")
        x_shape, y_shape, z_shape = (tuple(int(v) for v in s) for s in (x_shape, y_shape, z_shape))
        self._check_latent(y_shape)
        M = self.latent_depth
        z_string = np.asarray(z_string, dtype=object).reshape(-1)
        z_hat = self.em_z.decompress(z_string, z_shape).to(self.compute_dtype)
        batch = z_hat.shape[0]
        psi = self._psi(z_hat, y_shape)
        if self.context:
            y_hat = self._decompress_context(y_strings, psi, batch, y_shape, extras)
        else:
            y_strings = np.asarray(y_strings, dtype=object).reshape(-1)
            means, indexes = psi[..., :M].contiguous(), psi[..., M:].contiguous()
            y_hat = self.em_y.decompress(y_strings, indexes, loc=means)
        return self._reconstruct(y_hat, x_shape)


class MBT2018Model(HyperpriorContextModel):
    """compress() returns (x_shape, y_shape, z_shape, z_string [B], y_strings); with the context model y_strings holds
    one string per latent row, [B * Hl], image after image; without it one per image, [B]."""

    context_layer, params_class = layers.MaskedConv2D, context_ops.ContextParams

    def _scan(self, y, psi, params):
        return context_ops.context_scan(y, psi, params)

    def _write_strings(self, y, scan):
        return self.em_y.compress((y - scan.mu).contiguous(), scan.index_float).reshape(-1)

    def _read_strings(self, y_strings, psi, batch, y_shape):
        if y_strings.shape[0] != batch * y_shape[0]:
            raise ValueError(f"{batch * y_shape[0]} row strings are needed for {batch} image(s) of {y_shape[0]} "
                             f"latent rows, received {y_strings.shape[0]}")
        y_hat, ok = context_ops.context_decode(y_strings.reshape(batch, y_shape[0]), psi, self.context_params(),
                                               self.em_y.cdf, self.em_y.cdf_offset)
        if self.em_y.decode_sanity_check and not bool(ok.all()):
            raise RuntimeError("Sanity check failed.")
        return y_hat


if __name__ == "__main__":      # python -m compression_amd.models.mbt2018 compress in.png out.tfci
    import sys

    from .codec_io import main
    sys.exit(main(MBT2018Model))

"""Cheng, Sun, Takeuchi and Katto, "Learned image compression with discretized Gaussian mixture likelihoods and attention
modules" (CVPR 2020): the latent's likelihood is a mixture of K Gaussians per element, K weights, means and scales.

The reference tree holds no program text for this model.  This is the mixture likelihood on the transforms and the
hyperprior of models/mbt2018.py with a checkerboard context (models/checkerboard2021.py) in place of the paper's serial
one; the paper's residual blocks and attention modules are out of scope.  The definition is this project's own, parity
with anyone's checkpoints is unpinned.

No table set spans 3 K parameters per element, so the strings come from the coder that evaluates every element's CDF
where it codes it (`entropy_models.GaussianMixtureEntropyModel`, csrc/mixture_coder.hip), and the training rate from the
fused likelihood (csrc/mixture_bits.hip).  y_hat = round(y) on both sides: no mean is subtracted.

The checkerboard runs as two passes at host level.  Pass 0 codes the anchors (i + j even) with parameters from psi alone
(their context features are zero); pass 1 codes the other positions with parameters from psi and `CheckerboardConv2D`
over the decoded anchors.  Each pass gathers its positions into [B, N_p, M] and is one `compress` / `decompress` call of
the mixture model.  Strings decode on the build and device kind that encoded them, as for mbt2018; whether an image coded
in a batch also decodes alone depends on the convolution kernels giving a position the same value in both batches and is
tested (tests/test_cstk2020_gpu.py), not guaranteed.

    python -m compression_amd.models.cstk2020 --model_path m.pt train --train_glob 'images/*.png'
    python -m compression_amd.models.cstk2020 --model_path m.pt compress in.png out.tfci
    python -m compression_amd.models.cstk2020 --model_path m.pt decompress out.tfci rec.png"""
from __future__ import annotations

import numpy as np
import torch

from .. import entropy_models, layers
from ..ops import math_ops
from ..ops.checkerboard_ops import anchor_mask
from .mbt2018 import HyperpriorContextModel, _conv, _lrelu

__all__ = ["MixtureEntropyParameters", "CSTK2020Model"]


class MixtureEntropyParameters(torch.nn.Module):
    """Pointwise 4M -> h1 -> h2 -> 3 K M on concat(context features, psi), leaky ReLU (0.2) between; the hidden widths
    keep their thirds between input and output."""

    def __init__(self, latent_depth, num_components):
        super().__init__()
        cin, cout = 4 * latent_depth, 3 * num_components * latent_depth
        h1, h2 = (2 * cin + cout) // 3, (cin + 2 * cout) // 3
        kw = dict(corr=True, use_bias=True, kernel_parameter="variable", activation=None)
        self.layer_0 = _conv(h1, 1, cin, **kw)
        self.layer_1 = _conv(h2, 1, h1, **kw)
        self.layer_2 = _conv(cout, 1, h2, **kw)

    def forward(self, features):
        return self.layer_2(_lrelu(self.layer_1(_lrelu(self.layer_0(features)))))


def pass_positions(hl, wl, device=None):
    """The flat positions i * wl + j of pass 0 (i + j even) and of pass 1, each in raster order."""
    anchors = anchor_mask(hl, wl, device).reshape(-1)
    index = torch.arange(hl * wl, device=device)
    return index[anchors], index[~anchors]


class CSTK2020Model(HyperpriorContextModel):
    """compress() returns (x_shape, y_shape, z_shape, windows, z_string [B], y_strings): `windows` holds (lo, L) of pass
    0 and of pass 1 of every image, int32 [B * 4]; y_strings holds S_0 + S_1 strings per image in the order pass,
    stream, image after image, S_p = ceil(N_p M / stream_symbols) with N_0 = ceil(Hl Wl / 2), N_1 = floor(Hl Wl / 2)."""

    # .tfci layout = decompress()'s signature: three shapes, the windows, the z string(s), the y strings
    container_dtypes = [np.int32] * 4 + [bytes] * 2

    def __init__(self, lmbda=0.01, num_filters=192, latent_depth=192, num_components=3, stream_symbols=1024,
                 scale_min=0.11, compute_dtype=torch.float32):
        self.num_components, self.stream_symbols, self.scale_min = int(num_components), int(stream_symbols), scale_min
        # validates K and stream_symbols before any module is built
        entropy_models.GaussianMixtureEntropyModel(self.num_components, 2, self.stream_symbols)
        super().__init__(lmbda, num_filters, latent_depth, True, compute_dtype=compute_dtype)

    def _build_context(self):
        M = self.latent_depth
        self.context_prediction = layers.CheckerboardConv2D(2 * M, M, use_bias=False)
        self.entropy_parameters = MixtureEntropyParameters(M, self.num_components)

    def _models(self, compression):
        em_z = entropy_models.ContinuousBatchedEntropyModel(
            self.hyperprior, coding_rank=3, compression=compression, offset_heuristic=False,
            bottleneck_dtype=self.compute_dtype)
        em_y = entropy_models.GaussianMixtureEntropyModel(
            self.num_components, coding_rank=2, stream_symbols=self.stream_symbols, compression=compression,
            bottleneck_dtype=torch.float32)
        return em_y, em_z

    def context_params(self):
        raise NotImplementedError("the mixture model runs its context at host level: there are no packed weights")

    def _check_latent(self, y_shape):
        if y_shape[0] * y_shape[1] < 2:
            raise ValueError(f"a latent of {y_shape[0]} x {y_shape[1]} has no second pass: the checkerboard model needs "
                             "at least two latent positions (an image larger than 16 x 16)")

    def stream_counts(self, y_shape):
        """(S_0, S_1): the strings of pass 0 and of pass 1 of one image."""
        n = y_shape[0] * y_shape[1]
        return tuple(-(-(count * self.latent_depth) // self.stream_symbols) for count in ((n + 1) // 2, n // 2))

    # --- parameters ---------------------------------------------------------------------------------------------------
    def _mixture_parameters(self, ctx, psi):
        """Context features and psi, [B, Hl, Wl, 2M] each -> float32 (logits, loc, scale), [B, Hl, Wl, M, K] each."""
        out = self.entropy_parameters(torch.cat([ctx, psi], dim=-1)).float()
        out = out.reshape(*out.shape[:-1], 3, self.latent_depth, self.num_components)
        scale = math_ops.lower_bound(out[..., 2, :, :], self.scale_min)
        return out[..., 0, :, :].contiguous(), out[..., 1, :, :].contiguous(), scale.contiguous()

    def _pass_parameters(self, psi, anchors_hat, positions):
        """The parameters of one pass at its positions, [B, N_p, M, K] each: pass 0 with `anchors_hat` None (zero context
        features), pass 1 with the decoded anchors [B, Hl, Wl, M] (zeros elsewhere).  `compress` and `decompress` both
        come through here, with the same shapes.  The network runs over the whole latent in both passes and half of it
        is kept: twice the work a gather in front of the pointwise layers would need, on purpose, so that both sides
        and both passes call the convolution kernels at one shape and a position's value cannot depend on which tile
        of a gathered tensor it lands in."""
        if anchors_hat is None:
            ctx = torch.zeros_like(psi)
        else:
            ctx = self.context_prediction(anchors_hat.to(psi.dtype))
        b = psi.shape[0]
        return tuple(t.reshape(b, -1, *t.shape[3:])[:, positions].contiguous()
                     for t in self._mixture_parameters(ctx, psi))

    # --- the base class's three hooks ---------------------------------------------------------------------------------
    def _rate_context(self, em_y, y, psi, training):
        if training:
            # one noise sample: the same y + u feeds the context convolution, the rate and the synthesis
            u = torch.rand_like(y) - 0.5
            y_hat = y + u
            params = self._mixture_parameters(self.context_prediction(y_hat), psi)
            _, y_bits = em_y(y.float(), *params, training=True, noise=u.float())
            return y_bits, y_hat
        y_hat = em_y.quantize(y.float())
        others = (~anchor_mask(y.shape[1], y.shape[2], y.device)).to(y_hat.dtype)[:, :, None]
        # pass 1 sees the anchors alone, as the decoder does; the layer zeroes the features of the anchors themselves
        params = self._mixture_parameters(self.context_prediction((y_hat * (1 - others)).to(psi.dtype)), psi)
        _, y_bits = em_y(y_hat, *params, training=False)
        return y_bits, y_hat.to(self.compute_dtype)

    def _compress_context(self, y, psi):
        b, hl, wl, m = y.shape
        y_flat = y.float().reshape(b, hl * wl, m)
        y_hat = torch.zeros_like(y_flat)
        strings, windows, anchors_hat = [], [], None
        for positions in pass_positions(hl, wl, y.device):
            params = self._pass_parameters(psi, anchors_hat, positions)
            y_pass = y_flat[:, positions].contiguous()
            s, window = self.em_y.compress(y_pass, *params)
            y_hat[:, positions] = self.em_y.quantize(y_pass, window)
            strings.append(s.reshape(b, -1))
            windows.append(window)
            anchors_hat = y_hat.reshape(b, hl, wl, m).clone()
        # image, pass, stream; (lo, L) of pass 0, then of pass 1, image after image
        y_strings = np.concatenate(strings, axis=1).reshape(-1)
        windows = np.stack(windows, axis=1).astype(np.int32).reshape(-1)
        return y_strings, y_hat.reshape(b, hl, wl, m), (windows,)

    def _decompress_context(self, y_strings, psi, batch, y_shape, extras):
        hl, wl = y_shape
        m = self.latent_depth
        y_strings = np.asarray(y_strings, dtype=object).reshape(-1)
        counts = self.stream_counts(y_shape)
        if y_strings.shape[0] != batch * sum(counts):
            raise ValueError(f"{batch * sum(counts)} stream strings are needed for {batch} image(s) ({counts[0]} + "
                             f"{counts[1]} streams of {self.stream_symbols} symbols), received {y_strings.shape[0]}")
        windows = np.asarray(extras[0], dtype=np.int64).reshape(-1)
        if windows.size != batch * 4:
            raise ValueError(f"{batch * 4} window values are needed for {batch} image(s) ((lo, L) of pass 0 and of pass "
                             f"1), received {windows.size}")
        windows = windows.reshape(batch, 2, 2)
        y_strings = y_strings.reshape(batch, sum(counts))
        y_hat = torch.zeros(batch, hl * wl, m, dtype=torch.float32, device=psi.device)
        anchors_hat, first = None, 0
        for p, positions in enumerate(pass_positions(hl, wl, psi.device)):
            params = self._pass_parameters(psi, anchors_hat, positions)
            s = y_strings[:, first:first + counts[p]].reshape(-1)
            y_hat[:, positions] = self.em_y.decompress(s, windows[:, p], *params)
            first += counts[p]
            anchors_hat = y_hat.reshape(batch, hl, wl, m).clone()
        return y_hat.reshape(batch, hl, wl, m)

    def decompress(self, x_shape, y_shape, z_shape, windows, z_string, y_strings):
        """The arguments `compress` returned -> uint8 [B, H, W, 3]."""
        return self._decompress(x_shape, y_shape, z_shape, z_string, y_strings, (windows,))


if __name__ == "__main__":      # python -m compression_amd.models.cstk2020 compress in.png out.tfci
    import sys

    from .codec_io import main
    sys.exit(main(CSTK2020Model))

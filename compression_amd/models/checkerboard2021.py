"""He, Zheng, Sun, Wang and Qin, "Checkerboard context model for efficient learned image compression" (CVPR 2021) on
the transforms, hyperprior and entropy-parameter network of models/mbt2018.py: the serial scan of the joint
autoregressive prior is replaced by two passes that are parallel over positions.

The reference tree holds no program text for this model.  The layer shapes are mbt2018's (the paper's table 1 of
Minnen et al.), the definition of the context model (ops/checkerboard_ops.py, include/tfc_hip.h) and the container
layout are this project's own, and parity with anyone's checkpoints is unpinned.

Half of the latent positions, the anchors (i + j even), are coded from the hyperprior alone; the others see the 12
decoded anchors of their 5x5 window as well.  Training evaluates that in parallel (teacher forcing on the noisy
latent, `CheckerboardConv2D` on the convolution kernels); evaluation, `compress` and `decompress` run the definition
in one launch per pass (`checkerboard_scan` / `checkerboard_decode`), and every image carries two code streams.

    python -m compression_amd.models.checkerboard2021 --model_path m.pt train --train_glob 'images/*.png'
    python -m compression_amd.models.checkerboard2021 --model_path m.pt compress in.png out.tfci
    python -m compression_amd.models.checkerboard2021 --model_path m.pt decompress out.tfci rec.png"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import distributions, entropy_models, layers
from ..ops import checkerboard_ops
from .mbt2018 import EntropyParameters, HyperAnalysisTransform, HyperSynthesisTransform
from .ms2020 import AnalysisTransform, SynthesisTransform

__all__ = ["Checkerboard2021Model"]


class Checkerboard2021Model(torch.nn.Module):
    """compress() returns (x_shape, y_shape, z_shape, z_string [B], y_strings [2 B]): per image the string of pass 0
    (the anchors), then the string of pass 1, image after image."""

    def __init__(self, lmbda=0.01, num_filters=192, latent_depth=192, num_scales=64, scale_min=0.11, scale_max=256.0,
                 compute_dtype=torch.float32):
        super().__init__()
        self.lmbda, self.num_scales, self.compute_dtype = lmbda, int(num_scales), compute_dtype
        self.latent_depth = int(latent_depth)
        offset = math.log(scale_min)
        factor = (math.log(scale_max) - math.log(scale_min)) / (num_scales - 1.0)
        self.scale_fn = lambda i: torch.exp(offset + factor * i)
        M = self.latent_depth
        self.analysis_transform = AnalysisTransform(M, num_filters)
        self.synthesis_transform = SynthesisTransform(M, num_filters)
        self.hyper_analysis_transform = HyperAnalysisTransform(M, num_filters)
        self.hyper_synthesis_transform = HyperSynthesisTransform(num_filters, M)
        self.hyperprior = distributions.NoisyDeepFactorized(batch_shape=(num_filters,))
        self.context_prediction = layers.CheckerboardConv2D(2 * M, M)
        self.entropy_parameters = EntropyParameters(M)
        self.em_y = self.em_z = None
        self._packed = None

    # .tfci layout = decompress()'s signature: three shapes, the z string(s), the y strings
    container_dtypes = [np.int32] * 3 + [bytes] * 2

    def _models(self, compression):
        em_z = entropy_models.ContinuousBatchedEntropyModel(
            self.hyperprior, coding_rank=3, compression=compression, offset_heuristic=False,
            bottleneck_dtype=self.compute_dtype)
        em_y = entropy_models.LocationScaleIndexedEntropyModel(
            distributions.NoisyNormal, self.num_scales, self.scale_fn, coding_rank=2, compression=compression,
            bottleneck_dtype=torch.float32)
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
            params = checkerboard_ops.CheckerboardParams.from_layers(
                self.context_prediction, (ep.layer_0, ep.layer_1, ep.layer_2), self.num_scales)
            self._packed = (key, params)
        return self._packed[1]

    def _psi(self, z_hat, y_shape):
        return self.hyper_synthesis_transform(z_hat)[:, :y_shape[0], :y_shape[1], :].contiguous()

    @staticmethod
    def _check_latent(y_shape):
        if y_shape[0] * y_shape[1] < 2:
            raise ValueError(f"a latent of {y_shape[0]} x {y_shape[1]} has no second pass: the checkerboard model needs "
                             "at least two latent positions (an image larger than 16 x 16)")

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
        if training:
            # one noise sample: the same y + u feeds the context convolution, the rate and the synthesis
            u = torch.rand_like(y) - 0.5
            y_tilde = y + u
            out = self.entropy_parameters(torch.cat([self.context_prediction(y_tilde), psi], dim=-1))
            mu, indexes = out[..., :M].contiguous(), out[..., M:].contiguous()
            _, y_bits = em_y(y.float(), indexes.float(), loc=mu.float(), training=True, noise=u.float())
            y_hat = y_tilde
        else:
            scan = checkerboard_ops.checkerboard_scan(y.float(), psi.float(), self.context_params())
            _, y_bits = em_y(y.float(), scan.index_float, loc=scan.mu, training=False)
            y_hat = scan.y_hat.to(self.compute_dtype)
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
        y = self.analysis_transform(x)
        z = self.hyper_analysis_transform(y)
        x_shape, y_shape, z_shape = tuple(x.shape[1:-1]), tuple(y.shape[1:-1]), tuple(z.shape[1:-1])
        self._check_latent(y_shape)
        z_string = self.em_z.compress(z)
        # the closed loop uses quantize() in place of a decode of the string (as ms2020's compress does)
        z_hat = self.em_z.quantize(z).to(self.compute_dtype)
        psi = self._psi(z_hat, y_shape)
        y = y.float().contiguous()
        scan = checkerboard_ops.checkerboard_scan(y, psi.float(), self.context_params())
        residual = checkerboard_ops.checkerboard_split(y - scan.mu)
        index = checkerboard_ops.checkerboard_split(scan.index_float)
        per_pass = [np.asarray(self.em_y.compress(r, i), dtype=object).reshape(-1) for r, i in zip(residual, index)]
        y_strings = np.stack(per_pass, axis=1).reshape(-1)            # [B, 2] -> pass 0, pass 1 of image 0, of image 1...
        packed = (x_shape, y_shape, z_shape, z_string, y_strings)
        return packed + (self._reconstruct(scan.y_hat, x_shape),) if return_reconstruction else packed

    @torch.no_grad()
    def decompress(self, x_shape, y_shape, z_shape, z_string, y_strings):
        """The arguments `compress` returned -> uint8 [B, H, W, 3]."""
        if self.em_y is None:
            raise RuntimeError("decompress needs init_compression()")
        x_shape, y_shape, z_shape = (tuple(int(v) for v in s) for s in (x_shape, y_shape, z_shape))
        self._check_latent(y_shape)
        z_string = np.asarray(z_string, dtype=object).reshape(-1)
        z_hat = self.em_z.decompress(z_string, z_shape).to(self.compute_dtype)
        batch = z_hat.shape[0]
        psi = self._psi(z_hat, y_shape)
        y_strings = np.asarray(y_strings, dtype=object).reshape(-1)
        if y_strings.shape[0] != 2 * batch:
            raise ValueError(f"{2 * batch} pass strings are needed for {batch} image(s) (pass 0 and pass 1 of each), "
                             f"received {y_strings.shape[0]}")
        y_hat = checkerboard_ops.checkerboard_decode(y_strings.reshape(batch, 2), psi.float(), self.context_params(),
                                                     self.em_y)
        return self._reconstruct(y_hat, x_shape)


if __name__ == "__main__":      # python -m compression_amd.models.checkerboard2021 compress in.png out.tfci
    import sys

    from .codec_io import main
    sys.exit(main(Checkerboard2021Model))

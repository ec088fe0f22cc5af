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

import torch

from .. import layers
from ..ops import checkerboard_ops
from .mbt2018 import HyperpriorContextModel

__all__ = ["Checkerboard2021Model"]


class Checkerboard2021Model(HyperpriorContextModel):
    """compress() returns (x_shape, y_shape, z_shape, z_string [B], y_strings [2 B]): per image the string of pass 0
    (the anchors), then the string of pass 1, image after image."""

    context_layer, params_class = layers.CheckerboardConv2D, checkerboard_ops.CheckerboardParams

    def __init__(self, lmbda=0.01, num_filters=192, latent_depth=192, num_scales=64, scale_min=0.11, scale_max=256.0,
                 compute_dtype=torch.float32):
        super().__init__(lmbda, num_filters, latent_depth, True, num_scales, scale_min, scale_max, compute_dtype)

    def _check_latent(self, y_shape):
        if y_shape[0] * y_shape[1] < 2:
            raise ValueError(f"a latent of {y_shape[0]} x {y_shape[1]} has no second pass: the checkerboard model needs "
                             "at least two latent positions (an image larger than 16 x 16)")

    def _scan(self, y, psi, params):
        return checkerboard_ops.checkerboard_scan(y, psi, params)

    def _write_strings(self, y, scan):
        # [B, 2] -> pass 0, pass 1 of image 0, of image 1...
        return checkerboard_ops.checkerboard_encode(y, scan, self.em_y).reshape(-1)

    def _read_strings(self, y_strings, psi, batch, y_shape):
        if y_strings.shape[0] != 2 * batch:
            raise ValueError(f"{2 * batch} pass strings are needed for {batch} image(s) (pass 0 and pass 1 of each), "
                             f"received {y_strings.shape[0]}")
        return checkerboard_ops.checkerboard_decode(y_strings.reshape(batch, 2), psi, self.context_params(), self.em_y)


if __name__ == "__main__":      # python -m compression_amd.models.checkerboard2021 compress in.png out.tfci
    import sys

    from .codec_io import main
    sys.exit(main(Checkerboard2021Model))

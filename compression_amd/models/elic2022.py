"""The space-channel context model of He, Yang, Peng, Mao, Qin and Wang, "ELIC: efficient learned image compression
with unevenly grouped space-channel contextual adaptive coding" (CVPR 2022) on the transforms and hyperprior of
models/mbt2018.py: the latent's channels are cut into unevenly sized groups, the checkerboard of
models/checkerboard2021.py runs inside every group, and a group also sees all earlier groups.

The reference tree holds no program text for this model.  The transforms and the hyperprior are mbt2018's (ELIC's
residual-bottleneck and attention transforms are not built), the definition of the context model
(ops/scctx_ops.py, include/tfc_hip.h), the stream format and the layer shapes are this project's own, and parity
with anyone's checkpoints is unpinned.

Per group g of M_g channels that start at channel c_g: a plain 5x5 `SignalConv2D` without bias over the channels below
c_g (none for group 0), a `CheckerboardConv2D` over the group's own channels, and an `EntropyParameters` network on
[their sum, psi] with the hidden widths 2 M_g + 2 P // 3 and 2 M_g + P // 3.  Training evaluates all groups in parallel
(teacher forcing on the noisy latent, on the convolution kernels with autograd); evaluation, `compress` and
`decompress` run the definition in one launch per (group, pass) (`scctx_scan` / `scctx_decode`).  Every (group, pass)
of an image is cut into streams of `stream_positions` positions that decode side by side; `stream_positions` is part
of the configuration, like `num_scales`, and is not written into the container.

    python -m compression_amd.models.elic2022 --model_path m.pt train --train_glob 'images/*.png'
    python -m compression_amd.models.elic2022 --model_path m.pt compress in.png out.tfci
    python -m compression_amd.models.elic2022 --model_path m.pt decompress out.tfci rec.png"""
from __future__ import annotations

import torch

from .. import layers
from ..ops import scctx_ops
from .mbt2018 import EntropyParameters, HyperpriorContextModel

__all__ = ["ELIC2022Model"]


class ELIC2022Model(HyperpriorContextModel):
    """compress() returns (x_shape, y_shape, z_shape, z_string [B], y_strings [B T]) with T = G (S_0 + S_1) strings per
    image in the order group, pass, stream, image after image (S_p = ceil(N_p / stream_positions)).  `groups` defaults
    to the widths 16, 16, 32, 64 and then the rest of `latent_depth`."""

    def __init__(self, lmbda=0.01, num_filters=192, latent_depth=192, groups=None, stream_positions=64, num_scales=64,
                 scale_min=0.11, scale_max=256.0, compute_dtype=torch.float32):
        groups = scctx_ops.default_groups(latent_depth) if groups is None else groups
        self.groups = scctx_ops._check_groups(groups, latent_depth)
        self.stream_positions = scctx_ops._check_stream_positions(stream_positions)
        super().__init__(lmbda, num_filters, latent_depth, True, num_scales, scale_min, scale_max, compute_dtype)

    def _build_context(self):
        M, offsets = self.latent_depth, [sum(self.groups[:g]) for g in range(len(self.groups))]
        self.group_offsets = offsets
        # group g > 0 sees the channels below c_g through the whole window: entry g - 1 of the list
        self.channel_context = torch.nn.ModuleList(
            layers.SignalConv2D(2 * mg, (5, 5), corr=True, padding="same_zeros", use_bias=False, in_channels=c,
                                kernel_parameter="variable")
            for c, mg in zip(offsets[1:], self.groups[1:]))
        self.space_context = torch.nn.ModuleList(layers.CheckerboardConv2D(2 * mg, mg) for mg in self.groups)
        self.entropy_parameters = torch.nn.ModuleList(EntropyParameters(mg, hyper_depth=2 * M) for mg in self.groups)

    def _channel_context(self, g):
        return self.channel_context[g - 1] if g else None

    def _training_parameters(self, y_tilde, psi):
        mus, indexes = [], []
        for g, (c, mg) in enumerate(zip(self.group_offsets, self.groups)):
            ctx = self.space_context[g](y_tilde[..., c:c + mg].contiguous())
            if g:
                ctx = ctx + self._channel_context(g)(y_tilde[..., :c].contiguous())
            out = self.entropy_parameters[g](torch.cat([ctx, psi], dim=-1))
            mus.append(out[..., :mg])
            indexes.append(out[..., mg:])
        return torch.cat(mus, dim=-1).contiguous(), torch.cat(indexes, dim=-1).contiguous()

    def context_params(self):
        """The context model's weights as the kernels take them, packed once per value of the parameters."""
        modules = (self.channel_context, self.space_context, self.entropy_parameters)
        sources = [t for module in modules for t in module.parameters()]
        key = tuple((t.data_ptr(), t._version, str(t.device)) for t in sources)
        if self._packed is None or self._packed[0] != key:
            count = range(len(self.groups))
            params = scctx_ops.SpaceChannelParams.from_layers(
                [self._channel_context(g) for g in count], self.space_context,
                [(ep.layer_0, ep.layer_1, ep.layer_2) for ep in self.entropy_parameters], self.num_scales,
                self.stream_positions)
            if not params.fits_kernel():
                raise ValueError(f"the groups {self.groups} at a latent depth of {self.latent_depth} hold a group whose "
                                 "activations do not fit the kernel's LDS (ops/scctx_ops.py, fits_kernel): choose "
                                 "narrower groups")
            self._packed = (key, params)
        return self._packed[1]

    def _check_latent(self, y_shape):
        if y_shape[0] * y_shape[1] < 2:
            raise ValueError(f"a latent of {y_shape[0]} x {y_shape[1]} has no second pass: the space-channel model needs "
                             "at least two latent positions (an image larger than 16 x 16)")

    def _scan(self, y, psi, params):
        return scctx_ops.scctx_scan(y, psi, params)

    def _write_strings(self, y, scan):
        return scctx_ops.scctx_encode(y, scan, self.context_params(), self.em_y).reshape(-1)

    def _read_strings(self, y_strings, psi, batch, y_shape):
        counts = scctx_ops.stream_counts(y_shape[0], y_shape[1], self.stream_positions)
        per_image = len(self.groups) * sum(counts)
        if y_strings.shape[0] != batch * per_image:
            raise ValueError(f"{batch * per_image} stream strings are needed for {batch} image(s) ({len(self.groups)} "
                             f"groups x ({counts[0]} + {counts[1]}) streams of {self.stream_positions} positions each), "
                             f"received {y_strings.shape[0]}")
        return scctx_ops.scctx_decode(y_strings.reshape(batch, per_image), psi, self.context_params(), self.em_y)


if __name__ == "__main__":      # python -m compression_amd.models.elic2022 compress in.png out.tfci
    import sys

    from .codec_io import main
    sys.exit(main(ELIC2022Model))

"""LPIPS with the AlexNet trunk (Zhang et al. 2018, "The Unreasonable Effectiveness of Deep Features as a Perceptual
Metric", version 0.1), HiFiC's perceptual loss (models/hific/model.py:840-872, which loads it as the frozen graph
`net-lin_alex_v0.1`), on this library's convolution kernels, `max_pool2d` and `lpips_distance`.

Inputs `fake`, `real` [N, H, W, 3], channels last, values in [0, 1]:
  1. x = 2 img - 1, then (x - shift) / scale per channel.
  2. Cross-correlations with zero padding, each with a bias and a ReLU behind it:
       conv1 3 -> 64, 11 x 11, stride 4, pad 2;  max-pool 3 x 3 stride 2
       conv2 64 -> 192, 5 x 5, pad 2;            max-pool 3 x 3 stride 2
       conv3 192 -> 384, conv4 384 -> 256, conv5 256 -> 256, 3 x 3, pad 1
     The five taps are the ReLU outputs of conv1 ... conv5.
  3. Per tap, `functional.lpips_distance` with the tap's weights `lin` >= 0 and eps = 1e-10.
  4. lpips[image] = the sum of the five distances.
The smallest side is 31: 7 -> 3 -> 1 through conv1 and the pools.

conv1 on the kernels: `conv2d_down` at stride 4 computes y[j] = sum_t x[4 j + t - 5] w[t] per axis (pad 11 // 2 = 5);
pad 2 wants x[4 i + t - 2].  With ONE zero row / column in front (x' [m] = x[m - 1]) output j = i + 1 reads
x'[4 i + t - 1] = x[4 i + t - 2]: the outputs [1, 1 + o1), o1 = (L - 7) // 4 + 1, of the padded input, with
max(0, 4 o1 - L) zero rows behind so that the kernel computes that many.

There are no weights in this library and no way to fetch any: a user supplies them (`from_state_dict`,
`from_lpips_package`).  Parity with the published weights and with the reference's graph is unpinned; the checker is a
float64 evaluation of the definition above with random weights (tests/lpips_ref.py)."""
from __future__ import annotations

import math

import torch

from . import cached, functional

__all__ = ["LPIPS", "LPIPSLoss"]

# (name, support, in, out, stride, pad); a 3 x 3 stride-2 max-pool follows conv1 and conv2
_CONVS = (("conv1", 11, 3, 64, 4, 2), ("conv2", 5, 64, 192, 1, 2), ("conv3", 3, 192, 384, 1, 1),
          ("conv4", 3, 384, 256, 1, 1), ("conv5", 3, 256, 256, 1, 1))
_DEFAULT_SHIFT = (-.030, -.088, -.188)
_DEFAULT_SCALE = (.458, .448, .450)
MIN_SIDE = 31
EPSILON = 1e-10

# names of the PyTorch `lpips` package's state dict (lpips.LPIPS(net="alex")), written from memory: that package is not
# installed where this was written
_PACKAGE_CONVS = ("net.slice1.0", "net.slice2.3", "net.slice3.6", "net.slice4.8", "net.slice5.10")


def _conv1_outputs(length):
    return (length - 7) // 4 + 1


class LPIPS(cached.CachedValues, torch.nn.Module):
    """`LPIPS(weights)(fake, real)` -> float32 [N].  `weights`: this library's own keys — `conv{1..5}_kernel` (HWIO
    float32), `conv{1..5}_bias`, `lin{0..4}` ([C] >= 0), and optionally `shift`, `scale` ([3]).  Everything is a
    buffer: the network is frozen, its convolutions only ever produce the input gradient."""

    _cache_attrs = ("_keys",)

    def __init__(self, weights=None):
        super().__init__()
        if weights is None:
            raise ValueError("LPIPS weights are user-supplied: this library ships none.  Use LPIPS.from_state_dict, "
                             "LPIPS.from_lpips_package, or LPIPS.with_random_weights (tests and timing).")
        weights = dict(weights)
        weights.setdefault("shift", torch.tensor(_DEFAULT_SHIFT))
        weights.setdefault("scale", torch.tensor(_DEFAULT_SCALE))
        expected = {"shift": (3,), "scale": (3,)}
        for i, (name, k, cin, cout, _, _) in enumerate(_CONVS):
            expected[f"{name}_kernel"] = (k, k, cin, cout)
            expected[f"{name}_bias"] = (cout,)
            expected[f"lin{i}"] = (cout,)
        missing, extra = sorted(set(expected) - set(weights)), sorted(set(weights) - set(expected))
        if missing or extra:
            raise ValueError(f"LPIPS weights: missing {missing}, unexpected {extra}")
        for key, shape in expected.items():
            value = torch.as_tensor(weights[key]).detach().to(torch.float32)
            if tuple(value.shape) != shape:
                raise ValueError(f"LPIPS weights: {key} has shape {tuple(value.shape)}, expected {shape}")
            self.register_buffer(key, value.clone().contiguous())

    @classmethod
    def from_state_dict(cls, state_dict):
        """From this library's own keys (what `state_dict()` of an LPIPS returns)."""
        return cls(state_dict)

    @classmethod
    def from_lpips_package(cls, state_dict):
        """From the state dict of the public PyTorch `lpips` package's `LPIPS(net="alex")`: convolutions
        `net.slice1.0`, `net.slice2.3`, `net.slice3.6`, `net.slice4.8`, `net.slice5.10` (`.weight` OIHW -> HWIO,
        `.bias`), `lin{0..4}.model.1.weight` ([1, C, 1, 1] -> [C]), `scaling_layer.shift` / `.scale` ([1, 3, 1, 1] ->
        [3], optional).  These names were written from memory and COULD NOT BE VERIFIED: neither `lpips` nor
        `torchvision` was available.  A missing name raises a KeyError that says which."""
        sd = dict(state_dict)
        out = {}
        for i, ((name, *_), theirs) in enumerate(zip(_CONVS, _PACKAGE_CONVS)):
            out[f"{name}_kernel"] = torch.as_tensor(sd[f"{theirs}.weight"]).permute(2, 3, 1, 0)
            out[f"{name}_bias"] = torch.as_tensor(sd[f"{theirs}.bias"])
            out[f"lin{i}"] = torch.as_tensor(sd[f"lin{i}.model.1.weight"]).reshape(-1)
        for key in ("shift", "scale"):
            if f"scaling_layer.{key}" in sd:
                out[key] = torch.as_tensor(sd[f"scaling_layer.{key}"]).reshape(-1)
        return cls(out)

    @classmethod
    def with_random_weights(cls, seed=0):
        """For tests and timing: He-normal kernels, small biases, `lin` uniform in [0, 1 / C]."""
        gen = torch.Generator().manual_seed(int(seed))
        out = {}
        for i, (name, k, cin, cout, _, _) in enumerate(_CONVS):
            out[f"{name}_kernel"] = torch.randn(k, k, cin, cout, generator=gen) * math.sqrt(2.0 / (k * k * cin))
            out[f"{name}_bias"] = 0.05 * torch.randn(cout, generator=gen)
            out[f"lin{i}"] = torch.rand(cout, generator=gen) / cout
        return cls(out)

    def invalidate_kernel_cache(self):
        """Drops the library's packed fragments of the convolution weights (kept under no_grad)."""
        for key in self.__dict__.pop("_keys", {}).values():
            cached.drop_weights_key(key)

    def _weights_key(self, name):
        if torch.is_grad_enabled() or not cached.KEYED_WEIGHTS:
            return 0
        keys = self.__dict__.setdefault("_keys", {})
        if name not in keys:
            keys[name] = cached.new_weights_key()
        return keys[name]

    def _conv(self, x, name, k, stride, pad):
        kernel, bias = getattr(self, f"{name}_kernel"), getattr(self, f"{name}_bias")
        if not x.is_cuda:
            # the reference composition: the same cross-correlation as tensor ops
            y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), kernel.to(x.dtype).permute(3, 2, 0, 1),
                                           bias.to(x.dtype), stride=stride, padding=pad)
            return torch.relu(y).permute(0, 2, 3, 1)
        key = self._weights_key(name)
        if stride == 1:
            return functional.conv2d_down(x, kernel, bias, 1, "relu", weights_key=key)
        # conv1 (see the top of the file)
        outs = [_conv1_outputs(length) for length in x.shape[1:3]]
        back = [max(0, 4 * o - length) for o, length in zip(outs, x.shape[1:3])]
        x = functional.pad2d(x, (1, back[0]), (1, back[1]))
        y = functional.conv2d_down(x, kernel, bias, stride, "relu", weights_key=key)
        return y[:, 1:1 + outs[0], 1:1 + outs[1]]

    def features(self, images):
        """The five taps of `images` [N, H, W, 3] in [0, 1] (dtype of `images`)."""
        if images.dim() != 4 or images.shape[-1] != 3:
            raise ValueError(f"LPIPS takes [N, H, W, 3] images, received shape {tuple(images.shape)}.")
        if min(images.shape[1:3]) < MIN_SIDE:
            raise ValueError(f"LPIPS needs both sides to be at least {MIN_SIDE} (7 -> 3 -> 1 through conv1 and the "
                             f"pools), got {images.shape[1]} x {images.shape[2]}")
        ft = torch.float64 if images.dtype == torch.float64 else torch.float32
        x = ((2 * images.to(ft) - 1 - self.shift.to(ft)) / self.scale.to(ft)).to(images.dtype)
        taps = []
        for name, k, _, _, stride, pad in _CONVS:
            x = self._conv(x, name, k, stride, pad)
            taps.append(x)
            if name in ("conv1", "conv2"):
                x = functional.max_pool2d(x, 3, 2)
        return taps

    def forward(self, fake, real):
        if fake.shape != real.shape:
            raise ValueError(f"image shapes {tuple(fake.shape)} and {tuple(real.shape)} differ")
        n = fake.shape[0]
        # one batch of 2 N through the trunk
        taps = self.features(torch.cat([fake, real.to(fake.dtype)], 0))
        total = None
        for i, t in enumerate(taps):
            f1 = t[n:] if real.requires_grad else t[n:].detach()     # a gradient nobody needs is not computed
            d = functional.lpips_distance(t[:n], f1, getattr(self, f"lin{i}"), EPSILON)
            total = d if total is None else total + d
        return total


class LPIPSLoss:
    """`HiFiCTrainer(perceptual_loss=LPIPSLoss(lpips))`: NHWC images in [0, 1] -> the batch mean (model.py:872)."""

    def __init__(self, lpips):
        self.lpips = lpips

    def __call__(self, fake, real):
        return self.lpips(fake, real).mean()

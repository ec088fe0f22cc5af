"""Keras `Conv2D` / `Conv2DTranspose` with `padding="same"` as HiFiC uses them (models/hific/archs.py:86-103, 130-161,
201-206), channels last, bias on, no activation, on the two MFMA convolution kernels.

Per spatial axis, input length L, support k, stride s (Keras / TF "SAME"):
  Conv2D:           out = ceil(L / s), total = max((out - 1) s + k - L, 0), before = total // 2,
                    y[i] = sum_t x[i s + t - before] w[t]                        (cross-correlation, zeros outside)
  Conv2DTranspose:  out = L s, before as for the Conv2D that maps L s to L (= max(k - s, 0) // 2),
                    y[m] = f[m + before],  f[m] = sum_i x[i] w[m - i s]           (the full convolution)
The kernels compute (include/tfc_hip.h, tfc_conv2d_down / tfc_conv2d_up)
  down_s(x)[i] = sum_t x[i s + t - k // 2] w[t]    and    up_s(x)[n] = f[n + k // 2],
which is the same window for s = 1 and for odd L at k = 3, s = 2, and one sample later where `before` < k // 2 (k = 3,
s = 2, even L: before = 0).  `a` zero rows / columns in front of the input move the window back, and the first output
samples are dropped (as SignalConv._forward_general does):
  down:  a = m s - (k // 2 - before), m = ceil((k // 2 - before) / s):  y[i] = down_s(x')[i + m]
  up:    a = ceil((k // 2 - before) / s), o = a s - (k // 2 - before):  y[m] = up_s(x')[m + o]

Channel counts the kernels do not take are padded with zeros in the weights.  The forward kernels want 1 ... 4 or a
multiple of 16 INPUT channels and take any number of output channels, so under no_grad (compress / decompress) only
the input side is padded, to the next multiple of 16 (60 -> 64, 220 -> 224; 120, 240, 480, 960 go as they are), and the
output has exactly `filters` channels: no channel slice behind the layer.  The one activation that is padded is the
input of a layer whose own channel count is 60 or 220.  With gradients enabled the weight-gradient kernel wants 1 ... 4
or a multiple of 32 on BOTH sides: there both are padded to 32 and the padded output channels are sliced off.  Under
no_grad the padded weights are made once per weight value and the kernels keep their packed fragments of it
(`weights_key`, as SignalConv2D).  Where the window is moved (stride 2) the output is a cropped view: the next layer
that wants a contiguous tensor (ChannelNorm) copies it."""
from __future__ import annotations

import math

import torch

from . import cached, functional
from .functional import _ntuple

__all__ = ["KerasConv2D", "KerasConv2DTranspose", "same_before"]


def same_before(length, k, s):
    """(out, before) of a Keras / TF `padding="same"` convolution along one axis."""
    out = -(-length // s)
    return out, max((out - 1) * s + k - length, 0) // 2


def _padded_channels(c, multiple):
    return c if c <= 4 else -(-c // multiple) * multiple


class _KerasConvBase(cached.CachedValues, torch.nn.Module):
    transpose = False
    _cache_attrs = ("_padded_cache",)

    def __init__(self, filters, kernel_size, strides=1, in_channels=None):
        super().__init__()
        self.filters = int(filters)
        self.kernel_size = _ntuple(kernel_size, 2)
        if isinstance(strides, (tuple, list)):
            if len(set(strides)) != 1:
                raise NotImplementedError("one stride for both axes")
            strides = strides[0]
        self.strides = int(strides)
        self.kernel = self.bias = None
        if in_channels is not None:
            self.build(int(in_channels))

    def build(self, cin, device=None):
        if self.kernel is not None:
            return
        kh, kw = self.kernel_size
        # Keras' layouts: Conv2D [kh, kw, in, out], Conv2DTranspose [kh, kw, out, in]; glorot_uniform, zero bias
        shape = (kh, kw, self.filters, cin) if self.transpose else (kh, kw, cin, self.filters)
        fan_in, fan_out = kh * kw * shape[2], kh * kw * shape[3]
        limit = math.sqrt(6.0 / (fan_in + fan_out))
        self.kernel = torch.nn.Parameter(torch.empty(shape, device=device).uniform_(-limit, limit))
        self.bias = torch.nn.Parameter(torch.zeros(self.filters, device=device))

    def _hwio(self, kernel):
        return kernel.permute(0, 1, 3, 2) if self.transpose else kernel

    def _padded(self, cin_act):
        """(kernel HWIO with padded channel counts, padded bias, weights key) of the current weights."""
        if torch.is_grad_enabled():
            cin_p, cout_p = _padded_channels(cin_act, 32), _padded_channels(self.filters, 32)
        else:
            cin_p, cout_p = _padded_channels(cin_act, 16), self.filters

        def make():
            k = self._hwio(self.kernel)
            k = torch.nn.functional.pad(k, (0, cout_p - k.shape[3], 0, cin_p - k.shape[2]))
            return k, torch.nn.functional.pad(self.bias, (0, cout_p - self.filters))
        if torch.is_grad_enabled() or not self.kernel.is_cuda:
            return make() + (0,)
        versions = (cached.version_of(self.kernel), cached.version_of(self.bias))
        if None in versions:
            return make() + (0,)
        ident = (self.kernel.data_ptr(), self.bias.data_ptr(), versions, str(self.kernel.device), cin_p)
        hit = self.__dict__.get("_padded_cache")
        if hit is None or hit[0] != ident:
            self.invalidate_kernel_cache()
            k, b = make()
            k, b = k.contiguous(), b.contiguous()
            torch.cuda.current_stream().synchronize()          # complete before another stream reads them
            hit = (ident, k, b, cached.new_weights_key() if cached.KEYED_WEIGHTS else 0)
            self.__dict__["_padded_cache"] = hit
        return hit[1], hit[2], hit[3]

    def invalidate_kernel_cache(self):
        """Drops the padded weights and the library's packed fragments of them: after a write through `.data`, which
        advances neither address nor version counter (load_state_dict, .to(), train() / eval() do it themselves)."""
        hit = self.__dict__.pop("_padded_cache", None)
        if hit is not None and hit[3]:
            cached.drop_weights_key(hit[3])

    def output_size(self, h, w):
        s = self.strides
        return (h * s, w * s) if self.transpose else (-(-h // s), -(-w // s))

    def forward(self, x):
        if x.dim() != 4:
            raise ValueError(f"Input tensor must have rank 4, received shape {tuple(x.shape)}.")
        self.build(x.shape[-1], x.device)
        cin = self.kernel.shape[3] if self.transpose else self.kernel.shape[2]
        if x.shape[-1] != cin:
            raise ValueError(f"kernel expects {cin} input channels, input has {x.shape[-1]}")
        kernel, bias, key = self._padded(cin)
        if kernel.shape[2] != cin:
            x = torch.nn.functional.pad(x, (0, kernel.shape[2] - cin))
        y = self._run(x, kernel, bias, key)
        return y if y.shape[-1] == self.filters else y[..., :self.filters]


class KerasConv2D(_KerasConvBase):
    """tf.keras.layers.Conv2D(filters, kernel_size, strides, padding="same") — kernel [kh, kw, in, out], bias [out]."""

    def _run(self, x, kernel, bias, key, conv=None):
        """`conv`: the launcher behind the window arithmetic (SpectralNormConv2D puts its own there)."""
        conv = conv or functional.conv2d_down
        s = self.strides
        front, skip, back, outs = [], [], [], []
        for d in range(2):
            k, length = self.kernel_size[d], x.shape[1 + d]
            out, before = same_before(length, k, s)
            delta = k // 2 - before
            m = -(-delta // s)
            a = m * s - delta
            front.append(a)
            skip.append(m)
            outs.append(out)
            back.append(max(0, (m + out - 1) * s + 1 - (length + a)))
        if any(front) or any(back):
            x = functional.pad2d(x, (front[0], back[0]), (front[1], back[1]))
        y = conv(x, kernel, bias, s, None, weights_key=key)
        if any(skip) or y.shape[1] != outs[0] or y.shape[2] != outs[1]:
            y = y[:, skip[0]:skip[0] + outs[0], skip[1]:skip[1] + outs[1]]
        return y


class KerasConv2DTranspose(_KerasConvBase):
    """tf.keras.layers.Conv2DTranspose(filters, kernel_size, strides, padding="same") — kernel [kh, kw, out, in]."""
    transpose = True

    def _run(self, x, kernel, bias, key):
        s = self.strides
        front, skip, outs = [], [], []
        for d in range(2):
            k, length = self.kernel_size[d], x.shape[1 + d]
            before = max(k - s, 0) // 2
            delta = k // 2 - before
            a = -(-delta // s)
            front.append(a)
            skip.append(a * s - delta)
            outs.append(length * s)
        if any(front):
            x = functional.pad2d(x, (front[0], 0), (front[1], 0))
        y = functional.conv2d_up(x, kernel, bias, s, None, weights_key=key)
        if any(front):
            y = y[:, skip[0]:skip[0] + outs[0], skip[1]:skip[1] + outs[1]]
        return y

"""IntegerConv2D: the layer of an integer network (Ballé, Johnston and Minnen, ICLR 2019, sections 2-3) by this
project's own definition (ops/integer_ops.py states the integer layer).

Three float parameters, `kernel` H' [kh, kw, Cin, Cout], `bias` b' [Cout], `divisor` c' [Cout]; per output channel o

    H_o = Q(127 H'_o / max(max|H'_o|, 1e-20))             int8
    b_o = clamp(Q(256 b'_o), +-2^29)                      int32
    c_o = clamp(Q(256 r(c'_o)), 1, 2^24)                  int32,   r(c') = max(c', sqrt(1 + eps^2))^2 - eps^2, eps = 2^-18

with Q round-half-even.  A float input runs the training surrogate, y = clip((conv(u, H) + b) / c, 0, out_max) with
the Q'd values as floats: Q is the identity in the backward, the division is float division, and the clip's
derivative is replaced by exp(-alpha^beta |2 v / out_max - 1|^beta), beta = 4, alpha = Gamma(1 / beta) / beta.  An
int8 / uint8 input runs the integer layer from the buffers `freeze()` stored: the coding path never derives the
integers from the floats again (computed in float on two devices they may differ), the same rule as for CDF tables.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ..ops import integer_ops
from . import functional

__all__ = ["IntegerConv2D", "qrelu", "QRELU_ALPHA", "QRELU_BETA"]

QRELU_BETA = 4.0
QRELU_ALPHA = math.gamma(1.0 / QRELU_BETA) / QRELU_BETA
_EPS = 2.0 ** -18
_BUFFERS = ("integer_kernel", "integer_bias", "integer_divisor")


class _QReLU(torch.autograd.Function):
    """clip(v, 0, out_max); its derivative replaced by exp(-alpha^beta |2 v / out_max - 1|^beta)."""

    @staticmethod
    def forward(ctx, v, out_max):
        ctx.save_for_backward(v)
        ctx.out_max = float(out_max)
        return v.clamp(0.0, float(out_max))

    @staticmethod
    def backward(ctx, grad):
        (v,) = ctx.saved_tensors
        slope = torch.exp(-(QRELU_ALPHA ** QRELU_BETA) * torch.abs(2.0 * v / ctx.out_max - 1.0) ** QRELU_BETA)
        return grad * slope, None


def qrelu(v, out_max):
    return _QReLU.apply(v, out_max)


def _round_st(t):
    """Q: round-half-even, the identity in the backward."""
    return t + (torch.round(t) - t).detach()


def _float_conv(u, kernel, stride, up):
    """The float convolution of the surrogate: the project's kernels on the device (float32), the same geometry as
    tensor ops elsewhere (CPU, float64)."""
    if u.is_cuda and u.dtype == torch.float32:
        fn = functional.conv2d_up if up else functional.conv2d_down
        return fn(functional.pad_channels(u), functional.pad_channels(kernel, dim=-2), None, stride)
    kh, kw = kernel.shape[:2]
    x = u.permute(0, 3, 1, 2)
    if not up:
        x = F.pad(x, (kw // 2, (kw - 1) // 2, kh // 2, (kh - 1) // 2))
        y = F.conv2d(x, kernel.permute(3, 2, 0, 1), stride=stride)
    else:
        full = F.pad(F.conv_transpose2d(x, kernel.permute(2, 3, 0, 1), stride=stride), (0, stride, 0, stride))
        y = full[:, :, kh // 2:kh // 2 + u.shape[1] * stride, kw // 2:kw // 2 + u.shape[2] * stride]
    return y.permute(0, 2, 3, 1)


class IntegerConv2D(torch.nn.Module):
    """`same_zeros` padding, explicit padding, `extra_pad_end`.  corr=True with `strides_down` (1 or 2) is the geometry
    of `functional.conv2d_down`; corr=False with `strides_up` is that of `functional.conv2d_up`.  `input_signed`: the
    integer input is int8 (a first layer), else uint8 (the output of another integer layer).  Input channels are
    zero-padded to a multiple of 32 where the integer kernel needs it."""

    def __init__(self, filters, kernel_support, corr=False, strides_down=1, strides_up=1, in_channels=None,
                 out_max=255, input_signed=False):
        super().__init__()
        if in_channels is None:
            raise ValueError("IntegerConv2D needs in_channels")
        support = (kernel_support,) * 2 if isinstance(kernel_support, int) else tuple(int(k) for k in kernel_support)
        limit = integer_ops.IC_CONSTANTS["IC_MAX_SUPPORT"]
        if len(support) != 2 or not all(1 <= k <= limit for k in support):
            raise ValueError(f"kernel_support must be one or two extents of 1 ... {limit}, got {kernel_support!r}")
        strides_down, strides_up = int(strides_down), int(strides_up)
        if corr and strides_up != 1 or not corr and strides_down != 1:
            raise ValueError("IntegerConv2D takes corr=True with strides_down or corr=False with strides_up")
        self.up = not corr
        self.stride = strides_up if self.up else strides_down
        if self.stride not in (1, 2):
            raise ValueError(f"the stride must be 1 or 2, got {self.stride}")
        if not 1 <= int(out_max) <= 255:
            raise ValueError(f"out_max must be 1 ... 255, got {out_max}")
        self.filters, self.kernel_support, self.corr = int(filters), support, bool(corr)
        self.in_channels, self.out_max, self.input_signed = int(in_channels), int(out_max), bool(input_signed)
        if support[0] * support[1] * (self.in_channels + (-self.in_channels % 32)) \
                > integer_ops.IC_CONSTANTS["IC_MAX_REDUCTION"]:
            raise ValueError("kh * kw * in_channels exceeds what an int32 accumulator holds")
        kernel = torch.empty(support + (self.in_channels, self.filters))
        fan_in = support[0] * support[1] * self.in_channels
        bound = math.sqrt(3.0 / fan_in)
        torch.nn.init.uniform_(kernel, -bound, bound)
        self.kernel = torch.nn.Parameter(kernel)
        self.bias = torch.nn.Parameter(torch.zeros(self.filters))
        # r_o = max(127 / (256 max|H'_o|), 1) makes H / c ~ H' at the start; c' = sqrt(r + eps^2) inverts r(c')
        peak = kernel.abs().amax(dim=(0, 1, 2)).clamp_min(1e-20)
        r = (127.0 / (256.0 * peak)).clamp_min(1.0)
        self.divisor = torch.nn.Parameter(torch.sqrt(r + _EPS ** 2))
        for name in _BUFFERS:
            self.register_buffer(name, None)
        self._loaded_integers = False
        self._packed = None

    def extra_repr(self):
        return (f"filters={self.filters}, kernel_support={self.kernel_support}, corr={self.corr}, "
                f"stride={self.stride}, out_max={self.out_max}, input_signed={self.input_signed}")

    # ---- the integers --------------------------------------------------------------------------------------------
    def _quantized(self, dtype):
        """(H, b, c) as floats of `dtype`, integer-valued, differentiable with Q as the identity."""
        kernel, bias, divisor = self.kernel.to(dtype), self.bias.to(dtype), self.divisor.to(dtype)
        peak = kernel.abs().amax(dim=(0, 1, 2)).clamp_min(1e-20)
        h = _round_st(127.0 * kernel / peak)
        b = _round_st(256.0 * bias).clamp(-float(integer_ops.MAX_BIAS), float(integer_ops.MAX_BIAS))
        r = divisor.clamp_min(math.sqrt(1.0 + _EPS ** 2)) ** 2 - _EPS ** 2
        c = _round_st(256.0 * r).clamp(1.0, float(integer_ops.MAX_DIVISOR))
        return h, b, c

    @torch.no_grad()
    def integer_parameters(self):
        """(H int8 [kh, kw, Cin, Cout], b int32 [Cout], c int32 [Cout]) derived from the float parameters, in float32
        on their device."""
        h, b, c = self._quantized(torch.float32)
        return h.to(torch.int8), b.to(torch.int32), c.to(torch.int32)

    @torch.no_grad()
    def freeze(self):
        """Derives the integers once and stores them as buffers of the state_dict; the integer path reads only those."""
        for name, value in zip(_BUFFERS, self.integer_parameters()):
            self.register_buffer(name, value.contiguous())
        self._loaded_integers = False
        self._packed = None
        return self

    @property
    def frozen(self):
        return self.integer_kernel is not None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # a frozen layer's state loads into a layer that has not been frozen: the buffers take the stored values
        present = [prefix + name in state_dict for name in _BUFFERS]
        if all(present):
            for name in _BUFFERS:
                stored = state_dict[prefix + name]
                own = getattr(self, name)
                if own is None or own.shape != stored.shape:
                    self.register_buffer(name, torch.zeros_like(stored, device=self.kernel.device))
            self._loaded_integers = True
        self._packed = None
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _packed_kernel(self, device):
        """(kernel with Cin padded to a multiple of 32, its [kh, kw, Cout, Cin] copy, bias, divisor) on `device`, made
        once per value of the buffers."""
        key = (self.integer_kernel.data_ptr(), self.integer_kernel._version, self.integer_bias._version,
               self.integer_divisor._version, str(device))
        if self._packed is None or self._packed[0] != key:
            kernel = functional.pad_channels(self.integer_kernel.to(device), 32, dim=-2).contiguous()
            self._packed = (key, kernel, integer_ops.pack_integer_kernel(kernel),
                            self.integer_bias.to(device).contiguous(), self.integer_divisor.to(device).contiguous())
        return self._packed[1:]

    # ---- the two paths -------------------------------------------------------------------------------------------
    def forward(self, x):
        if x.dim() != 4 or x.shape[-1] != self.in_channels:
            raise ValueError(f"input must be [N, H, W, {self.in_channels}], received shape {tuple(x.shape)}")
        if x.dtype in (torch.int8, torch.uint8):
            return self._integer(x)
        if not x.is_floating_point():
            raise TypeError(f"IntegerConv2D takes float (training) or int8 / uint8 (coding) inputs, got {x.dtype}")
        return self._surrogate(x)

    def _integer(self, x):
        want = torch.int8 if self.input_signed else torch.uint8
        if x.dtype != want:
            raise TypeError(f"this layer's integer input is {want}, got {x.dtype}")
        if not self.frozen:
            raise RuntimeError("the integer path needs freeze() (or a loaded state_dict of a frozen layer) first")
        kernel, packed, bias, divisor = self._packed_kernel(x.device)
        x = functional.pad_channels(x, 32)
        return integer_ops.integer_conv2d(x, kernel, bias, divisor, self.stride, self.up, self.out_max,
                                          packed_kernel=packed if x.is_cuda else None)

    def _surrogate(self, u):
        dtype = torch.float64 if u.dtype == torch.float64 else torch.float32
        if torch.is_grad_enabled():
            self._loaded_integers = False       # the floats are being trained: loaded integers no longer stand for them
        h, b, c = self._quantized(dtype)
        v = (_float_conv(u.to(dtype), h, self.stride, self.up) + b) / c
        return qrelu(v, self.out_max).to(u.dtype)

"""The integer convolution layer of an integer network (Ballé, Johnston and Minnen, "Integer Networks for Data
Compression with Latent-Variable Models", ICLR 2019, sections 2-3), by this project's own definition
(include/tfc_hip.h, tfc_integer_conv2d); parity with anyone's checkpoints is not pinned.

    x [N, H, W, Cin] int8 (-128 ... 127) or uint8 (0 ... 255), kernel [kh, kw, Cin, Cout] int8 (HWIO),
    bias [Cout] int32 (|b| <= 2^29), divisor [Cout] int32 (1 <= c <= 2^24), out_max 1 ... 255

    v[n,p,o] = bias[o] + sum over taps t and i < Cin of W[t,i,o] x[n, src(p,t), i]      (exact, in int32)
    y[n,p,o] = min(max(floor((v + floor(c[o] / 2)) / c[o]), 0), out_max)                (uint8)

with the geometry of `functional.conv2d_down` (up = False) or `functional.conv2d_up` (up = True), zeros outside the
image, stride 1 or 2, any support from 1 to 9 per axis.  Cin is a multiple of 32 and kh kw Cin at most 32768, so no sum
leaves int32 and every order of summation gives the same integers: the same bytes on every device and build.

`integer_conv2d` runs csrc/integer_conv.hip (the i8 MFMA, int32 accumulators, the division and the clamp in the same
kernel).  `integer_conv2d_reference` is the same definition as float64 convolutions on the CPU, exact below 2^53;
torch has no integer matrix product on HIP.  CPU tensors take the reference.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import _lib

__all__ = ["integer_conv2d", "integer_conv2d_reference", "pack_integer_kernel", "IC_CONSTANTS"]

# the named constants of csrc/integer_conv_params.h (tile sizes, argument limits)
IC_CONSTANTS = _lib.kernel_constants("integer_conv_params.h", ("IC",))

MAX_BIAS = 1 << IC_CONSTANTS["IC_MAX_BIAS_LOG2"]
MAX_DIVISOR = 1 << IC_CONSTANTS["IC_MAX_DIVISOR_LOG2"]


def _check_args(x, kernel, bias, divisor, stride, up, out_max):
    if x.dtype not in (torch.int8, torch.uint8):
        raise TypeError(f"integer_conv2d takes int8 or uint8 activations, got {x.dtype}")
    if kernel.dtype != torch.int8:
        raise TypeError(f"the kernel must be int8, got {kernel.dtype}")
    if bias.dtype != torch.int32 or divisor.dtype != torch.int32:
        raise TypeError(f"bias and divisor must be int32, got {bias.dtype} and {divisor.dtype}")
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError(f"x must be [N, H, W, Cin] with every extent at least 1, received shape {tuple(x.shape)}")
    if kernel.dim() != 4 or kernel.shape[3] < 1:
        raise ValueError(f"the kernel must be [kh, kw, Cin, Cout], received shape {tuple(kernel.shape)}")
    kh, kw, cin, cout = kernel.shape
    limit = IC_CONSTANTS["IC_MAX_SUPPORT"]
    if not (1 <= kh <= limit and 1 <= kw <= limit):
        raise ValueError(f"the kernel support must be 1 ... {limit} per axis, got {kh} x {kw}")
    if cin != x.shape[3]:
        raise ValueError(f"kernel expects {cin} input channels, input has {x.shape[3]}")
    if cin % IC_CONSTANTS["IC_CIN_MULTIPLE"]:
        raise ValueError(f"Cin must be a multiple of {IC_CONSTANTS['IC_CIN_MULTIPLE']}, got {cin}")
    if kh * kw * cin > IC_CONSTANTS["IC_MAX_REDUCTION"]:
        raise ValueError(f"kh * kw * Cin must be at most {IC_CONSTANTS['IC_MAX_REDUCTION']}, got {kh * kw * cin}")
    if tuple(bias.shape) != (cout,) or tuple(divisor.shape) != (cout,):
        raise ValueError(f"bias and divisor must be [{cout}], received {tuple(bias.shape)} and {tuple(divisor.shape)}")
    if stride not in (1, 2):
        raise ValueError(f"stride must be 1 or 2, got {stride}")
    if not 1 <= int(out_max) <= 255:
        raise ValueError(f"out_max must be 1 ... 255, got {out_max}")
    return bool(up)


def integer_conv2d_reference(x, kernel, bias, divisor, stride=1, up=False, out_max=255):
    """The definition in exact arithmetic: float64 convolutions on the CPU (every partial sum is an integer below
    2^31, far inside float64's 2^53), then int64 for the bias, the rounding division and the clamps.  The result
    returns to x's device.  Checks the ranges of bias and divisor, which the kernel takes on trust."""
    up = _check_args(x, kernel, bias, divisor, stride, up, out_max)
    b64, c64 = bias.cpu().to(torch.int64), divisor.cpu().to(torch.int64)
    if int(b64.abs().max()) > MAX_BIAS:
        raise ValueError(f"|bias| must be at most 2^{IC_CONSTANTS['IC_MAX_BIAS_LOG2']}")
    if int(c64.min()) < 1 or int(c64.max()) > MAX_DIVISOR:
        raise ValueError(f"divisor must be 1 ... 2^{IC_CONSTANTS['IC_MAX_DIVISOR_LOG2']}")
    kh, kw = kernel.shape[:2]
    s = int(stride)
    xd = x.cpu().to(torch.float64).permute(0, 3, 1, 2)
    wd = kernel.cpu().to(torch.float64)
    if not up:
        xd = F.pad(xd, (kw // 2, (kw - 1) // 2, kh // 2, (kh - 1) // 2))
        v = F.conv2d(xd, wd.permute(3, 2, 0, 1), stride=s)
    else:
        # y[q s + phi] = sum_i x[i] w[phi + (q - i) s + k / 2]: the full transposed convolution from k / 2 on
        full = F.conv_transpose2d(xd, wd.permute(2, 3, 0, 1), stride=s)
        full = F.pad(full, (0, s, 0, s))
        v = full[:, :, kh // 2:kh // 2 + x.shape[1] * s, kw // 2:kw // 2 + x.shape[2] * s]
    v = v.permute(0, 2, 3, 1).round().to(torch.int64) + b64
    y = torch.div(v + torch.div(c64, 2, rounding_mode="floor"), c64, rounding_mode="floor")
    return y.clamp(0, int(out_max)).to(torch.uint8).contiguous().to(x.device)


def pack_integer_kernel(kernel):
    """The layout tfc_integer_conv2d reads: int8 [kh, kw, Cout, Cin], the cin bytes of one (tap, output channel)
    contiguous."""
    return kernel.permute(0, 1, 3, 2).contiguous()


def integer_conv2d(x, kernel, bias, divisor, stride=1, up=False, out_max=255, packed_kernel=None):
    """x [N, H, W, Cin] int8 / uint8, kernel [kh, kw, Cin, Cout] int8 (HWIO), bias / divisor [Cout] int32 -> uint8
    [N, H', W', Cout] on the integer MFMA kernel.  `packed_kernel`: `pack_integer_kernel(kernel)` made once by a caller
    whose weights do not change (a frozen layer).  bias and divisor are taken inside their ranges (|b| <= 2^29,
    1 <= c <= 2^24); the reference checks them.  CPU tensors take `integer_conv2d_reference`."""
    if not x.is_cuda:
        return integer_conv2d_reference(x, kernel, bias, divisor, stride, up, out_max)
    up = _check_args(x, kernel, bias, divisor, stride, up, out_max)
    if any(t.device != x.device for t in (kernel, bias, divisor)):
        raise ValueError("x, kernel, bias and divisor must be on the same device")
    if packed_kernel is None:
        packed_kernel = pack_integer_kernel(kernel)
    elif packed_kernel.dtype != torch.int8 or tuple(packed_kernel.shape) != tuple(kernel.permute(0, 1, 3, 2).shape) \
            or packed_kernel.device != x.device or not packed_kernel.is_contiguous():
        raise ValueError("packed_kernel must be pack_integer_kernel(kernel) on x's device")
    x, bias, divisor = x.contiguous(), bias.contiguous(), divisor.contiguous()
    n, h, w, cin = x.shape
    kh, kw, _, cout = kernel.shape
    s = int(stride)
    oh, ow = (h * s, w * s) if up else (-(-h // s), -(-w // s))
    y = torch.empty((n, oh, ow, cout), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().tfc_integer_conv2d(
        x.data_ptr(), int(x.dtype == torch.uint8), packed_kernel.data_ptr(), bias.data_ptr(), divisor.data_ptr(),
        y.data_ptr(), n, h, w, cin, cout, kh, kw, s, int(up), int(out_max), _lib.stream_ptr()))
    return y

"""SSIM and multiscale SSIM (`tf.image.ssim`, `tf.image.ssim_multiscale`) on the fused scale-pass kernels.

The functions are TensorFlow's, not the reference tree's: its models only call `tf.image.ssim_multiscale`
(models/bls2017.py:295, bmshj2018.py:371, ms2020.py:542).  The definition used here is restated in DESIGN.md; parity
is unpinned against TensorFlow itself.

`ssim` / `ssim_multiscale` run one launch of csrc/ssim.hip per scale, forward and backward, on device tensors of dtype
uint8, float32, bfloat16 or float16.  `ssim_reference` / `ssim_multiscale_reference` are the same functions composed op
by op from torch's conv2d, pad and avg_pool2d, on any device, in float32 or float64: the yardstick of the accuracy
tests and of the timing, used by no model path.  `scale_reference` is that composition for one scale pass, in the layout
of `scale_forward`; `SSIM_CONSTANTS` are the kernels' tile sides and tap limits, read from csrc/ssim_params.h."""
from __future__ import annotations

import ctypes as C
import functools
import math
import numbers

import torch

from .. import _lib
from .._lib import ptr as _ptr

__all__ = ["ssim", "ssim_multiscale", "ssim_reference", "ssim_multiscale_reference", "scale_reference",
           "MSSSIM_POWER_FACTORS", "SSIM_CONSTANTS"]

MSSSIM_POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
SSIM_CONSTANTS = _lib.kernel_constants("ssim_params.h", ("SSIM",))
MAX_FILTER_SIZE = SSIM_CONSTANTS["SSIM_MAX_TAPS"]       # csrc/ssim.hip: the taps travel in the kernel arguments

_DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2, torch.uint8: 3}


def _window(filter_size, filter_sigma):
    """The normalised 1-D Gaussian taps, as Python floats (float64)."""
    n = int(filter_size)
    sigma = float(filter_sigma)
    if not sigma > 0.0:
        raise ValueError(f"filter_sigma must be positive, got {filter_sigma}")
    g = [math.exp(-((i - (n - 1) / 2.0) ** 2) / (2.0 * sigma * sigma)) for i in range(n)]
    total = math.fsum(g)
    return [v / total for v in g]


def min_side(num_scales, filter_size):
    """The smallest H or W for which every one of `num_scales` scales still holds one window (161 for 5 x 11)."""
    return (int(filter_size) - 1) * 2 ** (num_scales - 1) + 1


def _check(img1, img2, filter_size, num_scales, max_filter):
    if isinstance(filter_size, bool) or not isinstance(filter_size, numbers.Integral):
        raise ValueError(f"filter_size must be an integer, got {filter_size!r}")
    if filter_size < 1 or filter_size > max_filter:
        raise ValueError(f"filter_size must be between 1 and {max_filter}, got {filter_size}")
    if img1.shape != img2.shape:
        raise ValueError(f"img1 and img2 must have the same shape, got {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img1.dim() < 3:
        raise ValueError(f"images must be [..., H, W, C], got shape {tuple(img1.shape)}")
    h, w = img1.shape[-3], img1.shape[-2]
    need = min_side(num_scales, filter_size)
    if h < need or w < need:
        raise ValueError(
            f"image of {h} x {w} is too small: with filter_size {filter_size} and {num_scales} scale(s) the smallest "
            f"accepted side is {need}")
    if img1.shape[-1] < 1 or img1.numel() == 0:
        raise ValueError(f"images must not be empty, got shape {tuple(img1.shape)}")


def _constants(max_val, k1, k2):
    max_val = float(max_val)
    return (float(k1) * max_val) ** 2, (float(k2) * max_val) ** 2


# ---------------------------------------------------------------------------------------------------------------------
# op-by-op reference
# ---------------------------------------------------------------------------------------------------------------------

def _planes_nchw(img, ft):
    lead = img.shape[:-3]
    h, w, c = img.shape[-3:]
    return img.reshape(-1, h, w, c).to(ft).permute(0, 3, 1, 2), lead


def _scale_reference(x, y, kernel, c1, c2):
    """x, y [B, C, H, W] -> (ssim_plane, cs_plane), each [B, C]."""
    c = x.shape[1]
    f = lambda t: torch.nn.functional.conv2d(t, kernel, groups=c)      # noqa: E731
    mu1, mu2 = f(x), f(y)
    s, p = f(x * x + y * y), f(x * y)
    lum = (2.0 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)
    cs = (2.0 * p - 2.0 * mu1 * mu2 + c2) / (s - mu1 * mu1 - mu2 * mu2 + c2)
    return (lum * cs).mean(dim=(-2, -1)), cs.mean(dim=(-2, -1))


def _reference_kernel(filter_size, filter_sigma, channels, ft, device):
    g = torch.tensor(_window(filter_size, filter_sigma), dtype=torch.float64)
    return torch.outer(g, g).to(ft)[None, None].repeat(channels, 1, 1, 1).to(device)


def _downsample_reference(t):
    h, w = t.shape[-2:]
    if h % 2 or w % 2:
        t = torch.nn.functional.pad(t, (0, w % 2, 0, h % 2), mode="replicate")
    return torch.nn.functional.avg_pool2d(t, 2)


def scale_reference(x, y, taps, c1, c2, pool):
    """The tensor-op twin of `scale_forward`: x, y [B, H, W, C] -> (means [B * C, 2], pooled_x, pooled_y) in its layout
    (the pooled pair [B * C, ceil(H / 2), ceil(W / 2), 1], or None without `pool`).  Any device; float64 inputs stay
    float64, anything else is computed in float32.  Differentiable in both images."""
    ft = torch.float64 if x.dtype == torch.float64 else torch.float32
    b, h, w, c = x.shape
    px, _ = _planes_nchw(x, ft)
    py, _ = _planes_nchw(y, ft)
    g = torch.tensor([float(v) for v in taps], dtype=torch.float64)
    kernel = torch.outer(g, g).to(ft)[None, None].repeat(c, 1, 1, 1).to(x.device)
    value, cs = _scale_reference(px, py, kernel, c1, c2)
    means = torch.stack((value, cs), dim=-1).reshape(b * c, 2)
    if not pool:
        return means, None, None
    halved = lambda t: _downsample_reference(t).reshape(b * c, (h + 1) // 2, (w + 1) // 2, 1)      # noqa: E731
    return means, halved(px), halved(py)


def ssim_reference(img1, img2, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """`ssim` composed from torch ops (float64 inputs stay float64, anything else is computed in float32)."""
    _check(img1, img2, filter_size, 1, 1 << 20)
    ft = torch.float64 if img1.dtype == torch.float64 else torch.float32
    x, lead = _planes_nchw(img1, ft)
    y, _ = _planes_nchw(img2, ft)
    c1, c2 = _constants(max_val, k1, k2)
    kernel = _reference_kernel(filter_size, filter_sigma, x.shape[1], ft, x.device)
    value, _ = _scale_reference(x, y, kernel, c1, c2)
    return value.mean(dim=-1).reshape(lead)


def ssim_multiscale_reference(img1, img2, max_val, power_factors=MSSSIM_POWER_FACTORS, filter_size=11,
                              filter_sigma=1.5, k1=0.01, k2=0.03):
    """`ssim_multiscale` composed from conv2d (groups = C), pad(mode="replicate") and avg_pool2d."""
    power_factors = tuple(float(v) for v in power_factors)
    _check(img1, img2, filter_size, len(power_factors), 1 << 20)
    ft = torch.float64 if img1.dtype == torch.float64 else torch.float32
    x, lead = _planes_nchw(img1, ft)
    y, _ = _planes_nchw(img2, ft)
    c1, c2 = _constants(max_val, k1, k2)
    kernel = _reference_kernel(filter_size, filter_sigma, x.shape[1], ft, x.device)
    values = []
    for j in range(len(power_factors)):
        if j:
            x, y = _downsample_reference(x), _downsample_reference(y)
        value, cs = _scale_reference(x, y, kernel, c1, c2)
        values.append(torch.relu(value if j == len(power_factors) - 1 else cs))
    stacked = torch.stack(values, dim=-1)                                   # [B, C, scales]
    weights = torch.tensor(power_factors, dtype=ft, device=stacked.device)
    return torch.prod(stacked ** weights, dim=-1).mean(dim=-1).reshape(lead)


# ---------------------------------------------------------------------------------------------------------------------
# fused scale pass
# ---------------------------------------------------------------------------------------------------------------------

def _taps_arg(taps):
    return (C.c_float * len(taps))(*taps)


def scale_forward(x, y, taps, c1, c2, pool):
    """tfc_ssim_scale_forward: x, y [B, H, W, C] contiguous -> (means [B * C, 2], pooled_x, pooled_y); the pooled pair
    is float32 [B * C, ceil(H / 2), ceil(W / 2), 1], or None without `pool`."""
    b, h, w, c = x.shape
    means = torch.empty((b * c, 2), dtype=torch.float32, device=x.device)
    px = py = None
    if pool:
        px = torch.empty((b * c, (h + 1) // 2, (w + 1) // 2, 1), dtype=torch.float32, device=x.device)
        py = torch.empty_like(px)
    _lib.check(_lib.lib().tfc_ssim_scale_forward(
        x.data_ptr(), y.data_ptr(), _DTYPE_CODE[x.dtype], b, h, w, c, _taps_arg(taps), len(taps), c1, c2,
        means.data_ptr(), _ptr(px), _ptr(py), _lib.stream_ptr()))
    return means, px, py


def scale_backward(x, y, taps, c1, c2, grad_means, grad_px, grad_py, need_x, need_y):
    """tfc_ssim_scale_backward -> (grad_x, grad_y), float32 in the shape of x (None where not needed)."""
    b, h, w, c = x.shape
    gx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_x else None
    gy = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_y else None
    _lib.check(_lib.lib().tfc_ssim_scale_backward(
        x.data_ptr(), y.data_ptr(), _DTYPE_CODE[x.dtype], b, h, w, c, _taps_arg(taps), len(taps), c1, c2,
        grad_means.data_ptr(), _ptr(grad_px), _ptr(grad_py), _ptr(gx), _ptr(gy), _lib.stream_ptr()))
    return gx, gy


class _ScalePass(torch.autograd.Function):
    """One scale: (x, y) -> (means, pooled_x, pooled_y).  Saves the two images only; backward recomputes the moments
    and takes the gradient of the pooled pair (the coarser scale's) in the same launch."""

    @staticmethod
    def forward(ctx, x, y, taps, c1, c2, pool):
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, y)
        ctx.cfg = (taps, c1, c2)
        means, px, py = scale_forward(x, y, taps, c1, c2, pool)
        if not pool:
            return means, None, None
        # an image that needs no gradient needs none through its halved copies either
        ctx.mark_non_differentiable(*[t for t, need in zip((px, py), ctx.needs_input_grad[:2]) if not need])
        return means, px, py

    @staticmethod
    def backward(ctx, grad_means, grad_px, grad_py):
        x, y = ctx.saved_tensors
        taps, c1, c2 = ctx.cfg
        need_x, need_y = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if grad_means is None:
            grad_means = torch.zeros((x.shape[0] * x.shape[3], 2), dtype=torch.float32, device=x.device)
        cont = lambda t: None if t is None else t.contiguous().float()      # noqa: E731
        gx, gy = scale_backward(x, y, taps, c1, c2, grad_means.contiguous().float(), cont(grad_px) if need_x else None,
                                cont(grad_py) if need_y else None, need_x, need_y)
        if gx is not None:
            gx = gx.to(x.dtype)
        if gy is not None:
            gy = gy.to(y.dtype)
        return gx, gy, None, None, None, None


def _prepare(img1, img2):
    """-> x, y [B, H, W, C] contiguous on the device in one kernel dtype, and the leading shape."""
    _lib.require_device()
    if not (img1.is_cuda and img2.is_cuda):
        raise ValueError("ssim / ssim_multiscale run on device tensors; ssim_reference / ssim_multiscale_reference "
                         "evaluate the same functions with torch ops on any device")
    if img1.dtype != img2.dtype or img1.dtype not in _DTYPE_CODE:
        # mixed or unsupported dtypes: both in float32 (a cast by torch; the kernels read one dtype)
        img1, img2 = img1.float(), img2.float()
    lead = img1.shape[:-3]
    h, w, c = img1.shape[-3:]
    return img1.reshape(-1, h, w, c).contiguous(), img2.reshape(-1, h, w, c).contiguous(), lead


@functools.lru_cache(maxsize=16)
def _weights(power_factors, device):
    """The exponents on the device, uploaded once (a host-to-device copy per call would hold the host up every step)."""
    return torch.tensor(power_factors, dtype=torch.float32, device=device)


def _scale_pass(x, y, taps, c1, c2, pool):
    floating = x.dtype.is_floating_point
    if torch.is_grad_enabled() and floating and (x.requires_grad or y.requires_grad):
        return _ScalePass.apply(x, y, taps, c1, c2, pool)
    return scale_forward(x, y, taps, c1, c2, pool)


def ssim(img1, img2, max_val, filter_size=11, filter_sigma=1.5, k1=0.01, k2=0.03):
    """`tf.image.ssim`: img1, img2 [..., H, W, C] (uint8, float32, bfloat16 or float16) -> float32 [...], the mean over
    the channels of the mean SSIM map of each.  One fused launch; differentiable in either floating-point image."""
    _check(img1, img2, filter_size, 1, MAX_FILTER_SIZE)
    taps = tuple(_window(int(filter_size), filter_sigma))
    c1, c2 = _constants(max_val, k1, k2)
    x, y, lead = _prepare(img1, img2)
    means, _, _ = _scale_pass(x, y, taps, c1, c2, False)
    return means[:, 0].reshape(x.shape[0], x.shape[3]).mean(dim=-1).reshape(lead)


def ssim_multiscale(img1, img2, max_val, power_factors=MSSSIM_POWER_FACTORS, filter_size=11, filter_sigma=1.5,
                    k1=0.01, k2=0.03):
    """`tf.image.ssim_multiscale`: img1, img2 [..., H, W, C] -> float32 [...].  One fused launch per scale (the pass
    also writes the halved pair of the next one); the relu, the powers, their product and the channel mean are torch
    ops on the [planes, scales] tensor.  Every scale must hold one window: H, W >= (filter_size - 1) * 2^(scales - 1) + 1
    (161 for the defaults), else ValueError.  Differentiable in either floating-point image."""
    power_factors = tuple(float(v) for v in power_factors)
    if not power_factors:
        raise ValueError("power_factors must not be empty")
    _check(img1, img2, filter_size, len(power_factors), MAX_FILTER_SIZE)
    taps = tuple(_window(int(filter_size), filter_sigma))
    c1, c2 = _constants(max_val, k1, k2)
    x, y, lead = _prepare(img1, img2)
    b, c = x.shape[0], x.shape[3]
    last = len(power_factors) - 1
    values = []
    for j in range(last + 1):
        means, px, py = _scale_pass(x, y, taps, c1, c2, j != last)
        values.append(means[:, 0] if j == last else means[:, 1])
        x, y = px, py
    stacked = torch.relu(torch.stack(values, dim=-1))                       # [planes, scales]
    return torch.prod(stacked ** _weights(power_factors, stacked.device), dim=-1).reshape(b, c).mean(dim=-1).reshape(lead)

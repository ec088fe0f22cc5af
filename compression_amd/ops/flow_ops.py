"""The scale-space warp of "Scale-space flow for end-to-end optimized video compression" (Agustsson, Minnen, Johnston,
Ballé, Hwang, Toderici, CVPR 2020, section 3.1).  The definition is this project's own, include/tfc_hip.h states it in
full and tests/flow_ref.py is its float64 form:

    gaussian_scale_space   x [N, H, W, C] -> V [N, M + 1, H, W, C]: plane 0 is x, plane p is x blurred separably (rows,
                           then columns) with sigma_p = sigma0 2^(p - 1), taps exp(-t^2 / 2 sigma_p^2) for |t| <=
                           ceil(3 sigma_p); taps outside the image are dropped and the rest renormalised
    scale_space_warp       V, flow [N, H, W, 3] = (dx, dy, s) -> [N, H, W, C]: trilinear sampling at
                           (j + dx, i + dy, s), every coordinate clamped into the volume (a NaN goes to 0), zero
                           flow gradient where a coordinate was clamped
    scale_space_predict    both in one call; its backward goes from the fixed-point volume gradient straight to the
                           image gradient

Each runs the kernels of csrc/scale_space.hip on device tensors (float32, contiguous, channels last) and is
bit-identical from call to call, the backward included: the scatter into the volume accumulates 64-bit integers.  Each
has a `*_reference` twin of plain tensor ops, which CPU tensors (and float64) take."""
from __future__ import annotations

import math

import torch

from .. import _lib
from .._lib import ptr as _ptr

__all__ = ["gaussian_scale_space", "scale_space_warp", "scale_space_predict", "gaussian_scale_space_reference",
           "scale_space_warp_reference", "scale_space_predict_reference", "scale_space_radii",
           "SCALE_SPACE_CONSTANTS"]


# the named constants of csrc/scale_space_params.h (tile sizes, the argument limits)
SCALE_SPACE_CONSTANTS = _lib.kernel_constants("scale_space_params.h", ("SS",))


def _check_levels(num_levels, sigma0):
    k = SCALE_SPACE_CONSTANTS
    if int(num_levels) != num_levels or not 1 <= num_levels <= k["SS_MAX_LEVELS"]:
        raise ValueError(f"num_levels must be an integer in [1, {k['SS_MAX_LEVELS']}], got {num_levels!r}")
    sigma0 = float(sigma0)
    if not sigma0 > 0.0 or not sigma0 * 2.0 ** (num_levels - 1) <= k["SS_MAX_SIGMA"]:
        raise ValueError(f"sigma0 must be positive and sigma0 * 2^(num_levels - 1) at most {k['SS_MAX_SIGMA']}, got "
                         f"{sigma0} with {num_levels} levels")
    return int(num_levels), sigma0


def scale_space_radii(num_levels=5, sigma0=1.5):
    """[ceil(3 sigma_p) for p = 1 .. num_levels]."""
    num_levels, sigma0 = _check_levels(num_levels, sigma0)
    return [int(math.ceil(3.0 * sigma0 * 2.0 ** p)) for p in range(num_levels)]


def _check_tensor(t, name, rank, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if t.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"{what}: {name} must be float32 (float64 for the reference), got {t.dtype}")
    if t.dim() != rank:
        raise ValueError(f"{what}: {name} must have rank {rank}, received shape {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{what}: {name} must be contiguous")


def _check_image(x, what):
    _check_tensor(x, "x", 4, what)
    k = SCALE_SPACE_CONSTANTS
    n, h, w, c = x.shape
    if not 1 <= c <= k["SS_MAX_C"]:
        raise ValueError(f"{what}: channels must be in [1, {k['SS_MAX_C']}], got {c}")
    if not (1 <= h <= k["SS_MAX_DIM"] and 1 <= w <= k["SS_MAX_DIM"]):
        raise ValueError(f"{what}: H and W must be in [1, {k['SS_MAX_DIM']}], got {h} x {w}")


def _check_flow(flow, nhw, what):
    _check_tensor(flow, "flow", 4, what)
    if flow.shape[-1] != 3:
        raise ValueError(f"{what}: flow must be [N, H, W, 3] = (dx, dy, s), received shape {tuple(flow.shape)}")
    if tuple(flow.shape[:3]) != tuple(nhw):
        raise ValueError(f"{what}: flow of shape {tuple(flow.shape)} does not match N, H, W = {tuple(nhw)}")


def _check_volume_flow(volume, flow, what):
    _check_tensor(volume, "volume", 5, what)
    if volume.shape[1] < 2:
        raise ValueError(f"{what}: the volume must have at least 2 planes, received shape {tuple(volume.shape)}")
    k = SCALE_SPACE_CONSTANTS
    if volume.shape[1] - 1 > k["SS_MAX_LEVELS"]:
        raise ValueError(f"{what}: the volume must have at most {k['SS_MAX_LEVELS'] + 1} planes, received shape "
                         f"{tuple(volume.shape)}")
    n, _, h, w, c = volume.shape
    if not 1 <= c <= k["SS_MAX_C"]:
        raise ValueError(f"{what}: channels must be in [1, {k['SS_MAX_C']}], got {c}")
    if not (1 <= h <= k["SS_MAX_DIM"] and 1 <= w <= k["SS_MAX_DIM"]):
        raise ValueError(f"{what}: H and W must be in [1, {k['SS_MAX_DIM']}], got {h} x {w}")
    _check_flow(flow, (n, h, w), what)
    if flow.dtype != volume.dtype:
        raise TypeError(f"{what}: volume and flow must share a dtype, got {volume.dtype} and {flow.dtype}")
    if flow.device != volume.device:
        raise ValueError(f"{what}: volume and flow must be on the same device")


def _on_kernels(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


# -------------------------------------------------------------------------------------------------------------------
# the twins


def _blur_matrix(n, sigma, dtype, device):
    """[n, n]: row i holds the renormalised taps of output position i."""
    radius = int(math.ceil(3.0 * sigma))
    at = torch.arange(n, device=device)
    d = (at[None, :] - at[:, None]).abs()
    w = torch.exp(-(d.to(dtype) ** 2) / (2.0 * sigma * sigma))
    w = torch.where(d <= radius, w, torch.zeros((), dtype=dtype, device=device))
    return w / w.sum(dim=1, keepdim=True)


def gaussian_scale_space_reference(x, num_levels=5, sigma0=1.5):
    """`gaussian_scale_space` as differentiable tensor ops: per plane two dense [W, W] and [H, H] blur matrices."""
    _check_image(x, "gaussian_scale_space")
    num_levels, sigma0 = _check_levels(num_levels, sigma0)
    _, h, w, _ = x.shape
    planes = [x]
    for p in range(num_levels):
        sigma = sigma0 * 2.0 ** p
        rows = torch.einsum("jk,nikc->nijc", _blur_matrix(w, sigma, x.dtype, x.device), x)
        planes.append(torch.einsum("ik,nkjc->nijc", _blur_matrix(h, sigma, x.dtype, x.device), rows))
    return torch.stack(planes, dim=1)


def _axis(raw, last):
    """-> (cell 0, cell 1, weight of cell 1): the clamped coordinate, differentiable only where it was not clamped."""
    value = raw.detach()
    hi = torch.full_like(value, float(last))
    clamped = torch.fmin(torch.fmax(value, torch.zeros_like(value)), hi)
    inside = (value > 0) & (value < last)
    p = clamped + torch.where(inside, raw - value, torch.zeros_like(value))
    a0 = torch.clamp(torch.floor(clamped).to(torch.int64), 0, max(last - 1, 0))
    a1 = torch.clamp(a0 + 1, max=last)
    return a0, a1, p - a0.to(raw.dtype)


def scale_space_warp_reference(volume, flow):
    """`scale_space_warp` as differentiable tensor ops: eight gathers and their weights."""
    _check_volume_flow(volume, flow, "scale_space_warp")
    n, planes, h, w, _ = volume.shape
    jj = torch.arange(w, device=flow.device, dtype=flow.dtype)[None, None, :]
    ii = torch.arange(h, device=flow.device, dtype=flow.dtype)[None, :, None]
    x0, x1, wx = _axis(jj + flow[..., 0], w - 1)
    y0, y1, wy = _axis(ii + flow[..., 1], h - 1)
    z0, z1, wz = _axis(flow[..., 2], planes - 1)
    nn = torch.arange(n, device=flow.device)[:, None, None].expand(n, h, w)
    out = None
    for z, az in ((z0, 1.0 - wz), (z1, wz)):
        for y, ay in ((y0, 1.0 - wy), (y1, wy)):
            for x, ax in ((x0, 1.0 - wx), (x1, wx)):
                term = ((az * ay) * ax)[..., None] * volume[nn, z, y, x]
                out = term if out is None else out + term
    return out


def scale_space_predict_reference(x, flow, num_levels=5, sigma0=1.5):
    """`scale_space_predict` as the composition of the two twins."""
    return scale_space_warp_reference(gaussian_scale_space_reference(x, num_levels, sigma0), flow)


# -------------------------------------------------------------------------------------------------------------------
# the kernels


def _volume_kernel(x, num_levels, sigma0):
    n, h, w, c = x.shape
    volume = torch.empty(n, num_levels + 1, h, w, c, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().tfc_scale_space_volume(x.data_ptr(), volume.data_ptr(), n, h, w, c, num_levels, sigma0,
                                                 _lib.stream_ptr()))
    return volume


def _warp_kernel(volume, flow):
    n, planes, h, w, c = volume.shape
    out = torch.empty(n, h, w, c, dtype=torch.float32, device=volume.device)
    _lib.check(_lib.lib().tfc_scale_space_warp_forward(volume.data_ptr(), flow.data_ptr(), out.data_ptr(), n, h, w, c,
                                                       planes - 1, _lib.stream_ptr()))
    return out


def _warp_backward_kernel(g, volume, flow, want_flow, want_volume, want_x, sigma0):
    n, planes, h, w, c = volume.shape
    g = g.to(torch.float32).contiguous()
    g_flow = torch.empty_like(flow) if want_flow else None
    g_volume = torch.empty_like(volume) if want_volume else None
    g_x = torch.empty(n, h, w, c, dtype=torch.float32, device=g.device) if want_x else None
    _lib.check(_lib.lib().tfc_scale_space_warp_backward(
        g.data_ptr(), volume.data_ptr(), flow.data_ptr(), _ptr(g_flow), _ptr(g_volume), _ptr(g_x), sigma0, n, h, w, c,
        planes - 1, _lib.stream_ptr()))
    return g_flow, g_volume, g_x


class _VolumeFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, num_levels, sigma0):
        ctx.levels, ctx.sigma0 = num_levels, sigma0
        return _volume_kernel(x, num_levels, sigma0)

    @staticmethod
    def backward(ctx, g):
        g = g.to(torch.float32).contiguous()
        n, _, h, w, c = g.shape
        g_x = torch.empty(n, h, w, c, dtype=torch.float32, device=g.device)
        _lib.check(_lib.lib().tfc_scale_space_volume_backward(g.data_ptr(), g_x.data_ptr(), n, h, w, c, ctx.levels,
                                                              ctx.sigma0, _lib.stream_ptr()))
        return g_x, None, None


class _WarpFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, volume, flow):
        ctx.save_for_backward(volume, flow)
        return _warp_kernel(volume, flow)

    @staticmethod
    def backward(ctx, g):
        volume, flow = ctx.saved_tensors
        g_flow, g_volume, _ = _warp_backward_kernel(g, volume, flow, ctx.needs_input_grad[1], ctx.needs_input_grad[0],
                                                    False, 1.0)
        return g_volume, g_flow


class _PredictFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, flow, num_levels, sigma0):
        volume = _volume_kernel(x, num_levels, sigma0)
        ctx.save_for_backward(volume, flow)
        ctx.sigma0 = sigma0
        return _warp_kernel(volume, flow)

    @staticmethod
    def backward(ctx, g):
        volume, flow = ctx.saved_tensors
        g_flow, _, g_x = _warp_backward_kernel(g, volume, flow, ctx.needs_input_grad[1], False,
                                               ctx.needs_input_grad[0], ctx.sigma0)
        return g_x, g_flow, None, None


def gaussian_scale_space(x, num_levels=5, sigma0=1.5):
    """x [N, H, W, C] float32 -> the scale-space volume [N, num_levels + 1, H, W, C] on the HIP kernels (two launches for
    all planes), differentiable in x.  CPU tensors and float64 take `gaussian_scale_space_reference`."""
    _check_image(x, "gaussian_scale_space")
    num_levels, sigma0 = _check_levels(num_levels, sigma0)
    if not _on_kernels(x):
        return gaussian_scale_space_reference(x, num_levels, sigma0)
    return _VolumeFunction.apply(x, num_levels, sigma0)


def scale_space_warp(volume, flow):
    """volume [N, M + 1, H, W, C], flow [N, H, W, 3] = (dx, dy, s), float32 -> [N, H, W, C] on the HIP kernels,
    differentiable in both; the gradients are bit-identical from call to call.  The volume gradient needs
    H W <= 2^22.  CPU tensors and float64 take `scale_space_warp_reference`."""
    _check_volume_flow(volume, flow, "scale_space_warp")
    if not _on_kernels(volume, flow):
        return scale_space_warp_reference(volume, flow)
    return _WarpFunction.apply(volume, flow)


def scale_space_predict(x, flow, num_levels=5, sigma0=1.5):
    """scale_space_warp(gaussian_scale_space(x, num_levels, sigma0), flow), the same bits, in one call; the backward
    reads the fixed-point volume gradient directly, the float one never exists."""
    _check_image(x, "scale_space_predict")
    num_levels, sigma0 = _check_levels(num_levels, sigma0)
    _check_flow(flow, x.shape[:3], "scale_space_predict")
    if flow.dtype != x.dtype:
        raise TypeError(f"scale_space_predict: x and flow must share a dtype, got {x.dtype} and {flow.dtype}")
    if flow.device != x.device:
        raise ValueError("scale_space_predict: x and flow must be on the same device")
    if not _on_kernels(x, flow):
        return scale_space_predict_reference(x, flow, num_levels, sigma0)
    return _PredictFunction.apply(x, flow, num_levels, sigma0)

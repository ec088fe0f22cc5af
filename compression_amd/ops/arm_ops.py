"""The rate of an autoregressive-MLP entropy model (the ARM of the overfitted codecs: Ladune et al., Cool-chic; Kim et
al., C3).  The definition is this project's own; parity with anyone's checkpoints is unpinned.

For every pixel (i, j) of a latent grid y [B, H, W]:

    h0[k]      = y[i + di_k, j + dj_k],  k < C         the C nearest causal neighbours (`arm_context_offsets`), 0 outside
    h          <- relu(h W_l + b_l) + h,  l < L         w [L, C, C], b [L, C]
    (mu, s)    = h W_out + b_out                        w_out [C, 2], b_out [2]
    scale      = exp(clamp(s, S_MIN, S_MAX))            the gradient is zero outside the clamp
    p          = the Laplace(mu, scale) mass of [y - 1/2, y + 1/2]
    bits       = -log2(max(p, 2^-16))                   the gradient is zero under the floor

and the result is `bits` summed per grid, [B].  With x = y - mu, a = |x| and r = 1 / scale the mass is taken as
differences of survival values on the side of mu where both ends lie, which keeps its relative error in the tails:

    a >= 1/2 :  p = exp(-(a - 1/2) r) (1 - exp(-r)) / 2
    a <  1/2 :  p = -(expm1(-(1/2 - a) r) + expm1(-(1/2 + a) r)) / 2

`arm_bits` runs tfc_arm_bits_forward / tfc_arm_bits_backward (csrc/arm_bits.hip): no [N, C] tensor exists in the forward
pass, a grid's bits do not depend on B, and both directions are bit-identical from call to call.
`arm_bits_reference` is the same definition as tensor ops in the caller's dtype; CPU tensors and float64 take it."""
from __future__ import annotations

import os
import re

import torch
import torch.nn.functional as F

from .. import _lib
from .._lib import ptr as _ptr

__all__ = ["arm_context_offsets", "arm_bits", "arm_bits_reference", "ARM_CONSTANTS", "ARM_CONTEXTS", "S_MIN", "S_MAX",
           "P_FLOOR"]

ARM_CONSTANTS = _lib.kernel_constants("arm_params.h", ("ARM",))
ARM_CONTEXTS = (8, 16, 24, 32)


def _read_header():
    """The two offset tables and the clamp ends of csrc/arm_params.h, where they stand once."""
    with open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "arm_params.h")) as f:
        text = f.read()
    tables = {}
    for name in ("ARM_DI", "ARM_DJ"):
        body = re.search(r"constexpr\s+int\s+%s\[32\]\s*=\s*\{([^}]*)\}" % name, text).group(1)
        tables[name] = tuple(int(v) for v in body.split(","))
        assert len(tables[name]) == 32
    ends = {name: float(re.search(r"constexpr\s+float\s+%s\s*=\s*(-?[0-9.]+)f\s*;" % name, text).group(1))
            for name in ("ARM_S_MIN", "ARM_S_MAX")}
    return tuple(zip(tables["ARM_DI"], tables["ARM_DJ"])), ends["ARM_S_MIN"], ends["ARM_S_MAX"]


_OFFSETS, S_MIN, S_MAX = _read_header()
P_FLOOR = 2.0 ** -ARM_CONSTANTS["ARM_FLOOR_LOG2"]


def arm_context_offsets(context):
    """The first `context` offsets (di, dj) of the causal half-plane (di < 0, or di == 0 and dj < 0) by ascending
    di^2 + dj^2, then di descending, then dj ascending."""
    if context not in ARM_CONTEXTS:
        raise ValueError(f"the context size must be one of {ARM_CONTEXTS}, got {context!r}")
    return _OFFSETS[:context]


def _check(y, w, b, w_out, b_out):
    if y.dim() != 3:
        raise ValueError(f"y must be [B, H, W], received shape {tuple(y.shape)}")
    if w.dim() != 3 or w.shape[1] != w.shape[2]:
        raise ValueError(f"w must be [L, C, C], received shape {tuple(w.shape)}")
    layers, c = w.shape[0], w.shape[1]
    if c not in ARM_CONTEXTS:
        raise ValueError(f"the context size must be one of {ARM_CONTEXTS}, got {c}")
    if not 1 <= layers <= ARM_CONSTANTS["ARM_MAX_L"]:
        raise ValueError(f"hidden layers must be in [1, {ARM_CONSTANTS['ARM_MAX_L']}], got {layers}")
    if tuple(b.shape) != (layers, c) or tuple(w_out.shape) != (c, 2) or tuple(b_out.shape) != (2,):
        raise ValueError(f"b, w_out, b_out must be [{layers}, {c}], [{c}, 2], [2], received {tuple(b.shape)}, "
                         f"{tuple(w_out.shape)}, {tuple(b_out.shape)}")
    for name, t in (("w", w), ("b", b), ("w_out", w_out), ("b_out", b_out)):
        if t.dtype != y.dtype or t.device != y.device:
            raise ValueError(f"{name} must share y's dtype and device")
    return layers, c


def arm_bits_reference(y, w, b, w_out, b_out, want_params=False):
    """The definition as differentiable tensor ops in y's dtype -> bits [B], or (bits, mu, scale).  This one does hold
    the [B, H, W, C] context."""
    bits, mu, scale, _ = _arm_terms(y, w, b, w_out, b_out)
    return (bits, mu, scale) if want_params else bits


def _arm_terms(y, w, b, w_out, b_out):
    """-> (bits, mu, scale, where the kinks lie: the pre-ReLU activations "pre" (one [B, H, W, C] per layer), "s", "p")."""
    _, c = _check(y, w, b, w_out, b_out)
    halo = ARM_CONSTANTS["ARM_HALO"]
    height, width = y.shape[1:]
    padded = F.pad(y, (halo, halo, halo, 0))
    h = torch.stack([padded[:, halo + di:halo + di + height, halo + dj:halo + dj + width]
                     for di, dj in arm_context_offsets(c)], dim=-1)
    pre = []
    for wl, bl in zip(w, b):
        pre.append(h @ wl + bl)
        h = torch.relu(pre[-1]) + h
    out = h @ w_out + b_out
    mu, s = out[..., 0], out[..., 1]
    sc = s.clamp(S_MIN, S_MAX)
    r = torch.exp(-sc)
    a = (y - mu).abs()
    # each branch's arguments are held where the other is taken, so that neither differentiates an overflow
    tail = 0.5 * torch.exp(-(a - 0.5).clamp_min(0.0) * r) * -torch.expm1(-r)
    centre = -0.5 * (torch.expm1(-(0.5 - a).clamp_min(0.0) * r) + torch.expm1(-(0.5 + a) * r))
    p = torch.where(a >= 0.5, tail, centre)
    bits = -torch.log2(p.clamp_min(P_FLOOR)).sum(dim=(1, 2))
    return bits, mu, torch.exp(sc), {"pre": [t.detach() for t in pre], "s": s.detach(), "p": p.detach()}


class _ArmBitsFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, want_params, y, w, b, w_out, b_out):
        y, w, b, w_out, b_out = (t.contiguous() for t in (y, w, b, w_out, b_out))
        batch, height, width = y.shape
        layers, c = w.shape[0], w.shape[1]
        bits = torch.empty(batch, dtype=torch.float32, device=y.device)
        mu = torch.empty_like(y) if want_params else None
        scale = torch.empty_like(y) if want_params else None
        _lib.check(_lib.lib().tfc_arm_bits_forward(
            y.data_ptr(), w.data_ptr(), b.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), batch, height, width, c, layers,
            bits.data_ptr(), _ptr(mu), _ptr(scale), _lib.stream_ptr()))
        ctx.save_for_backward(y, w, b, w_out, b_out)
        if not want_params:
            mu = scale = torch.empty(0, dtype=torch.float32, device=y.device)
        ctx.mark_non_differentiable(mu, scale)
        return bits, mu, scale

    @staticmethod
    def backward(ctx, g_bits, _g_mu, _g_scale):
        y, w, b, w_out, b_out = ctx.saved_tensors
        batch, height, width = y.shape
        layers, c = w.shape[0], w.shape[1]
        need_y, need_p = ctx.needs_input_grad[1], any(ctx.needs_input_grad[2:])
        if not (need_y or need_p):
            return (None,) * 6
        n_w, n_b = layers * c * c, layers * c
        d_y = torch.empty_like(y) if need_y else None
        d_params = torch.empty(n_w + n_b + 2 * c + 2, dtype=torch.float32, device=y.device) if need_p else None
        g = g_bits.to(torch.float32).contiguous()
        _lib.check(_lib.lib().tfc_arm_bits_backward(
            y.data_ptr(), w.data_ptr(), b.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), g.data_ptr(), batch, height,
            width, c, layers, _ptr(d_y), _ptr(d_params), _lib.stream_ptr()))
        d_w = d_b = d_wo = d_bo = None
        if need_p:
            d_w, d_b = d_params[:n_w].view(layers, c, c), d_params[n_w:n_w + n_b].view(layers, c)
            d_wo, d_bo = d_params[n_w + n_b:n_w + n_b + 2 * c].view(c, 2), d_params[n_w + n_b + 2 * c:]
        return None, d_y, d_w, d_b, d_wo, d_bo


def arm_bits(y, w, b, w_out, b_out, want_params=False):
    """y [B, H, W], w [L, C, C], b [L, C], w_out [C, 2], b_out [2], float32 on the device -> bits [B] on the HIP kernels,
    differentiable in all five; with `want_params` also mu and scale [B, H, W] (not differentiable).  The shape limits
    (B <= 65535, H W < 2^31) are the C entry's, reported as a ValueError before any launch.  CPU tensors and other
    dtypes take `arm_bits_reference`."""
    _check(y, w, b, w_out, b_out)
    if not y.is_cuda or y.dtype != torch.float32:
        out = arm_bits_reference(y, w, b, w_out, b_out, want_params)
        return (out[0], out[1].detach(), out[2].detach()) if want_params else out
    bits, mu, scale = _ArmBitsFunction.apply(bool(want_params), y, w, b, w_out, b_out)
    return (bits, mu, scale) if want_params else bits

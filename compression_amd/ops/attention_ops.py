"""Shifted-window attention and the two small operations a Swin block needs beside it (layer norm, exact GELU).

The definition of `window_attention` is this project's own (include/tfc_hip.h, tfc_window_attention_forward); parity
with anyone's checkpoints is not pinned.

    qkv [B, H, W, 3 C], C = heads d: channel which C + head d + j holds q (which = 0), k (1), v (2)
    table [heads, (2 ws - 1)^2] float32, window size ws, shift s (0 or ws / 2) -> out [B, H, W, C]

    Hp = ceil(H / ws) ws, Wp likewise.  Window (wy, wx), token (ty, tx) sits at rolled coordinate
    r = (wy ws + ty, wx ws + tx); its source is (yp, xp) = ((r_y + s) mod Hp, (r_x + s) mod Wp); it is valid iff
    yp < H and xp < W; its wrap flags are (r_y + s >= Hp, r_x + s >= Wp).
    S_ij = d^-1/2 q_i . k_j + table[head, (ty_i - ty_j + ws - 1) (2 ws - 1) + (tx_i - tx_j + ws - 1)]
    A key j takes part iff it is valid and has the wrap flags of i; every other key has weight exactly 0.
    P_i = softmax over the keys that take part; out_i = sum_j P_ij v_j, written at (yp, xp).

`window_attention` runs tfc_window_attention_forward / _backward (csrc/window_attention.hip): one kernel that reads
qkv once and writes out once (float32: fmaf chains; bfloat16: both products on the bf16 MFMA with float32
accumulation, softmax in float32, exp(S - max) rounded to bfloat16 before P.V), and a deterministic backward that
recomputes S and P.  `window_attention_reference` is
the same definition as differentiable tensor ops (pad, roll, partition, masked softmax, and back); CPU tensors take it.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .. import _lib
from .._lib import ptr as _ptr

__all__ = ["window_attention", "window_attention_reference", "layer_norm", "layer_norm_reference", "gelu",
           "gelu_reference", "WA_CONSTANTS", "SUPPORTED_WINDOWS", "SUPPORTED_HEAD_DIMS"]

# the named constants of csrc/window_attention_params.h (windows per workgroup, the dtable partial count)
WA_CONSTANTS = _lib.kernel_constants("window_attention_params.h", ("WA",))

SUPPORTED_WINDOWS = (4, 8)
SUPPORTED_HEAD_DIMS = (16, 32)


def _check_args(qkv, table, heads, window, shift, dtypes):
    if window not in SUPPORTED_WINDOWS:
        raise ValueError(f"window_attention supports window sizes {SUPPORTED_WINDOWS} and head dimensions "
                         f"{SUPPORTED_HEAD_DIMS}, got window {window}")
    if shift not in (0, window // 2):
        raise ValueError(f"shift must be 0 or window / 2 = {window // 2}, got {shift}")
    if not isinstance(heads, int) or heads < 1:
        raise ValueError(f"heads must be a positive integer, got {heads!r}")
    if qkv.dim() != 4 or min(qkv.shape[:3]) < 1:
        raise ValueError(f"qkv must be [B, H, W, 3 C] with B, H, W >= 1, received shape {tuple(qkv.shape)}")
    if qkv.shape[-1] % (3 * heads):
        raise ValueError(f"the last axis of qkv ({qkv.shape[-1]}) must be 3 * heads * d with heads = {heads}")
    d = qkv.shape[-1] // (3 * heads)
    if d not in SUPPORTED_HEAD_DIMS:
        raise ValueError(f"window_attention supports window sizes {SUPPORTED_WINDOWS} and head dimensions "
                         f"{SUPPORTED_HEAD_DIMS}, got head dimension {d}")
    if tuple(table.shape) != (heads, (2 * window - 1) ** 2):
        raise ValueError(f"table must be [{heads}, {(2 * window - 1) ** 2}], received shape {tuple(table.shape)}")
    if qkv.dtype not in dtypes:
        raise TypeError(f"window_attention supports {' and '.join(str(t) for t in dtypes)}, got qkv of {qkv.dtype}")
    return d


def _relative_index(window, device):
    """[T, T] int64: the table entry of (query i, key j)."""
    t = torch.arange(window * window, device=device)
    ty, tx = t // window, t % window
    return (ty[:, None] - ty[None, :] + window - 1) * (2 * window - 1) + (tx[:, None] - tx[None, :] + window - 1)


def window_attention_reference(qkv, table, heads, window, shift=0):
    """The definition as differentiable tensor ops in the dtype of qkv (float64 stays float64; bfloat16 is the bf16
    composition): zero-pad to (Hp, Wp), roll by -shift, partition, softmax over the keys that take part, and back."""
    d = _check_args(qkv, table, heads, window, shift, (torch.float32, torch.float64, torch.bfloat16))
    b, h, w, _ = qkv.shape
    ws, dev = window, qkv.device
    nwy, nwx = -(-h // ws), -(-w // ws)
    hp, wp = nwy * ws, nwx * ws
    x = F.pad(qkv, (0, 0, 0, wp - w, 0, hp - h))
    x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    # the class of a rolled coordinate: -1 invalid, else 2 wrap_y + wrap_x
    sy, sx = torch.arange(hp, device=dev) + shift, torch.arange(wp, device=dev) + shift
    cls = (sy >= hp).long()[:, None] * 2 + (sx >= wp).long()[None, :]
    valid = ((sy % hp) < h)[:, None] & ((sx % wp) < w)[None, :]
    cls = torch.where(valid, cls, torch.full_like(cls, -1))
    cls = cls.reshape(nwy, ws, nwx, ws).permute(0, 2, 1, 3).reshape(nwy, nwx, ws * ws)
    take = (cls[..., :, None] == cls[..., None, :]) & (cls[..., :, None] >= 0)            # [nwy, nwx, T, T]
    # (a padded query has no key: give it itself, its row is cropped away below)
    take = take | ((cls[..., :, None] < 0) & torch.eye(ws * ws, dtype=torch.bool, device=dev))
    x = x.reshape(b, nwy, ws, nwx, ws, 3, heads, d).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, b, nwy, nwx, heads, ws * ws, d)
    q, k, v = x[0], x[1], x[2]
    bias = table.to(qkv.dtype)[:, _relative_index(ws, dev)]                                # [heads, T, T]
    s = torch.matmul(q, k.transpose(-1, -2)) * (1.0 / math.sqrt(d)) + bias
    mask = take[None, :, :, None]
    s = s.masked_fill(~mask, float("-inf"))
    p = torch.softmax(s, dim=-1)
    out = torch.matmul(p, v)             # exp(-inf) = 0: an excluded key has weight exactly 0
    out = out.reshape(b, nwy, nwx, heads, ws, ws, d).permute(0, 1, 4, 2, 5, 3, 6).reshape(b, hp, wp, heads * d)
    out = torch.roll(out, shifts=(shift, shift), dims=(1, 2))
    return out[:, :h, :w].contiguous()


class _WindowAttentionFunction(torch.autograd.Function):
    """tfc_window_attention_forward / tfc_window_attention_backward.  A gradient nobody needs is not computed."""

    @staticmethod
    def forward(ctx, qkv, table, heads, window, shift):
        qkv = qkv.contiguous()
        table32 = table.detach().to(torch.float32).contiguous()
        b, h, w, c3 = qkv.shape
        out = torch.empty(b, h, w, c3 // 3, dtype=qkv.dtype, device=qkv.device)
        _lib.check(_lib.lib().tfc_window_attention_forward(
            qkv.data_ptr(), table32.data_ptr(), out.data_ptr(), _lib.DTYPE_CODE[qkv.dtype], b, h, w, heads,
            c3 // (3 * heads), window, shift, _lib.stream_ptr()))
        ctx.save_for_backward(qkv, table32)
        ctx.cfg = (heads, window, shift, table.dtype)
        return out

    @staticmethod
    def backward(ctx, grad):
        qkv, table32 = ctx.saved_tensors
        heads, window, shift, table_dtype = ctx.cfg
        need_qkv, need_table = ctx.needs_input_grad[:2]
        b, h, w, c3 = qkv.shape
        dqkv = torch.empty_like(qkv) if need_qkv else None
        dtable = torch.empty_like(table32) if need_table else None
        if need_qkv or need_table:
            grad = grad.to(qkv.dtype).contiguous()
            _lib.check(_lib.lib().tfc_window_attention_backward(
                qkv.data_ptr(), table32.data_ptr(), grad.data_ptr(), _ptr(dqkv), _ptr(dtable),
                _lib.DTYPE_CODE[qkv.dtype], b, h, w, heads, c3 // (3 * heads), window, shift, _lib.stream_ptr()))
        if dtable is not None:
            dtable = dtable.to(table_dtype)
        return dqkv, dtable, None, None, None


def window_attention(qkv, table, heads, window, shift=0):
    """qkv [B, H, W, 3 heads d] float32 or bfloat16, table [heads, (2 window - 1)^2] -> out [B, H, W, heads d] on the
    fused kernel; differentiable in qkv and table.  window in {4, 8}, d in {16, 32}, shift 0 or window / 2.  CPU
    tensors (float64 too) take `window_attention_reference`."""
    if not qkv.is_cuda:
        return window_attention_reference(qkv, table, heads, window, shift)
    _check_args(qkv, table, heads, window, shift, tuple(_lib.DTYPE_CODE))
    if table.device != qkv.device:
        raise ValueError("qkv and table must be on the same device")
    return _WindowAttentionFunction.apply(qkv, table, heads, window, shift)


# ---- layer norm --------------------------------------------------------------------------------------------------

def layer_norm_reference(x, gamma, beta, epsilon=1e-5, residual=None):
    """Layer norm over the last axis as tensor ops: biased variance, (x - mean) rsqrt(var + epsilon) gamma + beta, then
    `+ residual`; statistics in float32 (a float64 input stays float64)."""
    ft = torch.float64 if x.dtype == torch.float64 else torch.float32
    xf = x.to(ft)
    mean = xf.mean(dim=-1, keepdim=True)
    cen = xf - mean
    var = (cen * cen).mean(dim=-1, keepdim=True)
    y = cen * torch.rsqrt(var + epsilon)
    if gamma is not None:
        y = y * gamma.to(ft)
    if beta is not None:
        y = y + beta.to(ft)
    if residual is not None:
        y = y + residual.to(ft)
    return y.to(x.dtype)


def _layer_norm_args(x, gamma, beta, epsilon):
    if x.dtype not in _lib.DTYPE_CODE:
        raise TypeError(f"layer_norm supports float32 and bfloat16 on the device, got {x.dtype}")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"x must be [..., C] with C >= 1, received shape {tuple(x.shape)}")
    if not (math.isfinite(float(epsilon)) and float(epsilon) >= 0):
        raise ValueError(f"epsilon must be finite and non-negative, got {epsilon}")
    c = x.shape[-1]
    params = []
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            if tuple(t.shape) != (c,):
                raise ValueError(f"{name} shape {tuple(t.shape)} does not match C={c}")
            t = t.detach().to(x.device, torch.float32).contiguous()
        params.append(t)
    return x.contiguous(), params[0], params[1], c


class _LayerNormFunction(torch.autograd.Function):
    """tfc_layer_norm_forward / tfc_layer_norm_backward; the residual's gradient is the incoming one."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, epsilon):
        xc, g32, b32, c = _layer_norm_args(x, gamma, beta, epsilon)
        if residual is not None:
            if residual.shape != x.shape:
                raise ValueError(f"residual shape {tuple(residual.shape)} does not match the input's {tuple(x.shape)}")
            residual = residual.detach().to(x.dtype).contiguous()
        y = torch.empty_like(xc)
        _lib.check(_lib.lib().tfc_layer_norm_forward(
            xc.data_ptr(), _ptr(g32), _ptr(b32), _ptr(residual), y.data_ptr(), _lib.DTYPE_CODE[x.dtype],
            xc.numel() // c, c, float(epsilon), _lib.stream_ptr()))
        ctx.save_for_backward(xc, g32, b32)
        ctx.cfg = (float(epsilon), residual is not None, None if gamma is None else gamma.dtype,
                   None if beta is None else beta.dtype)
        return y

    @staticmethod
    def backward(ctx, grad):
        x, g32, b32 = ctx.saved_tensors
        epsilon, has_residual, gamma_dtype, beta_dtype = ctx.cfg
        c = x.shape[-1]
        need_x, need_g, need_b = ctx.needs_input_grad[:3]
        dx = dgamma = dbeta = None
        if need_x or need_g or need_b:
            g = grad.to(x.dtype).contiguous()
            dx = torch.empty_like(x)
            dgamma = torch.empty(c, dtype=torch.float32, device=x.device) if need_g else None
            dbeta = torch.empty(c, dtype=torch.float32, device=x.device) if need_b else None
            _lib.check(_lib.lib().tfc_layer_norm_backward(
                x.data_ptr(), g.data_ptr(), _ptr(g32), _ptr(b32), dx.data_ptr(), _ptr(dgamma), _ptr(dbeta),
                _lib.DTYPE_CODE[x.dtype], x.numel() // c, c, epsilon, _lib.stream_ptr()))
            dgamma = None if dgamma is None else dgamma.to(gamma_dtype)
            dbeta = None if dbeta is None else dbeta.to(beta_dtype)
        return (dx if need_x else None), dgamma, dbeta, (grad if has_residual else None), None


def layer_norm(x, gamma, beta, epsilon=1e-5, residual=None):
    """Layer norm over the last axis of x [..., C] on the fused kernel (the ChannelNorm kernels with the biased variance):
    gamma / beta [C] or None, then `+ residual` if given.  Differentiable in x, gamma, beta and residual.  CPU tensors
    take `layer_norm_reference`."""
    if not x.is_cuda:
        return layer_norm_reference(x, gamma, beta, epsilon, residual)
    if x.numel() == 0:
        return torch.empty_like(x)
    return _LayerNormFunction.apply(x, gamma, beta, residual, float(epsilon))


# ---- GELU --------------------------------------------------------------------------------------------------------

def gelu_reference(x):
    """0.5 x (1 + erf(x / sqrt 2)) as tensor ops, in float32 (a float64 input stays float64)."""
    ft = torch.float64 if x.dtype == torch.float64 else torch.float32
    xf = x.to(ft)
    return (0.5 * xf * (1.0 + torch.erf(xf * (1.0 / math.sqrt(2.0))))).to(x.dtype)


class _GeluFunction(torch.autograd.Function):
    """tfc_gelu_forward / tfc_gelu_backward."""

    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        y = torch.empty_like(x)
        _lib.check(_lib.lib().tfc_gelu_forward(x.data_ptr(), y.data_ptr(), _lib.DTYPE_CODE[x.dtype], x.numel(),
                                               _lib.stream_ptr()))
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        g = grad.to(x.dtype).contiguous()
        dx = torch.empty_like(x)
        _lib.check(_lib.lib().tfc_gelu_backward(x.data_ptr(), g.data_ptr(), dx.data_ptr(), _lib.DTYPE_CODE[x.dtype],
                                                x.numel(), _lib.stream_ptr()))
        return dx


def gelu(x):
    """Exact GELU on the fused kernel (float32 or bfloat16), differentiable.  CPU tensors take `gelu_reference`."""
    if not x.is_cuda:
        return gelu_reference(x)
    if x.dtype not in _lib.DTYPE_CODE:
        raise TypeError(f"gelu supports float32 and bfloat16 on the device, got {x.dtype}")
    return _GeluFunction.apply(x)

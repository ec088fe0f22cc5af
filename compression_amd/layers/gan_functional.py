"""Launchers and autograd wrappers of csrc/hific_gan.hip (include/tfc_hip.h, "HiFiC discriminator and GAN loss"):
spectral normalisation, the discriminator's front end, leaky ReLU behind a convolution, the non-saturating loss."""
from __future__ import annotations

import torch

from .. import _lib
from . import functional
from .functional import _DTYPE_CODE

__all__ = ["LRELU_SLOPE", "SN_EPSILON", "nearest_source", "nearest_first", "spectral_norm_forward",
           "spectral_norm_backward", "spectral_norm", "disc_front_forward", "disc_front_backward", "disc_front",
           "disc_front_composite", "lrelu_", "lrelu_bias_backward", "conv2d_bias_lrelu", "gan_loss_forward",
           "gan_loss_backward", "gan_losses"]

LRELU_SLOPE = 0.2
SN_EPSILON = 1e-12


def nearest_source(dst, size_in, size_out):
    """Source index of a nearest-neighbour resize, in integers: min(floor((2 dst + 1) in / (2 out)), in - 1)."""
    return min((2 * dst + 1) * size_in // (2 * size_out), size_in - 1)


def nearest_first(src, size_in, size_out):
    """The first destination index whose source is >= src (what the backward kernel walks from); `size_out` for src =
    size_in."""
    if src <= 0:
        return 0
    return max(0, min(size_out, -(-(2 * size_out * src - size_in) // (2 * size_in))))


def _dtype_code(t, what):
    _lib.require_device()
    if t.dtype not in _DTYPE_CODE:
        raise TypeError(f"{what} supports float32 and bfloat16, got {t.dtype}")
    return _DTYPE_CODE[t.dtype]


def _f32(t):
    return t.detach().to(torch.float32).contiguous()


def spectral_norm_forward(kernel, u):
    """tfc_spectral_norm_forward: kernel [..., cout] float32, u [rows] or [rows, 1] -> (kernel / sigma in the kernel's
    shape, u' [rows], v [cout], sigma [1])."""
    device = _lib.require_device()
    w, u = _f32(kernel).to(device), _f32(u).to(device).reshape(-1)
    cols = w.shape[-1]
    rows = w.numel() // cols
    if u.numel() != rows:
        raise ValueError(f"u has {u.numel()} entries, the kernel has {rows} rows")
    w_sn, u_new = torch.empty_like(w), torch.empty_like(u)
    v = torch.empty(cols, dtype=torch.float32, device=w.device)
    sigma = torch.empty(1, dtype=torch.float32, device=w.device)
    _lib.check(_lib.lib().tfc_spectral_norm_forward(
        w.data_ptr(), u.data_ptr(), rows, cols, w_sn.data_ptr(), u_new.data_ptr(), v.data_ptr(), sigma.data_ptr(),
        _lib.stream_ptr()))
    return w_sn, u_new, v, sigma


def spectral_norm_backward(grad, kernel, u_new, v, sigma):
    """tfc_spectral_norm_backward: dL/d(kernel / sigma) -> dL/dkernel with u' and v constant."""
    _lib.require_device()
    g, w = _f32(grad), _f32(kernel)
    cols = w.shape[-1]
    dw = torch.empty_like(w)
    _lib.check(_lib.lib().tfc_spectral_norm_backward(
        g.data_ptr(), w.data_ptr(), u_new.data_ptr(), v.data_ptr(), sigma.data_ptr(), w.numel() // cols, cols,
        dw.data_ptr(), _lib.stream_ptr()))
    return dw


class _SpectralNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kernel, u):
        w_sn, u_new, v, sigma = spectral_norm_forward(kernel, u)
        ctx.save_for_backward(kernel, u_new, v, sigma)
        ctx.mark_non_differentiable(u_new)
        return w_sn, u_new

    @staticmethod
    def backward(ctx, grad, _):
        kernel, u_new, v, sigma = ctx.saved_tensors
        return spectral_norm_backward(grad, kernel, u_new, v, sigma).to(kernel.dtype), None


def spectral_norm(kernel, u):
    """(kernel / sigma, u') of one power iteration from u; differentiable in the kernel."""
    if torch.is_grad_enabled() and kernel.requires_grad:
        return _SpectralNormFunction.apply(kernel, u)
    return spectral_norm_forward(kernel, u)[:2]


def _front_args(x, latent, padded_channels):
    code = _dtype_code(x, "the discriminator front end")
    if x.dim() != 4 or latent.dim() != 4 or x.shape[0] != latent.shape[0]:
        raise ValueError(f"x [N, H, W, c] and latent [N, h, w, c'] expected, got {tuple(x.shape)}, {tuple(latent.shape)}")
    if latent.dtype != x.dtype:
        raise TypeError(f"x is {x.dtype}, latent is {latent.dtype}")
    n, H, W, cx = x.shape
    _, h, w, cl = latent.shape
    return code, (n, H, W, h, w, cx, cl, int(padded_channels))


def disc_front_forward(x, latent, padded_channels):
    """tfc_disc_front_forward: x | lrelu(latent) resized to x's extent | zeros, [N, H, W, padded_channels]."""
    code, dims = _front_args(x, latent, padded_channels)
    x, latent = x.contiguous(), latent.contiguous()
    out = torch.empty(x.shape[:3] + (int(padded_channels),), dtype=x.dtype, device=x.device)
    _lib.check(_lib.lib().tfc_disc_front_forward(x.data_ptr(), latent.data_ptr(), out.data_ptr(), code, *dims,
                                                 _lib.stream_ptr()))
    return out


def disc_front_backward(grad, latent, image_channels):
    """tfc_disc_front_backward: dL/dout -> (dx, dlatent)."""
    code = _dtype_code(grad, "the discriminator front end")
    grad, latent = grad.contiguous(), latent.to(grad.dtype).contiguous()
    n, H, W, P = grad.shape
    _, h, w, cl = latent.shape
    dx = torch.empty((n, H, W, image_channels), dtype=grad.dtype, device=grad.device)
    dlatent = torch.empty_like(latent)
    _lib.check(_lib.lib().tfc_disc_front_backward(
        grad.data_ptr(), latent.data_ptr(), dx.data_ptr(), dlatent.data_ptr(), code, n, H, W, h, w, image_channels, cl,
        P, _lib.stream_ptr()))
    return dx, dlatent


class _DiscFrontFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, latent, padded_channels):
        ctx.save_for_backward(latent)
        ctx.cx = x.shape[-1]
        return disc_front_forward(x, latent, padded_channels)

    @staticmethod
    def backward(ctx, grad):
        latent, = ctx.saved_tensors
        dx, dlatent = disc_front_backward(grad, latent, ctx.cx)
        return dx, dlatent, None


def disc_front(x, latent, padded_channels):
    """The discriminator's input from the image and the latent branch's convolution output (archs.py:342-345), with
    the zero channels the next convolution wants; differentiable in both."""
    if torch.is_grad_enabled() and (x.requires_grad or latent.requires_grad):
        return _DiscFrontFunction.apply(x, latent, padded_channels)
    return disc_front_forward(x, latent, padded_channels)


class _NearestResizeFunction(torch.autograd.Function):
    """Nearest-neighbour resize of [N, h, w, C] to H x W as a gather.  Its backward is a SUM over each source pixel's
    replicas; written out here as tensor ops in the order tfc_disc_front_backward adds them (replica k = row-major
    position in the source's rectangle; four running sums over k = q, q + 4, ..., combined as (s0 + s2) + (s1 + s3)), so
    that the composite and the fused launch give the same bits in float32, not merely close sums."""

    @staticmethod
    def forward(ctx, t, H, W):
        h, w = t.shape[1:3]
        ctx.sizes = (h, w, H, W)
        iy = torch.tensor([nearest_source(d, h, H) for d in range(H)], device=t.device)
        ix = torch.tensor([nearest_source(d, w, W) for d in range(W)], device=t.device)
        return t[:, iy[:, None], ix[None, :]]

    @staticmethod
    def backward(ctx, grad):
        h, w, H, W = ctx.sizes
        y0 = torch.tensor([nearest_first(s, h, H) for s in range(h + 1)])
        x0 = torch.tensor([nearest_first(s, w, W) for s in range(w + 1)])
        rows, cols = y0[1:] - y0[:-1], x0[1:] - x0[:-1]
        count = rows[:, None] * cols[None, :]                                   # [h, w]
        steps = max(1, -(-int(count.max()) // 4))
        k = torch.arange(4 * steps)
        dy = k[None, None, :] // cols.clamp(min=1)[None, :, None]
        dx = k[None, None, :] - dy * cols[None, :, None]
        valid = (k[None, None, :] < count[:, :, None]).to(grad.device)
        Y = (y0[:-1, None, None] + dy).clamp(max=H - 1).expand(h, w, -1).to(grad.device)
        X = (x0[None, :-1, None] + dx).clamp(max=W - 1).expand(h, w, -1).to(grad.device)
        parts = grad[:, Y, X] * valid[None, :, :, :, None]                      # [N, h, w, 4 steps, C]
        parts = parts.reshape(parts.shape[:3] + (steps, 4, parts.shape[-1]))
        s = parts[:, :, :, 0]
        for j in range(1, steps):
            s = s + parts[:, :, :, j]
        return (s[..., 0, :] + s[..., 2, :]) + (s[..., 1, :] + s[..., 3, :]), None, None


def disc_front_composite(x, latent, padded_channels):
    """The same as tensor ops: leaky_relu, a gather with the integer source indexes, cat, pad.  The gather runs on
    float32 copies (exact both ways), so that its backward adds the replicas' gradients in float32."""
    act = torch.nn.functional.leaky_relu(latent, LRELU_SLOPE)
    out = torch.cat([x.float(), _NearestResizeFunction.apply(act.float(), x.shape[1], x.shape[2])], dim=-1)
    return torch.nn.functional.pad(out, (0, int(padded_channels) - out.shape[-1])).to(x.dtype)


def lrelu_(y):
    """tfc_lrelu_forward: y = max(y, 0.2 y) in place on a contiguous tensor."""
    code = _dtype_code(y, "leaky ReLU")
    if not y.is_contiguous():
        raise ValueError("lrelu_ works in place on a contiguous tensor")
    _lib.check(_lib.lib().tfc_lrelu_forward(y.data_ptr(), code, y.numel(), _lib.stream_ptr()))
    return y


def lrelu_bias_backward(gy, y=None, bias=True):
    """tfc_lrelu_bias_backward over [..., C]: y given -> (gy * (y > 0 ? 1 : 0.2), its sum per channel); y None -> (gy,
    the sum of gy per channel).  bias=False: no sums (None)."""
    code = _dtype_code(gy, "leaky ReLU")
    gy = gy.contiguous()
    C = gy.shape[-1]
    masked = y is not None
    if masked:
        y = y.contiguous()
        if y.shape != gy.shape or y.dtype != gy.dtype:
            raise ValueError(f"gy {tuple(gy.shape)} {gy.dtype} and y {tuple(y.shape)} {y.dtype} differ")
    if not masked and not bias:
        return gy, None
    gm = torch.empty_like(gy) if masked else gy
    db = torch.empty(C, dtype=torch.float32, device=gy.device) if bias else None
    _lib.check(_lib.lib().tfc_lrelu_bias_backward(
        gy.data_ptr(), y.data_ptr() if masked else None, gm.data_ptr() if masked else None,
        None if db is None else db.data_ptr(), code, gy.numel() // C, C, int(masked), _lib.stream_ptr()))
    return gm, db


class _ConvBiasLreluFunction(torch.autograd.Function):
    """Convolution + bias (+ leaky ReLU) on the project's launchers: the forward kernel, then the activation in place;
    backward: one pass for the masked gradient and the bias sums, the transposed kernel for dx, the weight-gradient
    kernel for dw."""

    @staticmethod
    def forward(ctx, x, kernel, bias, stride, lrelu):
        y = functional._conv(x, kernel, bias, stride, None, False)
        if lrelu:
            lrelu_(y)
        ctx.save_for_backward(x, kernel, y if lrelu else None)
        ctx.meta = (stride, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, kernel, y = ctx.saved_tensors
        stride, has_bias = ctx.meta
        gm, db = lrelu_bias_backward(gy.to(x.dtype), y, bias=has_bias and ctx.needs_input_grad[2])
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = functional._conv(gm, kernel.transpose(-1, -2), None, stride, None, True)[:, :x.shape[1], :x.shape[2]]
        if ctx.needs_input_grad[1]:
            dw = functional.conv2d_wgrad(x, gm, tuple(kernel.shape[:2]), stride, False).to(kernel.dtype)
        return dx, dw, db, None, None


def conv2d_bias_lrelu(x, kernel, bias, stride=1, activation=None, weights_key=0, lrelu=False):
    """`functional.conv2d_down` (same arguments; `activation` must be None) with leaky ReLU behind it when `lrelu`."""
    if activation is not None:
        raise ValueError("conv2d_bias_lrelu takes its activation as `lrelu`")
    needs = torch.is_grad_enabled() and (x.requires_grad or kernel.requires_grad
                                         or (bias is not None and bias.requires_grad))
    if needs:
        return _ConvBiasLreluFunction.apply(x, kernel, bias, int(stride), bool(lrelu))
    y = functional._conv(x, kernel, bias, stride, None, False, weights_key=weights_key)
    return lrelu_(y) if lrelu else y


def _logit_args(logits):
    code = _dtype_code(logits, "the GAN loss")
    logits = logits.contiguous().reshape(-1)
    if logits.numel() < 2 or logits.numel() % 2:
        raise ValueError(f"logits hold a real and a fake half, got {logits.numel()} values")
    return code, logits


def gan_loss_forward(logits):
    """tfc_gan_loss_forward: logits [2 M], real half first -> float32 [4]: d_loss, g_loss, mean sigmoid(real), mean
    sigmoid(fake)."""
    code, flat = _logit_args(logits)
    out = torch.empty(4, dtype=torch.float32, device=flat.device)
    _lib.check(_lib.lib().tfc_gan_loss_forward(flat.data_ptr(), code, flat.numel() // 2, out.data_ptr(),
                                               _lib.stream_ptr()))
    return out


def gan_loss_backward(logits, scale, mode):
    """tfc_gan_loss_backward: the gradient of d_loss (mode "d_loss") or g_loss ("g_loss") times `scale` (a scalar
    tensor), in the logits' shape and dtype."""
    code, flat = _logit_args(logits)
    scale = scale.detach().to(flat.device, torch.float32).reshape(1).contiguous()
    grad = torch.empty_like(flat)
    _lib.check(_lib.lib().tfc_gan_loss_backward(flat.data_ptr(), scale.data_ptr(), code, flat.numel() // 2,
                                                {"d_loss": 0, "g_loss": 1}[mode], grad.data_ptr(), _lib.stream_ptr()))
    return grad.reshape(logits.shape)


class _GanLossFunction(torch.autograd.Function):
    """logits -> [d_loss, g_loss, d_real, d_fake]; backward: the two losses' gradients, each times its incoming one."""

    @staticmethod
    def forward(ctx, logits):
        ctx.save_for_backward(logits)
        return gan_loss_forward(logits)

    @staticmethod
    def backward(ctx, g):
        logits, = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        return gan_loss_backward(logits, g[0:1], "d_loss") + gan_loss_backward(logits, g[1:2], "g_loss")


def gan_losses(logits):
    """compare_gan's non_saturating loss (model.py:616-638) of the discriminator's logits, real half first:
    (d_loss, g_loss, mean sigmoid(real), mean sigmoid(fake)), float32 scalars from one launch; d_loss and g_loss are
    differentiable in the logits."""
    if torch.is_grad_enabled() and logits.requires_grad:
        out = _GanLossFunction.apply(logits)
    else:
        out = gan_loss_forward(logits)
    return out[0], out[1], out[2].detach(), out[3].detach()

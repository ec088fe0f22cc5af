"""The layers of a Swin transformer transform ("Transformer-based Transform Coding", Zhu, Yang and Cohen, ICLR 2022) on
channels-last activations [B, H, W, C], which already are token grids: layer norm, shifted-window attention, the
block around them, and the patch merge / split that change the resolution.

The attention is `ops.attention_ops.window_attention` (this project's own definition; parity with anyone's checkpoints
is not pinned), the norm and the GELU are the fused kernels beside it, and every linear layer is a 1x1 `KerasConv2D` on
the MFMA convolution kernels.  CPU tensors evaluate the same formulas as tensor ops (float64 stays float64): that is the
checker's path, not a fallback of the device path."""
from __future__ import annotations

import torch

from ..ops import attention_ops
from .keras_conv import KerasConv2D

__all__ = ["LayerNorm", "WindowAttention", "SwinBlock", "PatchMerge", "PatchSplit"]


class LayerNorm(torch.nn.Module):
    """Per token, normalise over the channel (last) axis with the biased variance, scale by `gamma`, shift by `beta`;
    `forward(x, residual=r)` adds r in the same launch."""

    def __init__(self, num_channels, epsilon=1e-5):
        super().__init__()
        self.epsilon = float(epsilon)
        self.gamma = torch.nn.Parameter(torch.ones(int(num_channels)))
        self.beta = torch.nn.Parameter(torch.zeros(int(num_channels)))

    def forward(self, x, residual=None):
        if x.shape[-1] != self.gamma.shape[0]:
            raise ValueError(f"LayerNorm of {self.gamma.shape[0]} channels, input has {x.shape[-1]}")
        return attention_ops.layer_norm(x, self.gamma, self.beta, self.epsilon, residual)

    def extra_repr(self):
        return f"{self.gamma.shape[0]}, epsilon={self.epsilon}"


class _Linear(KerasConv2D):
    """A linear layer over the channel axis of [B, H, W, C]: a 1x1 convolution with a bias."""

    def __init__(self, cin, cout):
        super().__init__(cout, 1, 1, in_channels=cin)

    def forward(self, x):
        if x.is_cuda:
            return super().forward(x)
        return x @ self.kernel[0, 0].to(x.dtype) + self.bias.to(x.dtype)


class WindowAttention(torch.nn.Module):
    """Multi-head attention inside (shifted) windows of `window` x `window` tokens with a learned relative-position
    table [heads, (2 window - 1)^2]: qkv projection, `window_attention`, output projection."""

    def __init__(self, dim, heads, window, shift=0):
        super().__init__()
        if dim % heads:
            raise ValueError(f"heads ({heads}) must divide dim ({dim})")
        if window not in attention_ops.SUPPORTED_WINDOWS or dim // heads not in attention_ops.SUPPORTED_HEAD_DIMS:
            raise ValueError(f"window_attention supports window sizes {attention_ops.SUPPORTED_WINDOWS} and head "
                             f"dimensions {attention_ops.SUPPORTED_HEAD_DIMS}, got window {window} and head dimension "
                             f"{dim // heads}")
        if shift not in (0, window // 2):
            raise ValueError(f"shift must be 0 or window / 2 = {window // 2}, got {shift}")
        self.dim, self.heads, self.window, self.shift = int(dim), int(heads), int(window), int(shift)
        self.qkv = _Linear(dim, 3 * dim)
        self.proj = _Linear(dim, dim)
        self.table = torch.nn.Parameter(torch.nn.init.trunc_normal_(torch.empty(heads, (2 * window - 1) ** 2), std=0.02))

    def forward(self, x):
        out = attention_ops.window_attention(self.qkv(x).contiguous(), self.table, self.heads, self.window, self.shift)
        return self.proj(out)

    def extra_repr(self):
        return f"dim={self.dim}, heads={self.heads}, window={self.window}, shift={self.shift}"


class SwinBlock(torch.nn.Module):
    """x + attn(norm(x)), then x + mlp(norm(x)) with mlp = linear (mlp_ratio x), exact GELU, linear."""

    def __init__(self, dim, heads, window, shift=0, mlp_ratio=4):
        super().__init__()
        self.norm1 = LayerNorm(dim)
        self.attn = WindowAttention(dim, heads, window, shift)
        self.norm2 = LayerNorm(dim)
        self.fc1 = _Linear(dim, mlp_ratio * dim)
        self.fc2 = _Linear(mlp_ratio * dim, dim)

    def forward(self, x):
        x = x + self.attn(self.norm1(x))
        return x + self.fc2(attention_ops.gelu(self.fc1(self.norm2(x)).contiguous()))


def _blocks(dim, depth, head_dim, window):
    """`depth` blocks that alternate shift 0 and window / 2."""
    return torch.nn.Sequential(*[SwinBlock(dim, dim // head_dim, window, (window // 2) * (k % 2)) for k in range(depth)])


class PatchMerge(torch.nn.Module):
    """Halves the resolution: 2x2 space-to-depth (channel (dy 2 + dx) C + c), norm, linear to `cout`.  An odd extent gets
    one zero row or column first."""

    def __init__(self, cin, cout):
        super().__init__()
        self.norm = LayerNorm(4 * cin)
        self.reduce = _Linear(4 * cin, cout)

    def forward(self, x):
        b, h, w, c = x.shape
        if h % 2 or w % 2:
            x = torch.nn.functional.pad(x, (0, 0, 0, w % 2, 0, h % 2))
            h, w = h + h % 2, w + w % 2
        x = x.reshape(b, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h // 2, w // 2, 4 * c)
        return self.reduce(self.norm(x.contiguous()))


class PatchSplit(torch.nn.Module):
    """Doubles the resolution: linear to 4 `cout`, norm, depth-to-space (the inverse layout of `PatchMerge`)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.expand = _Linear(cin, 4 * cout)
        self.norm = LayerNorm(4 * cout)

    def forward(self, x):
        b, h, w, _ = x.shape
        x = self.norm(self.expand(x).contiguous())
        c = x.shape[-1] // 4
        return x.reshape(b, h, w, 2, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * h, 2 * w, c).contiguous()

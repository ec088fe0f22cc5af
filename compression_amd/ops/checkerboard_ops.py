"""The checkerboard context model of He, Zheng, Sun, Wang and Qin, "Checkerboard context model for efficient learned
image compression" (CVPR 2021) as two passes that are parallel over positions (csrc/checkerboard.hip).

The reference tree holds no program text for this model: the definition, the stream format and the layer shapes are
this project's own, and parity with anyone's checkpoints is unpinned.

Definition, with y [B, Hl, Wl, M] the latent, psi [B, Hl, Wl, P] the hyper-synthesis output and y_hat zero outside the
latent.  Position (i, j) is an anchor when i + j is even; pass 0 is the anchors, pass 1 the rest:

    taps       = (di, dj) in [-2, 2]^2 with di + dj odd, row-major: 12 taps, all anchors as seen from a pass-1 position
    ctx[i, j]  = bc                                                             pass 0
               = bc + sum over the taps of y_hat[i + di, j + dj] @ Wc[di + 2, dj + 2]      pass 1         M -> 2M
    out        = b3 + lrelu(b2 + lrelu(b1 + [ctx, psi] @ W1) @ W2) @ W3                    slope 0.2
    mu, index  = out[:M], out[M:]         idx = int32(min(max(index, 0), num_scales - 1))
    sym        = rint(y - mu)  (half to even)        y_hat = float32(sym) + mu

Compact order: the positions of one pass in raster order, channels innermost, [B, N_p, M] with N_0 = ceil(Hl Wl / 2)
and N_1 = floor(Hl Wl / 2); the slot of (i, j) is (i Wl + j) >> 1 when Wl is odd and i (Wl / 2) + (j >> 1) when it is
even.  Per image there are two code streams, pass 0 then pass 1: what `LocationScaleIndexedEntropyModel(...,
coding_rank=2).compress(y - mu, index)` writes for the compact tensor of the pass.

`checkerboard_scan` is the encoder side and the evaluation (two launches), `checkerboard_decode` the decoder side
(parameters of pass 0, decompress, place, parameters of pass 1, decompress, place), `checkerboard_scan_reference` and
`checkerboard_parameters_reference` the definition as tensor ops for any float dtype and for CPU tensors."""
from __future__ import annotations

import collections

import numpy as np
import torch

from .. import _lib
from . import context_ops
from .context_ops import ContextParams, _check_inputs, _index_prepare, _network, tap_sum

__all__ = ["CHECKER_TAPS", "CHECKERBOARD_CONSTANTS", "CheckerboardParams", "CheckerboardScan", "anchor_mask",
           "checkerboard_mask", "checkerboard_split", "checkerboard_merge", "checkerboard_parameters",
           "checkerboard_parameters_reference", "checkerboard_place", "checkerboard_scan", "checkerboard_scan_reference",
           "checkerboard_decode", "pass_positions"]

CheckerboardScan = collections.namedtuple("CheckerboardScan", ["sym", "idx", "mu", "y_hat", "index_float"])

# (di, dj) of the taps in the kernels' order: row-major over the 5x5 window, the elements with di + dj odd
CHECKER_TAPS = tuple((di, dj) for di in range(-2, 3) for dj in range(-2, 3) if (di + dj) % 2)

# the named constants of the checkerboard kernels in csrc/context_params.h
CHECKERBOARD_CONSTANTS = _lib.kernel_constants("context_params.h", ("CKB",))
assert context_ops.CONTEXT_CONSTANTS["CTX_TAPS"] == len(CHECKER_TAPS)
# the header's numbering: packed tap k is element 2 k + 1 of the window
assert all((di + 2) * 5 + dj + 2 == 2 * k + 1 for k, (di, dj) in enumerate(CHECKER_TAPS))


class CheckerboardParams(ContextParams):
    """`ContextParams` with the checkerboard mask and tap list: the same arguments, checks, cache and packed layout
    (csrc/context_params.h), the 12 x M rows of `wc` holding `CHECKER_TAPS` in order."""

    TAPS = CHECKER_TAPS

    def fits_kernel(self):
        """Whether the activations of one tile of positions fit the kernel's LDS (csrc/context_params.h, ckb_check)."""
        c = CHECKERBOARD_CONSTANTS
        return super().fits_kernel() and (self._ab_rows() + c["CKB_STAGE_K"]) * c["CKB_TILE"] <= c["CKB_LDS_FLOATS"]


def checkerboard_mask(dtype=torch.float32, device=None):
    """[5, 5, 1, 1]: 1 on the 12 taps with di + dj odd, 0 on the centre and the other 12."""
    return context_ops.tap_mask(CHECKER_TAPS, dtype, device)


def anchor_mask(hl, wl, device=None):
    """bool [Hl, Wl]: True where i + j is even (pass 0)."""
    i = torch.arange(int(hl), device=device)[:, None]
    j = torch.arange(int(wl), device=device)[None, :]
    return (i + j) % 2 == 0


def pass_positions(hl, wl, pass_):
    """N_p: ceil(Hl Wl / 2) anchors, floor(Hl Wl / 2) others."""
    return (int(hl) * int(wl) + (1 if pass_ == 0 else 0)) // 2


def _check_pass(pass_):
    if pass_ not in (0, 1):
        raise ValueError(f"pass_ must be 0 or 1, got {pass_!r}")
    return int(pass_)


def checkerboard_split(t):
    """t [B, Hl, Wl, C] -> (pass 0 [B, N_0, C], pass 1 [B, N_1, C]) in compact order."""
    if t.dim() != 4:
        raise ValueError(f"t must be [B, Hl, Wl, C], received shape {tuple(t.shape)}")
    b, hl, wl, c = t.shape
    anchors = anchor_mask(hl, wl, t.device).reshape(-1)
    flat = t.reshape(b, hl * wl, c)
    return flat[:, anchors].contiguous(), flat[:, ~anchors].contiguous()


def checkerboard_merge(a, b, hl, wl):
    """The inverse of `checkerboard_split`: (a [B, N_0, C], b [B, N_1, C]) -> [B, Hl, Wl, C]."""
    hl, wl = int(hl), int(wl)
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise ValueError(f"a and b must be [B, N_0, C] and [B, N_1, C], received {tuple(a.shape)} and {tuple(b.shape)}")
    if a.shape[1] != pass_positions(hl, wl, 0) or b.shape[1] != pass_positions(hl, wl, 1):
        raise ValueError(f"a {hl} x {wl} latent has {pass_positions(hl, wl, 0)} and {pass_positions(hl, wl, 1)} "
                         f"positions per pass, received {a.shape[1]} and {b.shape[1]}")
    anchors = anchor_mask(hl, wl, a.device).reshape(-1)
    out = torch.empty(a.shape[0], hl * wl, a.shape[2], dtype=a.dtype, device=a.device)
    out[:, anchors] = a
    out[:, ~anchors] = b.to(a.dtype)
    return out.reshape(a.shape[0], hl, wl, a.shape[2])


def _check(y, psi, params, what="y"):
    _check_inputs(y, psi, params, what, kind=CheckerboardParams)


def checkerboard_parameters_reference(y_hat, psi, params):
    """The parallel (teacher-forced) definition -> (mu, index_float), each [B, Hl, Wl, M] in the full layout: anchors get
    the bias alone as their context, the other positions the bias and the taps over `y_hat`."""
    _check(y_hat, psi, params, "y_hat")
    w = params.tensors(y_hat.dtype, y_hat.device)
    b, hl, wl, m = y_hat.shape
    conv = tap_sum(torch.zeros(b, hl, wl, 2 * m, dtype=y_hat.dtype, device=y_hat.device), y_hat, w[0], CHECKER_TAPS)
    others = (~anchor_mask(hl, wl, y_hat.device)).to(y_hat.dtype)[None, :, :, None]
    out = _network(w[1] + conv * others, psi, w)
    return out[..., :m], out[..., m:]


def checkerboard_scan_reference(y, psi, params):
    """The definition, pass after pass -> CheckerboardScan(sym int32, idx int32, mu, y_hat, index_float) in the full
    layout.  Any float dtype, any device."""
    _check(y, psi, params)
    b, hl, wl, m = y.shape
    anchors = anchor_mask(hl, wl, y.device)[None, :, :, None]
    mu0, _ = checkerboard_parameters_reference(torch.zeros_like(y), psi, params)
    decoded = torch.where(anchors, torch.round(y - mu0) + mu0, torch.zeros_like(y))
    mu, index_float = checkerboard_parameters_reference(decoded, psi, params)
    r = torch.round(y - mu)
    return CheckerboardScan(r.to(torch.int32), _index_prepare(index_float, params.num_scales), mu, r + mu, index_float)


def _on_kernel(t):
    return t.is_cuda and t.dtype == torch.float32


def _launch_params(pass_, y, y_hat, psi, params):
    """One tfc_checkerboard_params call -> (mu, index_float, idx, sym or None), compact."""
    b, hl, wl, _ = psi.shape
    n = pass_positions(hl, wl, pass_)
    packed = params.packed(psi.device)
    mu = torch.empty(b, n, params.m, dtype=torch.float32, device=psi.device)
    index_float = torch.empty_like(mu)
    idx = torch.empty(mu.shape, dtype=torch.int32, device=psi.device)
    sym = torch.empty_like(idx) if y is not None else None
    _lib.check(_lib.lib().tfc_checkerboard_params(
        pass_, None if y is None else y.data_ptr(), y_hat.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(),
        b, hl, wl, params.m, params.p, params.h1, params.h2, params.num_scales, mu.data_ptr(), index_float.data_ptr(),
        idx.data_ptr(), None if sym is None else sym.data_ptr(), _lib.stream_ptr()))
    return mu, index_float, idx, sym


def checkerboard_parameters(y_hat, psi, params, pass_):
    """(mu, index_float) of one pass in compact order, [B, N_pass, M], given `y_hat` [B, Hl, Wl, M] (read at the anchors
    by pass 1, not at all by pass 0).  float32 device tensors run tfc_checkerboard_params; CPU tensors and other float
    dtypes take `checkerboard_parameters_reference`."""
    _check(y_hat, psi, params, "y_hat")
    pass_ = _check_pass(pass_)
    if not _on_kernel(y_hat):
        mu, index_float = checkerboard_parameters_reference(y_hat, psi, params)
        return checkerboard_split(mu)[pass_], checkerboard_split(index_float)[pass_]
    mu, index_float, _, _ = _launch_params(pass_, None, y_hat.detach().contiguous(), psi.detach().contiguous(), params)
    return mu, index_float


def checkerboard_place(sym, mu, y_hat, pass_):
    """y_hat[positions of the pass] = float32(sym) + mu, in place, from compact `sym` and `mu` [B, N_pass, M]."""
    pass_ = _check_pass(pass_)
    b, hl, wl, m = y_hat.shape
    if tuple(sym.shape) != (b, pass_positions(hl, wl, pass_), m) or tuple(mu.shape) != tuple(sym.shape):
        raise ValueError(f"sym and mu must be [{b}, {pass_positions(hl, wl, pass_)}, {m}], received "
                         f"{tuple(sym.shape)} and {tuple(mu.shape)}")
    if not (_on_kernel(y_hat) and y_hat.is_contiguous()):
        anchors = anchor_mask(hl, wl, y_hat.device).reshape(-1)
        y_hat.view(b, hl * wl, m)[:, anchors if pass_ == 0 else ~anchors] = sym.to(y_hat.dtype) + mu.to(y_hat.dtype)
        return y_hat
    sym, mu = sym.to(torch.float32).contiguous(), mu.contiguous()
    _lib.check(_lib.lib().tfc_checkerboard_place(pass_, sym.data_ptr(), mu.data_ptr(), y_hat.data_ptr(), b, hl, wl, m,
                                                 _lib.stream_ptr()))
    return y_hat


def _scan_compact(y, psi, params):
    """The two launches -> (y_hat full, [(mu, index_float, idx, sym) of pass 0, of pass 1])."""
    y_hat = torch.zeros_like(y)
    passes = [_launch_params(pass_, y, y_hat, psi, params) for pass_ in (0, 1)]
    return y_hat, passes


def checkerboard_scan(y, psi, params):
    """y [B, Hl, Wl, M], psi [B, Hl, Wl, P] -> CheckerboardScan(sym int32, idx int32, mu, y_hat, index_float) in the
    full layout: float32 device tensors run tfc_checkerboard_params twice; CPU tensors and other float dtypes take
    `checkerboard_scan_reference`."""
    _check(y, psi, params)
    if not _on_kernel(y):
        return checkerboard_scan_reference(y, psi, params)
    y, psi = y.detach().contiguous(), psi.detach().contiguous()
    hl, wl = y.shape[1:3]
    y_hat, (a, b) = _scan_compact(y, psi, params)
    mu, index_float, idx, sym = (checkerboard_merge(u, v, hl, wl) for u, v in zip(a, b))
    return CheckerboardScan(sym, idx, mu, y_hat, index_float)


def checkerboard_decode(strings, psi, params, entropy_model):
    """The strings [B, 2] (pass 0 and pass 1 of every image: what `entropy_model.compress(y - mu, index_float)` writes
    for the compact tensors of a pass), psi [B, Hl, Wl, P] float32 on the device and the
    `LocationScaleIndexedEntropyModel` (coding_rank 2) that wrote them -> y_hat [B, Hl, Wl, M].  A latent of one
    position has no second pass: its second string is not read."""
    _check(None, psi, params)
    if not _on_kernel(psi):
        raise ValueError("checkerboard_decode needs float32 psi on the device")
    psi = psi.detach().contiguous()
    b, hl, wl, _ = psi.shape
    strings = np.asarray(strings, dtype=object)
    if strings.shape != (b, 2):
        raise ValueError(f"strings must have shape [{b}, 2] (pass 0 and pass 1 of every image), received "
                         f"{list(strings.shape)}")
    y_hat = torch.zeros(b, hl, wl, params.m, dtype=torch.float32, device=psi.device)
    for pass_ in (0, 1):
        if pass_positions(hl, wl, pass_) == 0:
            continue
        mu, index_float, _, _ = _launch_params(pass_, None, y_hat, psi, params)
        sym = entropy_model.decompress(strings[:, pass_], index_float)
        checkerboard_place(sym, mu, y_hat, pass_)
    return y_hat

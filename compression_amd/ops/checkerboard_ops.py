"""The checkerboard context model of He, Zheng, Sun, Wang and Qin, "Checkerboard context model for efficient learned
image compression" (CVPR 2021) as two passes that are parallel over positions.  It runs as the one-group case of the
space-channel model's kernels (csrc/space_channel.hip; c_g = 0, M_g = M, one stream per pass), and the launch sites and
the scan, encode and decode loops of both models are the ones in this file.

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

`checkerboard_scan` is the encoder side and the evaluation (two launches), `checkerboard_encode` writes the two strings
of a scan, `checkerboard_decode` is the decoder side (parameters of pass 0, decompress, place, parameters of pass 1,
decompress, place), `checkerboard_scan_reference` and `checkerboard_parameters_reference` the definition as tensor ops
for any float dtype and for CPU tensors."""
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
           "checkerboard_decode", "checkerboard_encode", "pass_positions"]

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


# ---- streams: consecutive compact slots of one pass (ops/scctx_ops.py; the checkerboard model has one per pass) -------

def _check_stream_positions(stream_positions):
    if int(stream_positions) != stream_positions or int(stream_positions) < 1:
        raise ValueError(f"stream_positions must be an integer >= 1, got {stream_positions!r}")
    return int(stream_positions)


def stream_split(t, stream_positions):
    """A compact tensor [B, N, C] -> (full [B, S_full, stream_positions, C] or None, last [B, 1, r, C] or None): the
    streams of stream_positions slots and the shorter last one."""
    sp = _check_stream_positions(stream_positions)
    if t.dim() != 3:
        raise ValueError(f"t must be [B, N, C], received shape {tuple(t.shape)}")
    b, n, c = t.shape
    s_full = n // sp
    full = t[:, :s_full * sp].reshape(b, s_full, sp, c) if s_full else None
    last = t[:, s_full * sp:].reshape(b, 1, n - s_full * sp, c) if n > s_full * sp else None
    return full, last


def stream_merge(full, last):
    """The inverse of `stream_split` -> [B, N, C]."""
    parts = [v.reshape(v.shape[0], -1, v.shape[3]) for v in (full, last) if v is not None]
    if not parts:
        raise ValueError("stream_merge needs at least one part")
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)


# ---- the kernels: both models run csrc/space_channel.hip, the checkerboard model as its one-group case ----------------
# `steps` holds, per channel group in coding order, (own, packed, c_g): the group's CheckerboardParams, its packed buffer
# on the device and its first channel; [(params, packed, 0)], one group that is the whole latent, for this model.

def _launch_params(pass_, y, y_hat, psi, own, packed, c_g):
    """One tfc_scctx_params call for the M_g channels from c_g of `y_hat` -> (mu, index_float, idx, sym or None),
    compact [B, N_pass, M_g]."""
    (b, hl, wl, _), m = psi.shape, y_hat.shape[3]
    n = pass_positions(hl, wl, pass_)
    mu = torch.empty(b, n, own.m, dtype=torch.float32, device=psi.device)
    index_float = torch.empty_like(mu)
    idx = torch.empty(mu.shape, dtype=torch.int32, device=psi.device)
    sym = torch.empty_like(idx) if y is not None else None
    _lib.check(_lib.lib().tfc_scctx_params(
        pass_, None if y is None else y.data_ptr(), y_hat.data_ptr(), psi.data_ptr(), packed.data_ptr(), packed.numel(),
        b, hl, wl, m, c_g, own.m, own.p, own.h1, own.h2, own.num_scales, mu.data_ptr(), index_float.data_ptr(),
        idx.data_ptr(), None if sym is None else sym.data_ptr(), _lib.stream_ptr()))
    return mu, index_float, idx, sym


def _scan_steps(y, psi, steps):
    """Two launches per group -> (sym, idx, mu, y_hat, index_float) in the full layout."""
    hl, wl = y.shape[1:3]
    y_hat = torch.zeros_like(y)
    per_group = []
    for own, packed, c_g in steps:
        a, b = (_launch_params(pass_, y, y_hat, psi, own, packed, c_g) for pass_ in (0, 1))
        per_group.append([checkerboard_merge(u, v, hl, wl) for u, v in zip(a, b)])
    mu, index_float, idx, sym = per_group[0] if len(per_group) == 1 else (
        torch.cat([group[k] for group in per_group], dim=-1) for k in range(4))
    return sym, idx, mu, y_hat, index_float


def _encode_steps(residual, index, spans, stream_positions, entropy_model):
    """The strings of residual and index [B, Hl, Wl, M], object array [B, T] in the order group, pass, stream: per
    (c_g, M_g) of `spans` and pass, the full streams go through one `compress` call as [B, S_full, stream_positions,
    M_g], a shorter last stream through a second."""
    columns = []
    for c, mg in spans:
        r_g = checkerboard_split(residual[..., c:c + mg].contiguous())
        i_g = checkerboard_split(index[..., c:c + mg].contiguous())
        for pass_ in (0, 1):
            for r, i in zip(stream_split(r_g[pass_], stream_positions), stream_split(i_g[pass_], stream_positions)):
                if r is not None:
                    strings = entropy_model.compress(r.contiguous(), i.contiguous())
                    columns.append(np.asarray(strings, dtype=object).reshape(residual.shape[0], -1))
    return np.concatenate(columns, axis=1)


def _decode_steps(strings, psi, steps, m, stream_positions, entropy_model):
    """strings [B, T] -> y_hat [B, Hl, Wl, m].  Per group and pass: the parameters (one launch), one `decompress` call
    for the full streams and one for a shorter last stream, the store."""
    b, hl, wl, _ = psi.shape
    y_hat = torch.zeros(b, hl, wl, m, dtype=torch.float32, device=psi.device)
    at = 0
    for own, packed, c_g in steps:
        for pass_ in (0, 1):
            if pass_positions(hl, wl, pass_) == 0:
                continue
            mu, index_float, _, _ = _launch_params(pass_, None, y_hat, psi, own, packed, c_g)
            parts = []
            for part in stream_split(index_float, stream_positions):
                if part is not None:
                    s = part.shape[1]
                    part = entropy_model.decompress(strings[:, at:at + s], part.contiguous())
                    at += s
                parts.append(part)
            checkerboard_place(stream_merge(*parts), mu, y_hat, pass_, c_g)
    return y_hat


def checkerboard_parameters(y_hat, psi, params, pass_):
    """(mu, index_float) of one pass in compact order, [B, N_pass, M], given `y_hat` [B, Hl, Wl, M] (read at the anchors
    by pass 1, not at all by pass 0).  float32 device tensors run tfc_checkerboard_params' kernel (tfc_scctx_params with
    one group); CPU tensors and other float dtypes take `checkerboard_parameters_reference`."""
    _check(y_hat, psi, params, "y_hat")
    pass_ = _check_pass(pass_)
    if not _on_kernel(y_hat):
        mu, index_float = checkerboard_parameters_reference(y_hat, psi, params)
        return checkerboard_split(mu)[pass_], checkerboard_split(index_float)[pass_]
    return _launch_params(pass_, None, y_hat.detach().contiguous(), psi.detach().contiguous(), params,
                          params.packed(psi.device), 0)[:2]


def checkerboard_place(sym, mu, y_hat, pass_, c_g=0):
    """y_hat[positions of the pass, c_g : c_g + M_g] = float32(sym) + mu, in place, from compact `sym` and `mu`
    [B, N_pass, M_g]: the whole depth M of y_hat for the checkerboard model, a channel group for ops/scctx_ops.py."""
    pass_ = _check_pass(pass_)
    b, hl, wl, m = y_hat.shape
    n, c_g = pass_positions(hl, wl, pass_), int(c_g)
    if sym.dim() != 3 or tuple(sym.shape[:2]) != (b, n) or tuple(mu.shape) != tuple(sym.shape):
        raise ValueError(f"sym and mu must be [{b}, {n}, M_g], received {tuple(sym.shape)} and {tuple(mu.shape)}")
    mg = int(sym.shape[2])
    if c_g < 0 or mg < 1 or c_g + mg > m:
        raise ValueError(f"the group must lie inside the latent: c_g {c_g}, M_g {mg}, M {m}")
    if not (_on_kernel(y_hat) and y_hat.is_contiguous()):
        anchors = anchor_mask(hl, wl, y_hat.device).reshape(-1)
        y_hat.view(b, hl * wl, m)[:, anchors if pass_ == 0 else ~anchors, c_g:c_g + mg] = (
            sym.to(y_hat.dtype) + mu.to(y_hat.dtype))
        return y_hat
    sym, mu = sym.to(torch.float32).contiguous(), mu.contiguous()
    _lib.check(_lib.lib().tfc_scctx_place(pass_, sym.data_ptr(), mu.data_ptr(), y_hat.data_ptr(), b, hl, wl, m, c_g, mg,
                                          _lib.stream_ptr()))
    return y_hat


def checkerboard_scan(y, psi, params):
    """y [B, Hl, Wl, M], psi [B, Hl, Wl, P] -> CheckerboardScan(sym int32, idx int32, mu, y_hat, index_float) in the
    full layout: float32 device tensors run the kernel twice; CPU tensors and other float dtypes take
    `checkerboard_scan_reference`."""
    _check(y, psi, params)
    if not _on_kernel(y):
        return checkerboard_scan_reference(y, psi, params)
    y, psi = y.detach().contiguous(), psi.detach().contiguous()
    return CheckerboardScan(*_scan_steps(y, psi, [(params, params.packed(psi.device), 0)]))


def checkerboard_encode(y, scan, entropy_model):
    """The strings of a scan, object array [B, 2]: pass 0 and pass 1 of every image, each what
    `entropy_model.compress(y - mu, index_float)` writes for the compact tensors of the pass."""
    hl, wl, m = y.shape[1:]
    return _encode_steps(y - scan.mu, scan.index_float, [(0, m)], max(1, pass_positions(hl, wl, 0)), entropy_model)


def checkerboard_decode(strings, psi, params, entropy_model):
    """The strings [B, 2] (pass 0 and pass 1 of every image: `checkerboard_encode`), psi [B, Hl, Wl, P] float32 on the
    device and the `LocationScaleIndexedEntropyModel` (coding_rank 2) that wrote them -> y_hat [B, Hl, Wl, M].  A latent
    of one position has no second pass: its second string is not read."""
    _check(None, psi, params)
    if not _on_kernel(psi):
        raise ValueError("checkerboard_decode needs float32 psi on the device")
    psi = psi.detach().contiguous()
    b, hl, wl, _ = psi.shape
    strings = np.asarray(strings, dtype=object)
    if strings.shape != (b, 2):
        raise ValueError(f"strings must have shape [{b}, 2] (pass 0 and pass 1 of every image), received "
                         f"{list(strings.shape)}")
    return _decode_steps(strings, psi, [(params, params.packed(psi.device), 0)], params.m,
                         max(1, pass_positions(hl, wl, 0)), entropy_model)          # a whole pass is one stream



"""The space-channel context model ("SCCTX") after He, Yang, Peng, Mao, Qin and Wang, "ELIC: efficient learned image
compression with unevenly grouped space-channel contextual adaptive coding" (CVPR 2022): the latent's channels are cut
into unevenly sized groups, the checkerboard of ops/checkerboard_ops.py runs inside every group, and a group sees all
earlier groups (csrc/space_channel.hip).

The reference tree holds no program text for this model: the definition, the stream format and the layer shapes are
this project's own, and parity with anyone's checkpoints is unpinned.

Definition, with y [B, Hl, Wl, M] the latent, psi [B, Hl, Wl, P] the hyper-synthesis output, y_hat zero outside the
latent, groups = (M_0, ..., M_{G-1}) with sum M and c_g = M_0 + ... + M_{g-1}.  Anchors (i + j even) are pass 0, the
other positions pass 1; the coding order is group 0 pass 0, group 0 pass 1, group 1 pass 0, ...: 2 G steps, each
parallel over positions.  Step (g, pass) at a position of the pass:

    ctx_g = bc_g
          + sum over ALL 25 taps (di, dj) of the 5x5 window, row-major, channels c < c_g ascending:
                y_hat[i + di, j + dj, c] * Wch_g[di + 2, dj + 2, c, :]                  (nothing for g = 0)
          + pass 1 only: sum over the 12 checkerboard taps (CHECKER_TAPS, row-major), channels of the group ascending:
                y_hat[i + di, j + dj, c_g + c] * Wsp_g[di + 2, dj + 2, c, :]                              -> 2 M_g
    out   = b3_g + lrelu(b2_g + lrelu(b1_g + [ctx_g, psi] W1_g) W2_g) W3_g       slope 0.2                -> 2 M_g
    mu, index = out[:M_g], out[M_g:]      idx = index_prepare(index, num_scales)
    sym   = rint(y[.., c_g + c] - mu)  (half to even)        y_hat[.., c_g + c] = float32(sym) + mu

With G = 1 this is the checkerboard model, term for term and in the same order.

Streams.  The compact order of a pass is the checkerboard's.  A stream is `stream_positions` consecutive compact slots
of one (image, group, pass), the group's channels innermost; the last stream of a pass takes what is left, so a pass of
N_p positions has S_p = ceil(N_p / stream_positions) streams.  Each stream holds what
`LocationScaleIndexedEntropyModel(..., coding_rank=2).compress(y - mu, index)` writes for that [positions, M_g] block.
An image has T = G (S_0 + S_1) strings in the order group, pass, stream.  `stream_positions` belongs to the
configuration, like `num_scales`, and is not written anywhere.

`scctx_scan` is the encoder side and the evaluation (2 G launches), `scctx_encode` writes the strings of a scan,
`scctx_decode` is the decoder side (per step: parameters, one or two `decompress` calls, place);
`scctx_scan_reference` and `scctx_parameters_reference` are the definition as tensor ops for any float dtype and for CPU
tensors, and the fallback off the device."""
from __future__ import annotations

import collections

import numpy as np
import torch

from .. import _lib
from .checkerboard_ops import (CHECKER_TAPS, CHECKERBOARD_CONSTANTS, CheckerboardParams, anchor_mask, checkerboard_place,
                               checkerboard_split, pass_positions, stream_merge, stream_split, _check_pass,
                               _check_stream_positions, _decode_steps, _encode_steps, _launch_params, _on_kernel,
                               _scan_steps)
from .context_ops import CONTEXT_CONSTANTS, _check_inputs, _index_prepare, _layout, _network, _pad, tap_sum

__all__ = ["ALL_TAPS", "SCCTX_CONSTANTS", "SpaceChannelParams", "SpaceChannelScan", "default_groups", "hidden_widths",
           "scctx_decode", "scctx_encode", "scctx_parameters", "scctx_parameters_reference", "scctx_place", "scctx_scan",
           "scctx_scan_reference", "stream_counts", "stream_merge", "stream_split"]

SpaceChannelScan = collections.namedtuple("SpaceChannelScan", ["sym", "idx", "mu", "y_hat", "index_float"])

# (di, dj) of the taps over the earlier groups in the kernels' order: the whole 5x5 window, row-major
ALL_TAPS = tuple((di, dj) for di in range(-2, 3) for dj in range(-2, 3))

# the named constants of csrc/space_channel_params.h
SCCTX_CONSTANTS = _lib.kernel_constants("space_channel_params.h", ("SCCTX",))
assert SCCTX_CONSTANTS["SCCTX_TAPS"] == len(ALL_TAPS)


def default_groups(m):
    """The group widths of a latent of depth `m`: 16, 16, 32, 64 and then the rest, stopping when `m` is used up;
    (16, 16, 32, 64, 64) for 192."""
    m = int(m)
    if m < 1:
        raise ValueError(f"the latent depth must be positive, got {m}")
    groups, left = [], m
    for width in (16, 16, 32, 64):
        if left == 0:
            break
        groups.append(min(width, left))
        left -= groups[-1]
    if left:
        groups.append(left)
    return tuple(groups)


def hidden_widths(m_g, p):
    """(H1, H2) of a group's entropy-parameter network: with in = 2 M_g + P and out = 2 M_g, out + 2 (in - out) // 3 and
    out + (in - out) // 3; mbt2018's 10 M // 3 and 8 M // 3 for a single group with P = 2 M."""
    out = 2 * int(m_g)
    return out + 2 * int(p) // 3, out + int(p) // 3


def _check_groups(groups, m=None):
    groups = tuple(int(v) for v in groups)
    if not groups or min(groups) < 1:
        raise ValueError(f"groups must be a non-empty sequence of positive widths, got {groups!r}")
    if m is not None and sum(groups) != int(m):
        raise ValueError(f"the group widths {groups!r} sum to {sum(groups)}, the latent depth is {int(m)}")
    return groups


class SpaceChannelParams:
    """The weights of the space-channel context model, checked and packed once per group.

    `groups`: one tuple per group g, (kernel_ch [5, 5, c_g, 2 M_g] or None for g = 0, kernel_sp [5, 5, M_g, 2 M_g],
    kernel_bias [2 M_g], w1 [2 M_g + P, H1], b1, w2 [H1, H2], b2, w3 [H2, 2 M_g], b3): HWIO kernels, rows are inputs.
    The checkerboard mask is applied to kernel_sp here, whatever its other taps hold; kernel_ch is used in full.  Any
    widths are taken; `hidden_widths` is the model's rule, not a check.  Holds detached copies."""

    TAPS = ALL_TAPS         # over the earlier groups; CHECKER_TAPS over the own group (`own`)

    def __init__(self, groups, num_scales, stream_positions=SCCTX_CONSTANTS["SCCTX_STREAM"]):
        groups = list(groups)
        if not groups:
            raise ValueError("groups must hold at least one group")
        self.num_scales = int(num_scales)
        self.stream_positions = _check_stream_positions(stream_positions)
        self.own, self.kernel_ch, self.offsets = [], [], []
        at = 0
        for g, group in enumerate(groups):
            if len(group) != 9:
                raise ValueError(f"group {g} must be (kernel_ch, kernel_sp, kernel_bias, w1, b1, w2, b2, w3, b3), received "
                                 f"{len(group)} entries")
            own = CheckerboardParams(*group[1:], num_scales)        # the checks and the layout of one group
            if g and own.p != self.own[0].p:
                raise ValueError(f"group {g} has P = {own.p}, group 0 has P = {self.own[0].p}")
            kernel_ch = group[0]
            if at == 0:
                if kernel_ch is not None and torch.as_tensor(kernel_ch).numel():
                    raise ValueError("group 0 has no earlier groups: its kernel_ch must be None")
                kernel_ch = torch.zeros(5, 5, 0, 2 * own.m, dtype=own.kernel.dtype)
            else:
                kernel_ch = torch.as_tensor(kernel_ch).detach()
                if tuple(kernel_ch.shape) != (5, 5, at, 2 * own.m):
                    raise ValueError(f"kernel_ch of group {g} must be [5, 5, {at}, {2 * own.m}], received shape "
                                     f"{tuple(kernel_ch.shape)}")
                if not kernel_ch.dtype.is_floating_point:
                    raise TypeError("the weights must be floating point")
            self.own.append(own)
            self.kernel_ch.append(kernel_ch)
            self.offsets.append(at)
            at += own.m
        self.m, self.p = at, self.own[0].p
        self.groups = tuple(own.m for own in self.own)
        if self.m > CONTEXT_CONSTANTS["CTX_MAX_DIM"]:
            raise ValueError(f"M must be at most {CONTEXT_CONSTANTS['CTX_MAX_DIM']}")
        self._cache = {}

    @classmethod
    def from_layers(cls, channel_convs, space_convs, networks, num_scales, stream_positions):
        """From, per group, the plain 5x5 `SignalConv2D` over the earlier groups (None for group 0), the
        `CheckerboardConv2D` over the own group (it carries the bias) and the three 1x1 layers of the network."""
        groups = []
        for ch, sp, layers in zip(channel_convs, space_convs, networks):
            w = [layer.kernel.reshape(layer.kernel.shape[-2], layer.kernel.shape[-1]) for layer in layers]
            b = [layer._bias_value() for layer in layers]
            groups.append((None if ch is None else ch.kernel, sp.kernel, sp._bias_value(), w[0], b[0], w[1], b[1], w[2],
                           b[2]))
        return cls(groups, num_scales, stream_positions)

    def __len__(self):
        return len(self.own)

    def tensors(self, g, dtype, device):
        """(kernel_ch, kernel_sp masked, kernel_bias, w1, b1, w2, b2, w3, b3) of group g in `dtype` on `device`."""
        key = ("tensors", g, dtype, str(device))
        if key not in self._cache:
            self._cache[key] = (self.kernel_ch[g].to(device=device, dtype=dtype),) + self.own[g].tensors(dtype, device)
        return self._cache[key]

    def fits_kernel(self):
        """Whether every group's activations of one tile of positions fit the kernel's LDS with its own widths:
        (max(2 M_g, H2_g) + max(H1_g, 2 M_g) + CKB_STAGE_K) * CKB_TILE <= CKB_LDS_FLOATS (padded to CTX_KPAD)."""
        return all(own.fits_kernel() for own in self.own)

    def packed_floats(self, g):
        """Floats of group g's buffer (scctx_layout of csrc/space_channel_params.h)."""
        own = self.own[g]
        return _layout(own.m, own.p, own.h1, own.h2)[1] + _pad(len(ALL_TAPS) * _pad(self.offsets[g]) * 2 * own.m)

    def packed(self, g, device):
        """Group g's float32 buffer (layout: csrc/space_channel_params.h): the checkerboard model's buffer of the group,
        then wch [25][c_g padded][2 M_g]."""
        key = ("packed", g, str(device))
        if key not in self._cache:
            own, c = self.own[g], self.offsets[g]
            head = own.packed("cpu")
            wch = torch.zeros(len(ALL_TAPS), _pad(c), 2 * own.m)
            kernel = self.kernel_ch[g].to(torch.float32)
            for k, (di, dj) in enumerate(ALL_TAPS):
                wch[k, :c] = kernel[di + 2, dj + 2]
            tail = torch.zeros(self.packed_floats(g) - head.numel())
            tail[:wch.numel()] = wch.reshape(-1)
            self._cache[key] = torch.cat([head, tail]).to(device)
        return self._cache[key]


# ---- streams --------------------------------------------------------------------------------------------------------

def stream_counts(hl, wl, stream_positions):
    """(S_0, S_1): the streams of a pass, ceil(N_p / stream_positions); a pass without positions has none."""
    sp = _check_stream_positions(stream_positions)
    return tuple(-(-pass_positions(hl, wl, p) // sp) for p in (0, 1))


# ---- the definition as tensor ops ---------------------------------------------------------------------------------------

def _check(y, psi, params, what="y"):
    _check_inputs(y, psi, params, what, kind=SpaceChannelParams)


def _check_group(g, params):
    if g not in range(len(params)):
        raise ValueError(f"g must be in [0, {len(params)}), got {g!r}")
    return int(g)


def _group_reference(y_hat, psi, params, g):
    """(mu, index_float) of group g for every position, [B, Hl, Wl, M_g], teacher-forced on `y_hat`: two tap sums."""
    w = params.tensors(g, y_hat.dtype, y_hat.device)
    c, mg = params.offsets[g], params.groups[g]
    b, hl, wl, _ = y_hat.shape
    ctx = w[2].expand(b, hl, wl, 2 * mg)
    if c:
        ctx = tap_sum(ctx, y_hat[..., :c], w[0], ALL_TAPS)
    own = tap_sum(torch.zeros(b, hl, wl, 2 * mg, dtype=y_hat.dtype, device=y_hat.device), y_hat[..., c:c + mg], w[1],
                  CHECKER_TAPS)
    others = (~anchor_mask(hl, wl, y_hat.device)).to(y_hat.dtype)[None, :, :, None]
    out = _network(ctx + own * others, psi, w[1:])
    return out[..., :mg], out[..., mg:]


def scctx_parameters_reference(y_hat, psi, params):
    """The parallel (teacher-forced) definition -> (mu, index_float), each [B, Hl, Wl, M] in the full layout."""
    _check(y_hat, psi, params, "y_hat")
    parts = [_group_reference(y_hat, psi, params, g) for g in range(len(params))]
    return torch.cat([p[0] for p in parts], dim=-1), torch.cat([p[1] for p in parts], dim=-1)


def scctx_scan_reference(y, psi, params):
    """The definition, step after step -> SpaceChannelScan(sym int32, idx int32, mu, y_hat, index_float) in the full
    layout.  Any float dtype, any device."""
    _check(y, psi, params)
    b, hl, wl, m = y.shape
    anchors = anchor_mask(hl, wl, y.device)[None, :, :, None]
    y_hat = torch.zeros_like(y)
    mus, indexes = [], []
    for g in range(len(params)):
        c, mg = params.offsets[g], params.groups[g]
        y_g = y[..., c:c + mg]
        mu0, _ = _group_reference(y_hat, psi, params, g)
        y_hat[..., c:c + mg] = torch.where(anchors, torch.round(y_g - mu0) + mu0, torch.zeros_like(y_g))
        mu, index_float = _group_reference(y_hat, psi, params, g)
        y_hat[..., c:c + mg] = torch.round(y_g - mu) + mu
        mus.append(mu)
        indexes.append(index_float)
    mu, index_float = torch.cat(mus, dim=-1), torch.cat(indexes, dim=-1)
    return SpaceChannelScan(torch.round(y - mu).to(torch.int32), _index_prepare(index_float, params.num_scales), mu,
                            y_hat, index_float)


# ---- the kernels: the launch sites and the loops are checkerboard_ops', which runs as the one-group case ---------------

def _steps(params, device, gs=None):
    """The step list of the groups `gs` (all of them when None), each checked against the kernel's LDS."""
    steps = []
    for g in range(len(params)) if gs is None else gs:
        own, c = params.own[g], CHECKERBOARD_CONSTANTS
        if not own.fits_kernel():
            raise ValueError(f"group {g} (M_g {own.m}, P {own.p}, H1 {own.h1}, H2 {own.h2}) does not fit the kernel: the "
                             f"activations of one tile of {c['CKB_TILE']} positions need more than "
                             f"{4 * c['CKB_LDS_FLOATS']} bytes of LDS")
        steps.append((own, params.packed(g, device), params.offsets[g]))
    return steps


def scctx_parameters(y_hat, psi, params, g, pass_):
    """(mu, index_float) of step (g, pass_) in compact order, [B, N_pass, M_g], given `y_hat` [B, Hl, Wl, M] (read at the
    channels of the earlier groups everywhere and, by pass 1, at the group's own channels at anchors).  float32 device
    tensors run tfc_scctx_params; CPU tensors and other float dtypes take the reference."""
    _check(y_hat, psi, params, "y_hat")
    g, pass_ = _check_group(g, params), _check_pass(pass_)
    if not _on_kernel(y_hat):
        mu, index_float = _group_reference(y_hat, psi, params, g)
        return checkerboard_split(mu)[pass_], checkerboard_split(index_float)[pass_]
    ((own, packed, c_g),) = _steps(params, psi.device, [g])
    return _launch_params(pass_, None, y_hat.detach().contiguous(), psi.detach().contiguous(), own, packed, c_g)[:2]


def scctx_place(sym, mu, y_hat, c_g, pass_):
    """y_hat[positions of the pass, c_g : c_g + M_g] = float32(sym) + mu, in place, from compact `sym` and `mu`
    [B, N_pass, M_g]."""
    return checkerboard_place(sym, mu, y_hat, pass_, c_g)


def scctx_scan(y, psi, params):
    """y [B, Hl, Wl, M], psi [B, Hl, Wl, P] -> SpaceChannelScan(sym int32, idx int32, mu, y_hat, index_float) in the full
    layout: float32 device tensors run tfc_scctx_params 2 G times; CPU tensors and other float dtypes take
    `scctx_scan_reference`."""
    _check(y, psi, params)
    if not _on_kernel(y):
        return scctx_scan_reference(y, psi, params)
    y, psi = y.detach().contiguous(), psi.detach().contiguous()
    return SpaceChannelScan(*_scan_steps(y, psi, _steps(params, psi.device)))


def scctx_encode(y, scan, params, entropy_model):
    """The strings of a scan, object array [B, T] with T = G (S_0 + S_1) in the order group, pass, stream: per step the
    full streams go through one `compress` call as [B, S_full, stream_positions, M_g], a shorter last stream through a
    second."""
    if not isinstance(params, SpaceChannelParams):
        raise TypeError("params must be a SpaceChannelParams")
    if y.dim() != 4 or y.shape[-1] != params.m or tuple(scan.mu.shape) != tuple(y.shape):
        raise ValueError(f"y and the scan must be [B, Hl, Wl, {params.m}], received shapes {tuple(y.shape)} and "
                         f"{tuple(scan.mu.shape)}")
    return _encode_steps(y - scan.mu, scan.index_float, zip(params.offsets, params.groups), params.stream_positions,
                         entropy_model)


def scctx_decode(strings, psi, params, entropy_model):
    """The strings [B, T] of `scctx_encode`, psi [B, Hl, Wl, P] float32 on the device and the
    `LocationScaleIndexedEntropyModel` (coding_rank 2) that wrote them -> y_hat [B, Hl, Wl, M].  Per step: the
    parameters (one launch), one `decompress` call for the full streams and one for a shorter last stream, the store."""
    _check(None, psi, params)
    if not _on_kernel(psi):
        raise ValueError("scctx_decode needs float32 psi on the device")
    psi = psi.detach().contiguous()
    b, hl, wl, _ = psi.shape
    counts = stream_counts(hl, wl, params.stream_positions)
    per_image = len(params) * sum(counts)
    strings = np.asarray(strings, dtype=object)
    if strings.shape != (b, per_image):
        raise ValueError(f"strings must have shape [{b}, {per_image}] ({len(params)} groups x ({counts[0]} + {counts[1]}) "
                         f"streams of {params.stream_positions} positions for every image), received "
                         f"{list(strings.shape)}")
    return _decode_steps(strings, psi, _steps(params, psi.device), params.m, params.stream_positions, entropy_model)


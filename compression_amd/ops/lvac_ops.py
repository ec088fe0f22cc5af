"""The two operations an LVAC training step spends its time in (models/lvac/lvac.ipynb, `Model.synthesize` and
`Model.reconstruct_at_level` / `evaluate_reconstruction_at_level`).

Inverse RAHT.  Level b of the binary tree turns parent rows into child rows; with the level's AC rows `ac`:

    child[c, :] = parent[p(c), :] + w(c) ac[k(c), :]     w = latent_coeff (left child), 1 (right child), no term (only child)

`RahtTree` holds the tables of every level on the device (checked once, on the host); `raht_synthesize` runs
tfc_raht_forward / tfc_raht_backward (csrc/lvac.hip), `raht_synthesize_reference` is the notebook's composition
(repeat + index_add) as tensor ops, which CPU tensors take.

The point decoder.  For every point n of block index[n]:

    recon[n] = A (W2^T relu(W1^T [position[n]; z[index[n]]] + b1) + b2) + o      (clipped to [0, 255] on request)
    loss     = sum_n |recon[n] - target[n]|^2 / (3 N)

`point_mlp_loss` runs tfc_point_mlp_forward / tfc_point_mlp_backward: no [N, H] tensor exists, in either direction.
`point_mlp_loss_reference` is the same definition as tensor ops; CPU tensors and shapes outside `LVAC_CONSTANTS`'
PM_MIN_C..PM_MAX_C, PM_MIN_H..PM_MAX_H take it."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import ptr as _ptr

__all__ = ["RahtTree", "PointBlocks", "raht_synthesize", "raht_synthesize_reference", "point_mlp_loss",
           "point_mlp_loss_reference", "point_mlp_eligible", "LVAC_CONSTANTS", "RGB_TO_YUV", "YUV_TO_RGB", "IDENTITY"]


# the named constants of csrc/lvac_params.h (tile sizes, the eligibility range)
LVAC_CONSTANTS = _lib.kernel_constants("lvac_params.h", ("RAHT", "PM"))

# The output maps as (A row-major, o): recon = A y + o.  The notebook's coefficients (not those of rgb_to_ycbcr).
IDENTITY = ((1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0))
RGB_TO_YUV = ((0.212600, 0.715200, 0.072200, -0.114572, -0.385428, 0.5, 0.5, -0.454153, -0.045847),
              (0.0, 128.0, 128.0))
# r = y + 1.57480 (v - 128) and so on: the offsets are the matrix applied to (0, -128, -128)
YUV_TO_RGB = ((1.0, 0.0, 1.57480, 1.0, -0.18733, -0.46813, 1.0, 1.85563, 0.0),
              (-128.0 * 1.57480, 128.0 * (0.18733 + 0.46813), -128.0 * 1.85563))


# ------------------------------------------------------------------------------------------------------------------
# inverse RAHT
# ------------------------------------------------------------------------------------------------------------------

class RahtTree:
    """The device tables of a binary tree, built once per cloud.

    `levels` is a sequence with one entry per level, top first, each a mapping (or an object with attributes)
    holding `child_count` (int [parents], every entry 1 or 2) and `latent_coeff` (float [two-child parents] or
    [.., 1]): what `build_octree_as_binarytree` leaves in binlevel[0 .. target_level - 1].  Children of a node are
    adjacent and in order, so the tables follow from these two alone.  Everything is checked here, on the host; a
    violation is a ValueError that names it."""

    def __init__(self, levels, n_root=1, device=None):
        self.n_root = int(n_root)
        self.device = torch.device(device) if device is not None else None
        self.levels = []
        rows = self.n_root
        for b, level in enumerate(levels):
            get = level.get if isinstance(level, dict) else lambda k, _l=level: getattr(_l, k)
            count = np.asarray(get("child_count")).astype(np.int64).ravel()
            coeff = np.asarray(get("latent_coeff"), dtype=np.float32).ravel()
            if count.shape[0] != rows:
                raise ValueError(f"RahtTree: level {b} has {count.shape[0]} child counts for {rows} parent rows")
            if count.size and not np.all((count == 1) | (count == 2)):
                raise ValueError(f"RahtTree: child_count of level {b} must be 1 or 2 everywhere")
            two = np.flatnonzero(count == 2)
            if coeff.shape[0] != two.shape[0]:
                raise ValueError(f"RahtTree: level {b} has {coeff.shape[0]} coefficients for {two.shape[0]} "
                                 "two-child nodes")
            if not np.all(np.isfinite(coeff)):
                raise ValueError(f"RahtTree: latent_coeff of level {b} must be finite")
            n_child = int(count.sum())
            if n_child >= 2 ** 31:
                raise ValueError(f"RahtTree: level {b} has {n_child} children, the tables are int32")
            first = np.cumsum(count) - count
            parent = np.repeat(np.arange(rows, dtype=np.int64), count)
            child_ac = np.full(n_child, -1, np.int64)
            weight = np.zeros(n_child, np.float32)
            left = first[two]
            child_ac[left] = np.arange(two.shape[0])
            child_ac[left + 1] = np.arange(two.shape[0])
            weight[left] = coeff
            weight[left + 1] = 1.0
            self.levels.append({
                "n_child": n_child, "n_parent": rows, "n_ac": int(two.shape[0]),
                "child_parent": parent.astype(np.int32), "child_ac": child_ac.astype(np.int32), "child_weight": weight,
                "parent_first": first.astype(np.int32), "parent_count": count.astype(np.int32),
                "ac_left": left.astype(np.int32), "ac_coeff": coeff})
            rows = n_child
        self.n_out = rows
        if len(self.levels) > LVAC_CONSTANTS["RAHT_MAX_LEVELS"]:
            raise ValueError(f"RahtTree: at most {LVAC_CONSTANTS['RAHT_MAX_LEVELS']} levels, got {len(self.levels)}")
        self._device_tables = {}

    TABLES = ("child_parent", "child_ac", "child_weight", "parent_first", "parent_count", "ac_left", "ac_coeff")

    @property
    def ac_rows(self):
        return [lv["n_ac"] for lv in self.levels]

    def tensors(self, device):
        """Per level, the index tensors of the tensor-op twin on `device`."""
        key = ("twin", str(device))
        if key not in self._device_tables:
            out = []
            for lv in self.levels:
                out.append({
                    "child_parent": torch.from_numpy(lv["child_parent"].astype(np.int64)).to(device),
                    "child_ac": torch.from_numpy(np.maximum(lv["child_ac"], 0).astype(np.int64)).to(device),
                    "child_weight": torch.from_numpy(lv["child_weight"]).to(device)})
            self._device_tables[key] = out
        return self._device_tables[key]

    def packed(self, device):
        """(desc host int64 [levels, 10], desc on the device, tables on the device, words) for the C entries."""
        key = ("packed", str(device))
        if key not in self._device_tables:
            desc = np.zeros((max(len(self.levels), 1), LVAC_CONSTANTS["RAHT_DESC"]), np.int64)
            parts, at = [], 0
            for b, lv in enumerate(self.levels):
                desc[b, :3] = (lv["n_child"], lv["n_parent"], lv["n_ac"])
                for j, name in enumerate(self.TABLES):
                    desc[b, 3 + j] = at
                    parts.append(lv[name].view(np.int32))
                    at += lv[name].shape[0]
            words = np.concatenate(parts) if parts else np.zeros(0, np.int32)
            words = np.concatenate([words, np.zeros(1, np.int32)])          # never an empty allocation
            self._device_tables[key] = (desc, torch.from_numpy(desc).to(device), torch.from_numpy(words).to(device), at)
        return self._device_tables[key]


def _check_raht(dc, ac_list, tree):
    if not isinstance(tree, RahtTree):
        raise TypeError("tree must be a RahtTree")
    if dc.dim() != 2 or dc.shape[0] != tree.n_root:
        raise ValueError(f"dc must be [{tree.n_root}, C], received shape {tuple(dc.shape)}")
    if len(ac_list) != len(tree.levels):
        raise ValueError(f"the tree has {len(tree.levels)} levels, got {len(ac_list)} AC tensors")
    for b, (ac, lv) in enumerate(zip(ac_list, tree.levels)):
        if ac.dim() != 2 or tuple(ac.shape) != (lv["n_ac"], dc.shape[1]):
            raise ValueError(f"ac[{b}] must be [{lv['n_ac']}, {dc.shape[1]}], received shape {tuple(ac.shape)}")
        if ac.dtype != dc.dtype or ac.device != dc.device:
            raise ValueError(f"ac[{b}] must share dc's dtype and device")


def raht_synthesize_reference(dc, ac_list, tree):
    """The notebook's composition as differentiable tensor ops: per level with AC rows, gather the parents and add the
    weighted AC rows.  dc [n_root, C], ac_list[b] [AC rows of level b, C] -> [n_out, C]."""
    _check_raht(dc, ac_list, tree)
    cur = dc
    for ac, lv, t in zip(ac_list, tree.levels, tree.tensors(dc.device)):
        if lv["n_ac"] == 0:
            continue                                     # every node has one child: the identity
        w = t["child_weight"].to(dc.dtype)[:, None]
        cur = cur[t["child_parent"]] + w * ac[t["child_ac"]]
    return cur


class _RahtFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tree, dc, *ac_list):
        dc = dc.contiguous()
        ac_list = [a.contiguous() for a in ac_list]
        desc, desc_dev, tables, words = tree.packed(dc.device)
        levels, c = len(tree.levels), dc.shape[1]
        out = torch.empty(tree.n_out, c, dtype=torch.float32, device=dc.device)
        ptrs = (C.c_void_p * max(levels, 1))(*[a.data_ptr() if a.numel() else None for a in ac_list])
        _lib.check(_lib.lib().tfc_raht_forward(
            dc.data_ptr(), tree.n_root, ptrs, desc.ctypes.data_as(C.POINTER(C.c_int64)), desc_dev.data_ptr(),
            tables.data_ptr(), words, levels, c, out.data_ptr(), tree.n_out, _lib.stream_ptr()))
        ctx.tree = tree
        ctx.channels = c
        return out

    @staticmethod
    def backward(ctx, g):
        tree, c = ctx.tree, ctx.channels
        g = g.to(torch.float32).contiguous()
        desc, desc_dev, tables, words = tree.packed(g.device)
        levels = len(tree.levels)
        d_dc = torch.empty(tree.n_root, c, dtype=torch.float32, device=g.device)
        d_ac = [torch.empty(lv["n_ac"], c, dtype=torch.float32, device=g.device) for lv in tree.levels]
        ptrs = (C.c_void_p * max(levels, 1))(*[a.data_ptr() if a.numel() else None for a in d_ac])
        _lib.check(_lib.lib().tfc_raht_backward(
            g.data_ptr(), tree.n_out, ptrs, desc.ctypes.data_as(C.POINTER(C.c_int64)), desc_dev.data_ptr(),
            tables.data_ptr(), words, levels, c, d_dc.data_ptr(), tree.n_root, _lib.stream_ptr()))
        return (None, d_dc) + tuple(d_ac)


def raht_synthesize(dc, ac_list, tree):
    """dc [n_root, C], ac_list[b] [AC rows of level b, C], float32 -> the leaves' rows [n_out, C] on the HIP kernels,
    differentiable in dc and every AC tensor, bit-identical from call to call.  CPU tensors (and float64) take
    `raht_synthesize_reference`."""
    ac_list = list(ac_list)
    if not dc.is_cuda or dc.dtype != torch.float32:
        return raht_synthesize_reference(dc, ac_list, tree)
    _check_raht(dc, ac_list, tree)
    return _RahtFunction.apply(tree, dc, *ac_list)


# ------------------------------------------------------------------------------------------------------------------
# the point decoder
# ------------------------------------------------------------------------------------------------------------------

class PointBlocks:
    """The point -> block index of a cloud, checked once: `index` int32 [N], non-decreasing, inside [0, n_blocks).
    Holds the index and the blocks' offsets ([n_blocks + 1] int64) on the device it is asked for."""

    def __init__(self, index, n_blocks):
        idx = index.detach().cpu().numpy() if isinstance(index, torch.Tensor) else np.asarray(index)
        if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError("index must be a vector of integers")
        self.n_blocks = int(n_blocks)
        self.n = int(idx.shape[0])
        if self.n and (idx.min() < 0 or idx.max() >= self.n_blocks):
            raise ValueError(f"index must lie in [0, {self.n_blocks}), got [{idx.min()}, {idx.max()}]")
        if self.n > 1 and np.any(np.diff(idx.astype(np.int64)) < 0):
            raise ValueError("index must be non-decreasing (the points of a block are contiguous)")
        self._index = idx.astype(np.int32)
        self._offset = np.searchsorted(idx, np.arange(self.n_blocks + 1), side="left").astype(np.int64)
        self._on = {}

    @classmethod
    def from_counts(cls, counts):
        counts = np.asarray(counts).astype(np.int64).ravel()
        return cls(np.repeat(np.arange(counts.shape[0], dtype=np.int32), counts), counts.shape[0])

    def on(self, device):
        key = str(device)
        if key not in self._on:
            self._on[key] = (torch.from_numpy(self._index).to(device), torch.from_numpy(self._offset).to(device))
        return self._on[key]


def point_mlp_eligible(channels, hidden):
    k = LVAC_CONSTANTS
    return k["PM_MIN_C"] <= channels <= k["PM_MAX_C"] and k["PM_MIN_H"] <= hidden <= k["PM_MAX_H"]


def _check_point_args(z, blocks, position, w1, b1, w2, b2, target, affine):
    if z.dim() != 2 or z.shape[0] != blocks.n_blocks:
        raise ValueError(f"z must be [{blocks.n_blocks}, C], received shape {tuple(z.shape)}")
    c, n = z.shape[1], blocks.n
    rows = c + (3 if position is not None else 0)
    if position is not None and tuple(position.shape) != (n, 3):
        raise ValueError(f"position must be [{n}, 3], received shape {tuple(position.shape)}")
    if w1.dim() != 2 or w1.shape[0] != rows:
        raise ValueError(f"w1 must be [{rows}, H], received shape {tuple(w1.shape)}")
    h = w1.shape[1]
    if tuple(b1.shape) != (h,) or tuple(w2.shape) != (h, 3) or tuple(b2.shape) != (3,):
        raise ValueError(f"b1, w2, b2 must be [{h}], [{h}, 3], [3], received {tuple(b1.shape)}, {tuple(w2.shape)}, "
                         f"{tuple(b2.shape)}")
    if tuple(target.shape) != (n, 3):
        raise ValueError(f"target must be [{n}, 3], received shape {tuple(target.shape)}")
    a, o = affine
    if len(a) != 9 or len(o) != 3:
        raise ValueError("affine must be (9 matrix entries row-major, 3 offsets)")
    return n, c, h


def _as_blocks(index, n_blocks):
    return index if isinstance(index, PointBlocks) else PointBlocks(index, n_blocks)


def point_mlp_loss_reference(z, index, position, w1, b1, w2, b2, target, affine=IDENTITY, clip=False):
    """The definition as differentiable tensor ops -> (loss, recon [N, 3]).  `index` is a PointBlocks or an integer
    vector.  This one does hold the [N, H] activations."""
    blocks = _as_blocks(index, z.shape[0])
    n, _, _ = _check_point_args(z, blocks, position, w1, b1, w2, b2, target, affine)
    idx = blocks.on(z.device)[0].to(torch.int64)
    x = z[idx]
    if position is not None:
        x = torch.cat([position.to(z.dtype), x], dim=-1)
    y = torch.relu(x @ w1 + b1) @ w2 + b2
    a = torch.tensor(affine[0], dtype=z.dtype, device=z.device).reshape(3, 3)
    o = torch.tensor(affine[1], dtype=z.dtype, device=z.device)
    recon = y @ a.T + o
    if clip:
        recon = recon.clamp(0.0, 255.0)
    if n == 0:
        return recon.sum() * 0.0, recon
    return torch.square(recon - target).sum() / (3 * n), recon


class _PointMlpFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blocks, affine, clip, want_recon, z, position, w1, b1, w2, b2, target):
        z, w1, b1, w2, b2, target = (t.contiguous() for t in (z, w1, b1, w2, b2, target))
        position = position.contiguous() if position is not None else None
        index, offset = blocks.on(z.device)
        n, c, h = blocks.n, z.shape[1], w1.shape[1]
        need_grad = any(ctx.needs_input_grad)
        recon = torch.empty(n, 3, dtype=torch.float32, device=z.device) if want_recon else None
        gerr = torch.empty(n, 3, dtype=torch.float32, device=z.device) if need_grad else None
        sse = torch.empty(1, dtype=torch.float32, device=z.device)
        aff = (C.c_float * 12)(*affine[0], *affine[1])
        _lib.check(_lib.lib().tfc_point_mlp_forward(
            z.data_ptr(), index.data_ptr(), _ptr(position), w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(),
            aff, target.data_ptr(), n, blocks.n_blocks, c, h, int(bool(clip)), _ptr(recon), _ptr(gerr), sse.data_ptr(),
            _lib.stream_ptr()))
        ctx.save_for_backward(z, position, w1, b1, w2, b2, gerr)
        ctx.blocks, ctx.affine = blocks, affine
        if recon is None:
            recon = torch.empty(0, 3, dtype=torch.float32, device=z.device)
        ctx.mark_non_differentiable(recon)
        return sse.reshape(()), recon

    @staticmethod
    def backward(ctx, g_sse, _g_recon):
        z, position, w1, b1, w2, b2, gerr = ctx.saved_tensors
        blocks = ctx.blocks
        index, offset = blocks.on(z.device)
        n, c, h = blocks.n, z.shape[1], w1.shape[1]
        need_z = ctx.needs_input_grad[4]
        need_p = any(ctx.needs_input_grad[6:10])
        rows = w1.shape[0]
        d_params = torch.empty(rows * h + h + 3 * h + 3, dtype=torch.float32, device=z.device) if need_p else None
        d_z = torch.empty_like(z) if need_z else None
        g = g_sse.to(torch.float32).reshape(1).contiguous()
        aff = (C.c_float * 12)(*ctx.affine[0], *ctx.affine[1])
        if need_z or need_p:
            _lib.check(_lib.lib().tfc_point_mlp_backward(
                z.data_ptr(), index.data_ptr(), offset.data_ptr(), _ptr(position), w1.data_ptr(), b1.data_ptr(),
                w2.data_ptr(), b2.data_ptr(), aff, gerr.data_ptr(), g.data_ptr(), n, blocks.n_blocks, c, h,
                _ptr(d_params), _ptr(d_z), _lib.stream_ptr()))
        d_w1 = d_b1 = d_w2 = d_b2 = None
        if need_p:
            a, b = rows * h, rows * h + h
            d_w1, d_b1 = d_params[:a].view(rows, h), d_params[a:b]
            d_w2, d_b2 = d_params[b:b + 3 * h].view(h, 3), d_params[b + 3 * h:]
        return None, None, None, None, d_z, None, d_w1, d_b1, d_w2, d_b2, None


def point_mlp_loss(z, index, position, w1, b1, w2, b2, target, affine=IDENTITY, clip=False, want_recon=False):
    """z [n_blocks, C], index (a PointBlocks, or an int32 vector [N] that is checked on every call), position [N, 3] or
    None, w1 [C + 3 or C, H], b1 [H], w2 [H, 3], b2 [3], target [N, 3], float32 -> (loss, recon [N, 3] or None): the
    mean squared error of the decoded colours on the HIP kernels, differentiable in z and the four parameters.
    Ineligible shapes and CPU tensors take `point_mlp_loss_reference`."""
    blocks = _as_blocks(index, z.shape[0])
    n, c, h = _check_point_args(z, blocks, position, w1, b1, w2, b2, target, affine)
    tensors = [t for t in (z, position, w1, b1, w2, b2, target) if t is not None]
    fused = (z.is_cuda and point_mlp_eligible(c, h) and all(t.dtype == torch.float32 for t in tensors))
    if not fused:
        loss, recon = point_mlp_loss_reference(z, blocks, position, w1, b1, w2, b2, target, affine, clip)
        return loss, (recon.detach() if want_recon else None)
    if any(t.device != z.device for t in tensors):
        raise ValueError("every tensor must be on z's device")
    affine = (tuple(float(v) for v in affine[0]), tuple(float(v) for v in affine[1]))
    sse, recon = _PointMlpFunction.apply(blocks, affine, bool(clip), bool(want_recon), z, position, w1, b1, w2, b2,
                                         target)
    loss = sse / (3 * n) if n else sse
    return loss, (recon if want_recon else None)

"""The streaming ops of the training loop (csrc/train.hip, csrc/scale_crop.hip): the random crops of the input
pipeline, with and without HiFiC's random resize, and the Keras Adam step.

    crop_patches         B patches [P, P, 3] out of a flat pool of decoded images -> [B, P, P, 3]   (models/bls2017.py:198-200)
    scale_crop_patches   the same out of the bilinearly RESIZED images, which never exist      (models/hific/model.py:316-351)
    keras_adam           one step of tf.keras.optimizers.Adam over a list of float32 tensors, in place

Each runs one kernel (tfc_crop_patches, tfc_scale_crop_patches, tfc_keras_adam; one per KERAS_ADAM_CAPACITY tensors) on
device tensors and has a `*_reference` twin of plain tensor ops, which CPU tensors take.  include/tfc_hip.h states the
definitions in full; tests/train_ref.py and tests/scale_crop_ref.py hold the numpy / float64 forms.  The Adam rule, every
operation rounded to float32 on its own:

    m' = m + (g - m) * c1                      c1 = float32(1 - beta_1)
    v' = v + (g * g - v) * c2                  c2 = float32(1 - beta_2)
    p' = p - (m' * alpha) / (sqrt(v') + eps)   alpha = float32(lr sqrt(1 - beta_2^t) / (1 - beta_1^t)), eps = float32(epsilon)

with t counting from 1.  The kernel is bit-identical to the twin."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from .. import _lib
from .video_ops import DTYPE_CODE

__all__ = ["crop_patches", "crop_patches_reference", "scale_crop_patches", "scale_crop_patches_reference",
           "keras_adam", "keras_adam_reference", "keras_adam_constants",
           "KERAS_ADAM_CAPACITY", "KERAS_ADAM_CHUNK"]

KERAS_ADAM_CAPACITY = 64       # tensors per launch (TFC_KERAS_ADAM_CAPACITY)
KERAS_ADAM_CHUNK = 4096        # elements of one tensor per workgroup (TFC_KERAS_ADAM_CHUNK)


# -------------------------------------------------------------------------------------------------------------------
# crops


def _check_crop(pool, table, patchsize, dtype):
    if pool.dtype != torch.uint8:
        raise TypeError(f"pool must be uint8, got {pool.dtype}")
    if pool.dim() != 1 or not pool.is_contiguous():
        raise ValueError(f"pool must be a flat contiguous tensor, received shape {tuple(pool.shape)}")
    if dtype not in DTYPE_CODE:
        raise TypeError(f"dtype must be torch.uint8, float32 or bfloat16, got {dtype}")
    if table.device.type != "cpu" or table.dtype != torch.int64:
        raise TypeError(f"table must be a CPU int64 tensor, got {table.dtype} on {table.device}")
    if table.dim() != 2 or table.shape[1] != 4:
        raise ValueError(f"table must be [B, 4] (offset, width, top, left), received shape {tuple(table.shape)}")
    patchsize = int(patchsize)
    if patchsize < 1:
        raise ValueError(f"patchsize must be positive, got {patchsize}")
    table = table.contiguous()
    off, width, top, left = table.unbind(1)
    end = off + ((top + (patchsize - 1)) * width + left + patchsize) * 3
    bad = (table < 0).any(dim=1) | (table[:, 1:] > 2 ** 24).any(dim=1) | (end > pool.numel())
    if bad.any():
        row = int(bad.nonzero()[0])
        o, w, t, l = table[row].tolist()
        if min(o, w, t, l) < 0:
            raise ValueError(f"table row {row} has a negative entry: offset {o}, width {w}, top {t}, left {l}")
        if max(w, t, l) > 2 ** 24:
            raise ValueError(f"table row {row}: width {w}, top {t} and left {l} must not exceed 2^24")
        raise ValueError(f"table row {row}: a {patchsize} x {patchsize} patch at top {t}, left {l} of the image of "
                         f"width {w} at byte {o} ends at byte {int(end[row])}, the pool has {pool.numel()}")
    return table, patchsize


def crop_patches_reference(pool, table, patchsize, dtype=torch.uint8):
    """`crop_patches` as tensor ops: one strided view of the pool per patch."""
    table, P = _check_crop(pool, table, patchsize, dtype)
    base = pool.storage_offset()
    rows = [pool.as_strided((P, P, 3), (3 * w, 3, 1), base + o + (t * w + l) * 3) for o, w, t, l in table.tolist()]
    if not rows:
        return torch.empty((0, P, P, 3), dtype=dtype, device=pool.device)
    return torch.stack(rows).to(dtype)


def crop_patches(pool, table, patchsize, dtype=torch.uint8):
    """pool: flat uint8, decoded images [H_i, W_i, 3] back to back; table: CPU int64 [B, 4], per patch the byte offset
    of the image's first pixel, the image width, top and left -> [B, P, P, 3] of `dtype` (uint8, float32 or bfloat16:
    the integers 0...255).  The table is checked here (no negative entry, every patch inside the pool; ValueError names
    the row) and then uploaded, one small copy.  One kernel on a device pool, bit-exact with `crop_patches_reference`,
    which a CPU pool takes."""
    if not pool.is_cuda:
        return crop_patches_reference(pool, table, patchsize, dtype)
    table, P = _check_crop(pool, table, patchsize, dtype)
    out = torch.empty((table.shape[0], P, P, 3), dtype=dtype, device=pool.device)
    dev_table = table.to(pool.device, non_blocking=True)
    with torch.cuda.device(pool.device):
        _lib.check(_lib.lib().tfc_crop_patches(pool.data_ptr(), pool.numel(), dev_table.data_ptr(), table.shape[0], P,
                                               DTYPE_CODE[dtype], out.data_ptr(), _lib.stream_ptr()))
    return out


# -------------------------------------------------------------------------------------------------------------------
# crops of resized images


def _check_scale_crop(pool, table, patchsize, dtype):
    if pool.dtype != torch.uint8:
        raise TypeError(f"pool must be uint8, got {pool.dtype}")
    if pool.dim() != 1 or not pool.is_contiguous():
        raise ValueError(f"pool must be a flat contiguous tensor, received shape {tuple(pool.shape)}")
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"dtype must be torch.float32 or bfloat16 (the values are not integers), got {dtype}")
    if table.device.type != "cpu" or table.dtype != torch.int64:
        raise TypeError(f"table must be a CPU int64 tensor, got {table.dtype} on {table.device}")
    if table.dim() != 2 or table.shape[1] != 7:
        raise ValueError("table must be [B, 7] (offset, width, height, resized width, resized height, top, left), "
                         f"received shape {tuple(table.shape)}")
    patchsize = int(patchsize)
    if patchsize < 1 or patchsize > 2 ** 15:
        raise ValueError(f"patchsize must be in [1, 2^15], got {patchsize}")
    if table.shape[0] * patchsize * patchsize * 3 >= 2 ** 31:
        raise ValueError(f"{table.shape[0]} patches of {patchsize} x {patchsize} x 3 values: one call takes fewer than "
                         "2^31 values")
    table = table.contiguous()
    off, width, height, new_width, new_height, top, left = table.unbind(1)
    sizes = table[:, 1:5]
    negative = (table < 0).any(dim=1)
    # a negative entry is reported as such; the products below are formed for the other rows only
    out_of_range = ~negative & ((sizes < 1) | (sizes > 2 ** 24)).any(dim=1)
    sound = ~negative & ~out_of_range
    outside = sound & ((top + patchsize > new_height) | (left + patchsize > new_width))
    end = off + 3 * width.clamp(0, 2 ** 24) * height.clamp(0, 2 ** 24)
    past = sound & ((off > pool.numel()) | (end > pool.numel()))
    bad = negative | out_of_range | outside | past
    if bad.any():
        row = int(bad.nonzero()[0])
        o, w, h, ow, oh, t, l = table[row].tolist()
        if negative[row]:
            raise ValueError(f"table row {row} has a negative entry: offset {o}, width {w}, height {h}, resized width "
                             f"{ow}, resized height {oh}, top {t}, left {l}")
        if out_of_range[row]:
            raise ValueError(f"table row {row}: width {w}, height {h}, resized width {ow} and resized height {oh} must "
                             "be in [1, 2^24]")
        if outside[row]:
            raise ValueError(f"table row {row}: a {patchsize} x {patchsize} patch at top {t}, left {l} does not fit the "
                             f"resized image of {oh} x {ow}")
        raise ValueError(f"table row {row}: the {h} x {w} image at byte {o} ends at byte {int(end[row])}, the pool has "
                         f"{pool.numel()}")
    return table, patchsize


def scale_crop_patches_reference(pool, table, patchsize, dtype=torch.float32):
    """`scale_crop_patches` as tensor ops, one float32 operation per line of the definition (no lerp or addcmul, which
    may fuse): what the kernel is bit-identical to."""
    table, P = _check_scale_crop(pool, table, patchsize, dtype)
    f32 = torch.float32
    off, width, height, new_width, new_height, top, left = table.unbind(1)
    steps = torch.arange(P, dtype=torch.int64)

    def axis(size, new_size, first):
        scale = size.to(f32) / new_size.to(f32)
        pos = (first[:, None] + steps).to(f32) * scale[:, None]                   # [B, P]
        low_f = torch.minimum(torch.floor(pos), (size - 1).to(f32)[:, None])
        low = low_f.to(torch.int64)
        high = torch.minimum(low + 1, (size - 1)[:, None])
        return low, high, pos - low_f

    y0, y1, wy = axis(height, new_height, top)
    x0, x1, wx = axis(width, new_width, left)
    channel = torch.arange(3, dtype=torch.int64)

    def pixels(y, x):
        at = off[:, None, None] + (y[:, :, None] * width[:, None, None] + x[:, None, :]) * 3      # [B, P, P]
        return pool[(at[..., None] + channel).to(pool.device)].to(f32)

    wx = wx[:, None, :, None].to(pool.device)
    wy = wy[:, :, None, None].to(pool.device)
    tl, tr, bl, br = pixels(y0, x0), pixels(y0, x1), pixels(y1, x0), pixels(y1, x1)
    upper = tl + (tr - tl) * wx
    lower = bl + (br - bl) * wx
    return (upper + (lower - upper) * wy).to(dtype)


def scale_crop_patches(pool, table, patchsize, dtype=torch.float32):
    """B patches [P, P, 3] of bilinearly resized images, computed from the decoded images: the resized images never
    exist (TF1 `resize_bilinear`, align_corners=False, half_pixel_centers=False, as `tf.image.resize_images` of
    models/hific/model.py:346 runs it; the definition is stated in include/tfc_hip.h).

    pool: flat uint8, decoded images [H_i, W_i, 3] back to back; table: CPU int64 [B, 7], per patch the byte offset of
    the image's first pixel, its width W and height H, the resized width OW and height OH, and top and left IN THE
    RESIZED IMAGE -> [B, P, P, 3] of `dtype` (float32, or bfloat16: the float32 value rounded to nearest even).  The
    table is checked here (no negative entry, the four sizes in [1, 2^24], the patch inside the resized image, the
    image inside the pool; ValueError names the row) and then uploaded, one small copy.  One kernel on a device pool,
    bit-exact with `scale_crop_patches_reference`, which a CPU pool takes."""
    if not pool.is_cuda:
        return scale_crop_patches_reference(pool, table, patchsize, dtype)
    table, P = _check_scale_crop(pool, table, patchsize, dtype)
    out = torch.empty((table.shape[0], P, P, 3), dtype=dtype, device=pool.device)
    dev_table = table.to(pool.device, non_blocking=True)
    with torch.cuda.device(pool.device):
        _lib.check(_lib.lib().tfc_scale_crop_patches(pool.data_ptr(), pool.numel(), dev_table.data_ptr(),
                                                     table.shape[0], P, DTYPE_CODE[dtype], out.data_ptr(),
                                                     _lib.stream_ptr()))
    return out


# -------------------------------------------------------------------------------------------------------------------
# Keras Adam


def keras_adam_constants(lr, beta_1, beta_2, epsilon, step):
    """-> (alpha, c1, c2, eps): float64 arithmetic on the host, each rounded to float32 once (returned as Python floats
    that float32 holds exactly)."""
    step = int(step)
    if step < 1:
        raise ValueError(f"step counts from 1, got {step}")
    alpha = float(lr) * math.sqrt(1.0 - float(beta_2) ** step) / (1.0 - float(beta_1) ** step)
    return tuple(float(np.float32(v)) for v in (alpha, 1.0 - float(beta_1), 1.0 - float(beta_2), float(epsilon)))


def _check_adam(params, grads, ms, vs):
    params, grads, ms, vs = list(params), list(grads), list(ms), list(vs)
    if not len(params) == len(grads) == len(ms) == len(vs):
        raise ValueError("params, grads, ms and vs must have the same length")
    for k, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        for name, t in (("parameter", p), ("gradient", g), ("exp_avg", m), ("exp_avg_sq", v)):
            if t.dtype != torch.float32:
                raise TypeError(f"keras_adam: {name} {k} must be float32, got {t.dtype}")
            if not t.is_contiguous():
                raise ValueError(f"keras_adam: {name} {k} must be contiguous")
            if t.shape != p.shape or t.device != p.device:
                raise ValueError(f"keras_adam: {name} {k} has shape {tuple(t.shape)} on {t.device}, the parameter "
                                 f"{tuple(p.shape)} on {p.device}")
    return params, grads, ms, vs


@torch.no_grad()
def keras_adam_reference(params, grads, ms, vs, *, lr, beta_1, beta_2, epsilon, step):
    """The float32 twin of `keras_adam`: separate tensor ops in the order of the definition (no addcmul or lerp, which
    may fuse), in place on params, ms and vs.  The square root is taken in float64 and rounded to float32, which is the
    correctly rounded float32 root (53 bits are more than the 2 * 24 + 2 at which the second rounding cannot matter);
    torch's vectorised float32 `sqrt` on CPU tensors is not correctly rounded (torch 2.10 with AVX-512: 0.7 % of
    random inputs one unit off against numpy), its sum, difference, product and quotient are."""
    params, grads, ms, vs = _check_adam(params, grads, ms, vs)
    alpha, c1, c2, eps = keras_adam_constants(lr, beta_1, beta_2, epsilon, step)
    for p, g, m, v in zip(params, grads, ms, vs):
        m.copy_(m + (g - m) * c1)
        v.copy_(v + (g * g - v) * c2)
        root = torch.sqrt(v.to(torch.float64)).to(torch.float32)
        p.copy_(p - (m * alpha) / (root + eps))


@torch.no_grad()
def keras_adam(params, grads, ms, vs, *, lr, beta_1, beta_2, epsilon, step, skip=None):
    """One Keras Adam step, in place.  Device tensors take one tfc_keras_adam launch per KERAS_ADAM_CAPACITY tensors
    (all on one device), CPU tensors `keras_adam_reference`.  `skip`: an int32 tensor of one element on the tensors'
    device, or None; while it is nonzero nothing is written.  Nothing here waits for the device."""
    params, grads, ms, vs = _check_adam(params, grads, ms, vs)
    if not params:
        return
    device = params[0].device
    if any(p.device != device for p in params):
        raise ValueError("keras_adam: all tensors of one call must be on one device")
    if skip is not None:
        if skip.dtype != torch.int32 or skip.numel() != 1:
            raise TypeError("keras_adam: skip must be an int32 tensor of one element")
        if skip.device != device:
            raise ValueError(f"keras_adam: skip is on {skip.device}, the tensors on {device}")
    if device.type != "cuda":
        if skip is None or int(skip) == 0:
            keras_adam_reference(params, grads, ms, vs, lr=lr, beta_1=beta_1, beta_2=beta_2, epsilon=epsilon, step=step)
        return
    alpha, c1, c2, eps = keras_adam_constants(lr, beta_1, beta_2, epsilon, step)
    lib = _lib.lib()
    with torch.cuda.device(device):
        stream = _lib.stream_ptr()
        for at in range(0, len(params), KERAS_ADAM_CAPACITY):
            part = slice(at, at + KERAS_ADAM_CAPACITY)
            n = len(params[part])
            ptrs = [(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts[part]]) for ts in (params, grads, ms, vs)]
            numels = (ctypes.c_int64 * n)(*[p.numel() for p in params[part]])
            _lib.check(lib.tfc_keras_adam(*ptrs, numels, n, alpha, c1, c2, eps,
                                          None if skip is None else skip.data_ptr(), stream))
    # written through raw pointers: tell autograd, and the caches keyed on a tensor's version (layers/cached.py)
    torch.autograd.graph.increment_version(params + ms + vs)
